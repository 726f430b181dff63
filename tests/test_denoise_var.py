"""Host side of the variance-guided filter, without a GPU: pt_denoise_var_host
(the header code the kernels compile, csrc/pt_denoise.h) against the
independent numpy-float32 restatement of tests/denoise_var_ref.py, bit for
bit, the argument checks, and the zero-variance limit."""
import ctypes
import subprocess

import numpy as np
import pytest

import denoise_var_ref as R
import native
import ptamd
from support import bits, same

PT_OK, PT_ERR_INVALID = 0, -1


def test_symbols_and_defaults():
    L = ptamd.lib()
    for name in ("pt_moments_device_ptr", "pt_read_moments", "pt_denoise_var_default_params", "pt_denoise_var",
                 "pt_denoise_var_host"):
        assert hasattr(L, name), name
        assert name in ptamd.EXPORTS
    assert ptamd.PT_OPT_MOMENTS == 27
    assert L.pt_abi_version() == 3
    p = ptamd.denoise_var_default_params()
    assert (p.iterations, p.sigma_lum, p.sigma_normal, p.sigma_depth) == tuple(
        np.float32(x) if k else x for k, x in enumerate(R.DEFAULTS))
    assert L.pt_denoise_var_default_params(None) == PT_ERR_INVALID


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("W,H", [(16, 16), (37, 23), (64, 48)])
def test_host_filter_matches_restatement(W, H, iterations):
    n = 8
    rgba, moments, guide = R.make_images(W, H, seed=100 * W + H, n_samples=n)
    # what the images are there to exercise
    var0 = R.var_of_mean(moments, n)
    assert np.any(moments[..., 1] < moments[..., 0] * moments[..., 0])       # m2 < m1 * m1 by rounding
    assert np.any(var0 == 0) and np.any(var0 > 1.0) and np.any(guide[..., 3] >= 1e30)
    params = (iterations, 1.5, 0.35, 0.25)
    got = ptamd.denoise_var_host(rgba, moments, n, guide, W, H, params)
    ref = R.atrous_var(rgba, moments, n, guide, W, H, params)
    assert np.all(np.isfinite(got))
    same(got, ref, "against the restatement")
    assert np.array_equal(bits(got[..., 3]), bits(rgba[..., 3]))           # alpha passes through
    assert not np.array_equal(bits(got[..., :3]), bits(rgba[..., :3]))     # ... and the filter filters


def test_host_filter_default_params_and_sample_count():
    W, H = 37, 23
    rgba, moments, guide = R.make_images(W, H, seed=7)
    got = ptamd.denoise_var_host(rgba, moments, 8, guide, W, H, None)
    assert np.array_equal(bits(got), bits(R.atrous_var(rgba, moments, 8, guide, W, H, R.DEFAULTS)))
    # the sample count scales the variance of the mean: another n, another image
    other = ptamd.denoise_var_host(rgba, moments, 32, guide, W, H, None)
    assert np.array_equal(bits(other), bits(R.atrous_var(rgba, moments, 32, guide, W, H, R.DEFAULTS)))
    assert not np.array_equal(bits(other), bits(got))


def test_host_filter_rejects_bad_arguments():
    L = ptamd.lib()
    W, H = 16, 16
    rgba, moments, guide = R.make_images(W, H, seed=1)
    a, m, g = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (rgba, moments, guide))
    out = np.zeros(W * H * 4, np.float32)

    def call(params=None, n=8, w=W, h=H, a_=a.ctypes.data, m_=m.ctypes.data, g_=g.ctypes.data, o_=out.ctypes.data):
        p = None if params is None else ctypes.byref(ptamd.DenoiseVarParams(*params))
        return L.pt_denoise_var_host(a_, m_, n, g_, w, h, p, o_)

    assert call() == PT_OK
    for n in (0, 1):                                                   # no variance of the mean below 2 samples
        assert call(n=n) == PT_ERR_INVALID
    assert call(n=2) == PT_OK
    for w, h in [(0, 16), (16, 0), (-1, 16)]:
        assert call(w=w, h=h) == PT_ERR_INVALID
    for null in ("a_", "m_", "g_", "o_"):
        assert call(**{null: None}) == PT_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    for bad in [(0, 1.5, 0.35, 0.25), (7, 1.5, 0.35, 0.25), (-1, 1.5, 0.35, 0.25),
                (5, 0.0, 0.35, 0.25), (5, -1.0, 0.35, 0.25), (5, inf, 0.35, 0.25), (5, nan, 0.35, 0.25),
                (5, 1.5, 0.0, 0.25), (5, 1.5, nan, 0.25), (5, 1.5, 0.35, 0.0), (5, 1.5, 0.35, inf),
                (5, 1e-30, 0.35, 0.25), (5, 1.5, 1e-30, 0.25), (5, 1.5, 0.35, 1e30)]:   # squares 0 or inf
        assert call(params=bad) == PT_ERR_INVALID, bad
    for it in (1, 6):
        assert call(params=(it, 1.5, 0.35, 0.25)) == PT_OK
    with pytest.raises(ptamd.PTError):
        ptamd.denoise_var_host(rgba, moments[:-1], 8, guide, W, H)     # the wrapper's size check


@pytest.mark.parametrize("iterations", [1, 5])
def test_zero_variance_frame_comes_back_unchanged(iterations):
    """With zero variance everywhere den is 1e-6, so a tap whose luminance
    differs from the centre's by 0.01 or more weighs exp(-1e4) = 0 exactly and
    the centre tap alone remains: the pixel comes back as (h * c) / h, h = 9/64,
    which float32 rounds to c or, for some c, to the float next to it."""
    W, H = 37, 23
    rng = np.random.default_rng(3)
    grey = (rng.permutation(W * H).astype(np.float32) * np.float32(0.01)).reshape(H, W)   # every luminance its own
    rgba = np.repeat(grey[..., None], 4, axis=-1).astype(np.float32)
    rgba[..., 3] = 1.0
    lum = R.lum(rgba)
    flat = np.sort(lum.reshape(-1))
    assert np.min(np.diff(flat)) > 5e-3
    moments = np.stack([lum, lum * lum], axis=-1).astype(np.float32)
    _, _, guide = R.make_images(W, H, seed=9)
    got = ptamd.denoise_var_host(rgba, moments, 8, guide, W, H, (iterations, 1.5, 0.35, 0.25))
    assert np.all(np.isfinite(got))
    # the centre tap alone: each pass is (h * c) / h in float32, which is c or its neighbour
    h = np.float32(0.375) * np.float32(0.375)
    want = rgba.copy()
    for _ in range(iterations):
        want[..., :3] = (h * want[..., :3]) / h
    assert np.array_equal(bits(got), bits(want))
    ulps = np.abs(bits(got[..., :3]).astype(np.int64) - bits(rgba[..., :3]).astype(np.int64))
    assert int(ulps.max()) <= iterations and np.count_nonzero(ulps) < 0.2 * ulps.size
    # ... and a flat zero-variance frame (every neighbour alike) stays finite too
    flat_rgba = np.full((H, W, 4), 0.5, np.float32)
    fl = R.lum(flat_rgba)
    fm = np.stack([fl, fl * fl], axis=-1).astype(np.float32)
    out = ptamd.denoise_var_host(flat_rgba, fm, 8, guide, W, H, (iterations, 1.5, 0.35, 0.25))
    assert np.all(np.isfinite(out)) and np.allclose(out, 0.5, rtol=1e-6)


def test_stand_alone_check_program(tmp_path):
    """tests/denoise_var_check.cpp (the program sanitizer runs use), built
    plainly against the library and run."""
    exe = native.against_library("denoise_var_check", tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.startswith("ok:")
