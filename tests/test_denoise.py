"""Host side of the guide image and the a-trous denoiser, without a GPU:
pt_guide_ray and pt_denoise_host (the header code the kernels compile,
csrc/pt_denoise.h) against the independent numpy-float32 restatements of
tests/denoise_ref.py, bit for bit, and the argument checks."""
import ctypes

import numpy as np
import pytest

import denoise_ref as R
import ptamd
import scenes
from support import bits, same

PT_ERR_INVALID = -1


@pytest.mark.parametrize("cam", [scenes.DEFAULT_CAMERA, scenes.camera((3, 2, 4))], ids=["default", "from_3_2_4"])
def test_guide_ray_matches_restatement(cam):
    W, H = 64, 48
    o_ref, d_ref = R.guide_rays(cam, W, H)
    got = np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            o, d = ptamd.guide_ray(cam, W, H, x, y)
            assert np.array_equal(bits(o), bits(o_ref))
            got[y, x] = d
    same(got, d_ref, "against the restatement")
    if cam is scenes.DEFAULT_CAMERA:   # the column the wide walk hands to the exact walk
        assert np.all(got[:, W // 2, 0] == 0.0)


def test_guide_ray_rejects_bad_pixels():
    L = ptamd.lib()
    cam = np.ascontiguousarray(scenes.DEFAULT_CAMERA, np.float32)
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for w, h, x, y in [(0, 4, 0, 0), (4, 0, 0, 0), (4, 4, 4, 0), (4, 4, 0, 4), (4, 4, -1, 0)]:
        assert L.pt_guide_ray(cam.ctypes.data, w, h, x, y, o.ctypes.data, d.ctypes.data) == PT_ERR_INVALID


@pytest.mark.parametrize("iterations", [1, 5, 6])
@pytest.mark.parametrize("W,H", [(67, 45), (20, 12), (1, 1)])
def test_host_filter_matches_restatement(W, H, iterations):
    rgba, guide = R.make_images(W, H, seed=100 * W + H)
    params = (iterations, 0.6, 0.35, 0.25)
    got = ptamd.denoise_host(rgba, guide, W, H, params)
    ref = R.atrous(rgba, guide, W, H, params)
    assert np.all(np.isfinite(got))
    same(got, ref, "against the restatement")
    assert np.array_equal(bits(got[..., 3]), bits(rgba[..., 3]))   # alpha passes through
    if (W, H) == (1, 1):
        assert np.array_equal(bits(got), bits(rgba))               # the centre tap alone


def test_host_filter_default_params():
    p = ptamd.denoise_default_params()
    assert (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth) == tuple(
        [R.DEFAULTS[0]] + [float(np.float32(v)) for v in R.DEFAULTS[1:]])
    rgba, guide = R.make_images(20, 12, seed=7)
    assert np.array_equal(bits(ptamd.denoise_host(rgba, guide, 20, 12)),
                          bits(ptamd.denoise_host(rgba, guide, 20, 12, R.DEFAULTS)))


def test_host_filter_edges_do_not_mix():
    """A hit next to a miss has weight 0: a constant colour per side of the
    miss block's border stays that constant."""
    W, H = 24, 16
    guide = np.zeros((H, W, 4), np.float32)
    guide[..., 2] = 1.0
    guide[..., 3] = 3.0
    guide[:, W // 2:] = np.array([0, 0, 0, 1e30], np.float32)
    rgba = np.ones((H, W, 4), np.float32)
    rgba[:, : W // 2, :3] = 0.25
    rgba[:, W // 2:, :3] = 4.0
    out = ptamd.denoise_host(rgba, guide, W, H, (5, 100.0, 0.35, 0.25))   # colour alone would blur it all
    assert np.array_equal(out, rgba)


@pytest.mark.parametrize("params", [
    (0, 0.6, 0.35, 0.25), (7, 0.6, 0.35, 0.25), (-1, 0.6, 0.35, 0.25),
    (5, 0.0, 0.35, 0.25), (5, 0.6, 0.0, 0.25), (5, 0.6, 0.35, 0.0),
    (5, -0.6, 0.35, 0.25), (5, 0.6, -0.35, 0.25), (5, 0.6, 0.35, -0.25),
    (5, float("nan"), 0.35, 0.25), (5, 0.6, float("nan"), 0.25), (5, 0.6, 0.35, float("nan")),
    (5, float("inf"), 0.35, 0.25), (5, 0.6, float("inf"), 0.25), (5, 0.6, 0.35, float("inf")),
    (5, 1e-30, 0.35, 0.25),   # sigma_color^2 underflows to 0: the centre tap would be 0 / 0
])
def test_bad_parameters_are_invalid(params):
    L = ptamd.lib()
    rgba, guide = R.make_images(4, 4, seed=1)
    out = np.zeros_like(rgba)
    p = ptamd.DenoiseParams(*params)
    rc = L.pt_denoise_host(rgba.ctypes.data, guide.ctypes.data, 4, 4, ctypes.byref(p), out.ctypes.data)
    assert rc == PT_ERR_INVALID, params
    assert L.pt_last_error()


def test_null_and_size_arguments_are_invalid():
    L = ptamd.lib()
    rgba, guide = R.make_images(4, 4, seed=1)
    out = np.zeros_like(rgba)
    assert L.pt_denoise_host(None, guide.ctypes.data, 4, 4, None, out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_denoise_host(rgba.ctypes.data, None, 4, 4, None, out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_denoise_host(rgba.ctypes.data, guide.ctypes.data, 4, 4, None, None) == PT_ERR_INVALID
    assert L.pt_denoise_host(rgba.ctypes.data, guide.ctypes.data, 0, 4, None, out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_denoise_default_params(None) == PT_ERR_INVALID
