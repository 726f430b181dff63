"""Host side of temporal reprojection, without a GPU: pt_reproject_host and
pt_denoise_var_plane_host (the header code the kernels compile,
csrc/pt_denoise.h) against the independent numpy-float32 restatements of
tests/temporal_ref.py, bit for bit; the no-history branches; the argument
checks; and a one-pixel camera shift that must read the neighbour's history."""
import ctypes
import subprocess

import numpy as np
import pytest

import denoise_var_ref as V
import native
import ptamd
import scenes
import temporal_ref as T
from support import same

PT_OK, PT_ERR_INVALID = 0, -1
F = np.float32
CUR = scenes.DEFAULT_CAMERA                        # (0, 0, 5) looking down -z at the plane z = 0
AWAY = np.array(CUR, F)
AWAY[6] = 1.0                                      # the same place, looking the other way
# previous camera -> the no-history branches its pixels can reach, beside the misses of the guide
CAMERAS = {
    "identical": (CUR, {"miss", "no_valid"}),
    "orbit2": (T.rotate_y(CUR, -2.0), {"miss", "no_valid"}),
    "away": (AWAY, {"miss", "behind"}),
    "orbit60": (T.rotate_y(CUR, -60.0), {"miss", "outside", "no_valid"}),
}
SIZES = [(16, 16), (37, 23), (64, 48)]


def test_symbols_and_defaults():
    L = ptamd.lib()
    for name in ("pt_temporal_default_params", "pt_reproject", "pt_reproject_host", "pt_temporal_advance",
                 "pt_temporal_reset", "pt_temporal_info", "pt_temporal_device_ptr", "pt_read_temporal",
                 "pt_temporal_denoise", "pt_denoise_var_plane_host"):
        assert hasattr(L, name), name
        assert name in ptamd.EXPORTS
    assert ptamd.PT_OPT_SEED_BASE == 29
    assert L.pt_abi_version() == 3
    p = ptamd.temporal_default_params()
    assert (p.max_history, p.alpha_min, p.normal_min, p.depth_rel) == (64, F(0.0), F(0.5), F(0.05))
    assert (p.max_history, p.alpha_min, p.normal_min, p.depth_rel) == tuple(
        F(x) if k else x for k, x in enumerate(T.DEFAULTS))
    assert L.pt_temporal_default_params(None) == PT_ERR_INVALID


def test_make_inputs_hold_every_hostile_case():
    W, H = 37, 23
    d = T.make_inputs(W, H, 5, CUR, CAMERAS["orbit2"][0])
    hc, hm, hl, hg = d["history"]
    assert np.any(d["guide"][..., 3] >= 1e30) and np.any(d["guide"][..., 3] < 1e30)      # a block of misses
    assert np.any(hg[..., 0] == F(0.6)) and np.any(hg[..., 2] == F(1.0))                  # two normal regions
    t = hg[..., 3]
    assert np.any(t[(3 * H) // 4:] > F(1.15) * t[:(3 * H) // 4].max())                    # the depth step
    assert np.any(hl == 0) and np.any(hl > 64) and np.any((hl > 0) & (hl < 64))
    assert np.any(d["fire"]) and d["color"][d["fire"], :3].max() > 10.0                   # fireflies
    for m in (d["moments"], hm):
        assert np.any(m[..., 1] < m[..., 0] * m[..., 0])                                  # m2 < m1 * m1 by an ulp
    *_, info = T.reproject(CUR, CAMERAS["orbit2"][0], W, H, 2, d["color"], d["moments"], d["guide"], d["history"])
    assert all(info["taps"][k] > 0 for k in (1, 2, 3, 4)), info                            # one to three valid taps


@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("W,H", SIZES)
def test_host_matches_restatement(W, H, cam):
    prev, branches = CAMERAS[cam]
    n = 2
    d = T.make_inputs(W, H, 100 * W + H, CUR, prev)
    for params in (None, (8, 0.25, 0.9, 0.02)):
        got = ptamd.reproject_host(CUR, prev, W, H, n, d["color"], d["moments"], d["guide"], d["history"], params)
        *ref, info = T.reproject(CUR, prev, W, H, n, d["color"], d["moments"], d["guide"], d["history"],
                                 T.DEFAULTS if params is None else params)
        for g, r, what in zip(got, ref, ("colour", "moments", "length", "variance")):
            assert np.all(np.isfinite(g)), what
            same(g, r, f"{cam} {W}x{H} {params}: {what}")
        taken = {k for k in ("miss", "behind", "outside", "no_valid") if info[k] > 0}
        assert taken == branches, info
        assert (info["blended"] > 0) == (cam != "away"), info
        same(got[0][..., 3], d["color"][..., 3], "alpha passes through")
        cap = 64 if params is None else params[0]
        assert got[2].min() == n and got[2].max() <= cap + n
        if cam != "away":
            assert got[2].max() == cap + n                                 # a history longer than max_history is capped


def test_null_history_gives_the_new_frame():
    W, H, n = 37, 23, 3
    d = T.make_inputs(W, H, 11, CUR, CUR)
    c, m, l, v = ptamd.reproject_host(CUR, CAMERAS["orbit2"][0], W, H, n, d["color"], d["moments"], d["guide"], None)
    same(c, d["color"], "colour")
    same(m, d["moments"], "moments")
    assert np.all(l == F(n))
    m1, m2 = d["moments"][..., 0], d["moments"][..., 1]
    same(v, np.maximum(F(0), m2 - m1 * m1) / F(n - 1), "variance of the mean")
    assert np.any(v == 0) and np.any(v > 0)
    ref = T.reproject(CUR, CUR, W, H, n, d["color"], d["moments"], d["guide"], None)
    same(v, ref[3], "variance against the restatement")
    # one sample: the divisor is fmax(n - 1, 1) = 1
    v1 = ptamd.reproject_host(CUR, CUR, W, H, 1, d["color"], d["moments"], d["guide"], None)[3]
    same(v1, np.maximum(F(0), m2 - m1 * m1), "variance at n = 1")


def test_argument_checks():
    L = ptamd.lib()
    W, H = 16, 16
    d = T.make_inputs(W, H, 1, CUR, CUR)
    arr = {k: np.ascontiguousarray(d[k], F).reshape(-1) for k in ("color", "moments", "guide")}
    hist = [np.ascontiguousarray(a, F).reshape(-1) for a in d["history"]]
    outs = [np.zeros(W * H * k, F) for k in (4, 2, 1, 1)]
    cam = np.ascontiguousarray(CUR, F)

    def images(**over):
        ptrs = [arr["color"], arr["moments"], arr["guide"], *hist, *outs]
        im = ptamd.ReprojectImages(*[a.ctypes.data for a in ptrs])
        for k, v in over.items():
            setattr(im, k, v)
        return im

    def call(n=2, w=W, h=H, params=None, cur=cam.ctypes.data, prev=cam.ctypes.data, **over):
        p = None if params is None else ctypes.byref(ptamd.TemporalParams(*params))
        im = images(**over)
        return L.pt_reproject_host(cur, prev, w, h, n, ctypes.byref(im), p)

    assert call() == PT_OK
    for n in (0, 65537):
        assert call(n=n) == PT_ERR_INVALID
    for n in (1, 65536):
        assert call(n=n) == PT_OK
    for w, h in [(0, 16), (16, 0), (-1, 16)]:
        assert call(w=w, h=h) == PT_ERR_INVALID
    assert call(cur=None) == PT_ERR_INVALID and call(prev=None) == PT_ERR_INVALID
    assert L.pt_reproject_host(cam.ctypes.data, cam.ctypes.data, W, H, 2, None, None) == PT_ERR_INVALID
    for k in ("color", "moments", "guide", "out_color", "out_moments", "out_length", "out_variance"):
        assert call(**{k: None}) == PT_ERR_INVALID, k
    for k in ("hist_color", "hist_moments", "hist_length", "hist_guide"):          # all four or none
        assert call(**{k: None}) == PT_ERR_INVALID, k
    assert call(hist_color=None, hist_moments=None, hist_length=None, hist_guide=None) == PT_OK
    assert call(out_color=arr["color"].ctypes.data) == PT_ERR_INVALID              # an output is an input
    assert call(out_length=hist[2].ctypes.data) == PT_ERR_INVALID
    assert call(out_variance=outs[2].ctypes.data) == PT_ERR_INVALID                # two outputs alike
    inf, nan = float("inf"), float("nan")
    for bad in [(0, 0.0, 0.5, 0.05), (65537, 0.0, 0.5, 0.05), (64, -0.1, 0.5, 0.05), (64, 1.1, 0.5, 0.05),
                (64, nan, 0.5, 0.05), (64, 0.0, -1.1, 0.05), (64, 0.0, 1.1, 0.05), (64, 0.0, nan, 0.05),
                (64, 0.0, 0.5, 0.0), (64, 0.0, 0.5, -1.0), (64, 0.0, 0.5, inf), (64, 0.0, 0.5, nan)]:
        assert call(params=bad) == PT_ERR_INVALID, bad
    for good in [(1, 0.0, -1.0, 1e-6), (65536, 1.0, 1.0, 1e6)]:
        assert call(params=good) == PT_OK, good
    with pytest.raises(ptamd.PTError):
        ptamd.reproject_host(CUR, CUR, W, H, 2, d["color"], d["moments"][:-1], d["guide"])


@pytest.mark.parametrize("hlen", [5, 100])
@pytest.mark.parametrize("W,H", SIZES)
def test_one_pixel_shift_reads_the_neighbour(W, H, hlen):
    """The camera at (0, 0, 5) looks down -z with up +y, so right =
    normalize(cross(dir, -up)) = (-1, 0, 0) and pixel x looks at world X =
    D * ndcX * tan_fov * aspect, D = 5: neighbouring pixels are s = 2 D tan_fov
    aspect / W apart on the plane.  A previous camera at pos + right * s sees
    the point of pixel x at v.x = X + s, hence sx = ndcX + 2 / W and fx = x + 1:
    every pixel with x + 1 inside the frame reads the history of its right-hand
    neighbour (x + 1, y).  fx is x + 1 up to roundings below 64 * 2^-18 of a
    pixel, which weigh the tap beside it by as much: 1e-3 of the history's
    value range bounds the difference."""
    n, max_history = 2, 64
    pos, cdir, right, up, tan_fov = T.cam_basis(CUR)
    assert np.array_equal(right, np.array([-1, 0, 0], F))
    s = 2.0 * 5.0 * float(tan_fov) * (W / H) / W
    prev = np.array(CUR, F)
    prev[0:3] = (pos.astype(np.float64) + right.astype(np.float64) * s).astype(F)
    rng = np.random.default_rng(W + H)
    color = rng.uniform(0.0, 1.0, (H, W, 4)).astype(F)
    hcolor = rng.uniform(0.0, 1.0, (H, W, 4)).astype(F)                    # value range 1
    lum, hlum = V.lum(color), V.lum(hcolor)
    moments = np.stack([lum, lum * lum + F(0.1)], -1).astype(F)
    hmoments = np.stack([hlum, hlum * hlum + F(0.1)], -1).astype(F)        # within [0, 1.1]
    guide, hguide = T.plane_guide(CUR, W, H), T.plane_guide(prev, W, H)
    assert np.all(guide[..., 3] < 1e30) and np.all(hguide[..., 3] < 1e30)
    hlength = np.full((H, W), hlen, F)
    c, m, l, v = ptamd.reproject_host(CUR, prev, W, H, n, color, moments, guide, (hcolor, hmoments, hlength, hguide))
    N = min(hlen, max_history)
    assert np.all(l[:, :W - 1] == F(N + n))                                # exactly
    a = n / (N + n)
    hc, hm = hcolor[:, 1:, :3].astype(np.float64), hmoments[:, 1:].astype(np.float64)
    want_c = hc + (color[:, :W - 1, :3].astype(np.float64) - hc) * a
    want_m = hm + (moments[:, :W - 1].astype(np.float64) - hm) * a
    assert np.abs(c[:, :W - 1, :3] - want_c).max() <= 1e-3 * 1.0
    assert np.abs(m[:, :W - 1] - want_m).max() <= 1e-3 * 1.1
    # the last column's source x + 1 = W lies outside the frame (fx < W fails or only the tap W - 1 remains)
    assert np.all((l[:, W - 1] == F(n)) | (l[:, W - 1] == F(N + n)))


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("W,H", SIZES)
def test_filter_from_a_variance_plane(W, H, iterations):
    n = 8
    rgba, moments, guide = V.make_images(W, H, seed=100 * W + H, n_samples=n)
    rng = np.random.default_rng(W * H)
    plane = (rng.uniform(0.0, 2.0, (H, W)) * (rng.uniform(size=(H, W)) > 0.2)).astype(F)   # a fifth of it exactly 0
    params = (iterations, 1.5, 0.35, 0.25)
    got = ptamd.denoise_var_plane_host(rgba, plane, guide, W, H, params)
    assert np.all(np.isfinite(got))
    same(got, T.atrous_var_plane(rgba, plane, guide, W, H, params), "plane filter")
    # pt_denoise_var_host is the plane filter after its own var0, and still equals its restatement
    host = ptamd.denoise_var_host(rgba, moments, n, guide, W, H, params)
    same(host, V.atrous_var(rgba, moments, n, guide, W, H, params), "pt_denoise_var_host")
    same(host, ptamd.denoise_var_plane_host(rgba, V.var_of_mean(moments, n), guide, W, H, params), "var0 then plane")


def test_filter_plane_rejects_bad_arguments():
    L = ptamd.lib()
    W, H = 16, 16
    rgba, _, guide = V.make_images(W, H, seed=1)
    a, g = (np.ascontiguousarray(x, F).reshape(-1) for x in (rgba, guide))
    v, out = np.ones(W * H, F), np.zeros(W * H * 4, F)
    assert L.pt_denoise_var_plane_host(a.ctypes.data, v.ctypes.data, g.ctypes.data, W, H, None, out.ctypes.data) == PT_OK
    assert L.pt_denoise_var_plane_host(a.ctypes.data, None, g.ctypes.data, W, H, None, out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_denoise_var_plane_host(a.ctypes.data, v.ctypes.data, g.ctypes.data, 0, H, None, out.ctypes.data) == PT_ERR_INVALID
    bad = ctypes.byref(ptamd.DenoiseVarParams(7, 1.5, 0.35, 0.25))
    assert L.pt_denoise_var_plane_host(a.ctypes.data, v.ctypes.data, g.ctypes.data, W, H, bad, out.ctypes.data) == PT_ERR_INVALID
    with pytest.raises(ptamd.PTError):
        ptamd.denoise_var_plane_host(rgba, v[:-1], guide, W, H)


def test_stand_alone_check_program(tmp_path):
    """tests/temporal_check.cpp (the program sanitizer runs use), built plainly
    against the library and run."""
    exe = native.against_library("temporal_check", tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.startswith("ok:")
