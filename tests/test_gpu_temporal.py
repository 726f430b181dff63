"""GPU: temporal reprojection.  reproject_kernel against the host's run of the
same header code (pt_reproject_host) and the independent numpy restatement
(tests/temporal_ref.py), bit for bit; the loop of pt_temporal_advance against
a chain of seed-base renders and host reprojections; pt_temporal_denoise
against the host filter from the variance plane; what forgets the history;
the error paths; the pt_render flag; and what the history buys in error."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import ptamd
import scenes
import temporal_ref as T
from support import PKG, dev, mse, read_device, read_pfm, renderer, same, scene

pytestmark = pytest.mark.gpu

F = np.float32
PT_OK, PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 0, -1, -5
START = {"box": (0.0, 0.0, 5.0), "sphere": (3.0, 2.0, 4.0)}
SIZE = {"box": (64, 48), "sphere": (67, 45)}                  # edge tiles in both directions
CUR = scenes.DEFAULT_CAMERA
AWAY = np.array(CUR, F)
AWAY[6] = 1.0
PREV = {"identical": CUR, "orbit2": T.rotate_y(CUR, -2.0), "away": AWAY, "orbit60": T.rotate_y(CUR, -60.0)}


def _orbit(name, degrees):
    """scenes.camera of the scene's start position rotated about +y."""
    x, y, z = START[name]
    a = np.deg2rad(degrees)
    return scenes.camera((x * np.cos(a) + z * np.sin(a), y, z * np.cos(a) - x * np.sin(a)))


def _renderer(name, W=None, H=None, moments=1):
    w, h = SIZE[name]
    return renderer(scene(name), _orbit(name, 0), size=(W or w, H or h), options=[(ptamd.PT_OPT_MOMENTS, moments)])


def _device_reproject(r, cur, prev, W, H, n, color, moments, guide, history, params=None):
    ins = [dev(color), dev(moments), dev(guide)] + ([None] * 4 if history is None else [dev(a) for a in history])
    outs = [torch.full((H, W, k), -7.0, dtype=torch.float32, device="cuda") for k in (4, 2, 1, 1)]
    torch.cuda.synchronize()
    im = ptamd.ReprojectImages(*[None if t is None else t.data_ptr() for t in ins + outs])
    r.reproject(cur, prev, W, H, n, im, params)
    r.synchronize()
    got = [o.cpu().numpy() for o in outs]
    unchanged = [None if t is None else t.cpu().numpy() for t in ins]
    return (got[0], got[1], got[2][..., 0], got[3][..., 0]), unchanged


@pytest.mark.parametrize("cam", list(PREV))
@pytest.mark.parametrize("W,H", [(16, 16), (37, 23), (64, 48)])
def test_device_matches_host_and_restatement(W, H, cam):
    r = ptamd.Renderer(0)
    prev, n = PREV[cam], 2
    d = T.make_inputs(W, H, 100 * W + H, CUR, prev)
    for history, params in ((d["history"], None), (d["history"], (8, 0.25, 0.9, 0.02)), (None, None)):
        got, after = _device_reproject(r, CUR, prev, W, H, n, d["color"], d["moments"], d["guide"], history, params)
        host = ptamd.reproject_host(CUR, prev, W, H, n, d["color"], d["moments"], d["guide"], history, params)
        *ref, _ = T.reproject(CUR, prev, W, H, n, d["color"], d["moments"], d["guide"], history,
                              T.DEFAULTS if params is None else params)
        for g, h_, f_, what in zip(got, host, ref, ("colour", "moments", "length", "variance")):
            same(g, h_, f"{cam} {W}x{H} {params}: device against host, {what}")
            same(g, f_, f"{cam} {W}x{H} {params}: device against the restatement, {what}")
        ins = [d["color"], d["moments"], d["guide"]] + ([None] * 4 if history is None else list(history))
        for a, b in zip(after, ins):
            if b is not None:
                same(a, b, "an input image after the call")
        if history is None:
            same(got[0], d["color"], "null history: colour")
            assert np.all(got[2] == F(n))


def _frames(r, name, k, n):
    """Frame k of the loop rendered plainly on r: seed base k * n, camera k."""
    W, H = SIZE[name]
    cam = _orbit(name, 2 * k)
    r.set_camera(cam)
    r.set_option(ptamd.PT_OPT_SEED_BASE, k * n)
    r.clear()
    r.render(0, n)
    accum = r.read_accum().reshape(H, W, 4)
    moments, got_n = r.read_moments()
    assert got_n == n
    r.render_guide()
    return cam, accum, moments, r.read_guide()


@functools.lru_cache(maxsize=None)
def _loop(name, frames=8, n=2):
    """The loop on the device and its chain on the host; the asserts of the
    loop test are made here once, the other tests share the results."""
    W, H = SIZE[name]
    r, plain = _renderer(name), _renderer(name)
    hist, prev_cam, steps = None, None, []
    for k in range(frames):
        cam, accum, moments, guide = _frames(plain, name, k, n)
        want = ptamd.reproject_host(cam, cam if prev_cam is None else prev_cam, W, H, n, accum, moments, guide, hist)
        r.temporal_advance(cam, n)
        c, m, l = r.read_temporal()
        v = read_device(r, r.temporal_ptr(3), (H, W))
        for g, w_, what in zip((c, m, l, v), want, ("colour", "moments", "length", "variance")):
            same(g, w_, f"{name}: frame {k}, {what}")
        same(r.read_accum(), accum, f"{name}: frame {k}, the accumulation image")
        same(r.read_moments()[0], moments, f"{name}: frame {k}, the moments")
        assert r.temporal_info() == (k + 1, (k + 1) * n)
        hist, prev_cam = (want[0], want[1], want[2], guide), cam
        steps.append((cam, accum, moments, guide, want))
    return r, steps


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_the_loop_equals_the_host_chain(name):
    r, steps = _loop(name)
    assert len(steps) == 8
    # rendered frames through pt_reproject with device images, against the host and the restatement
    W, H = SIZE[name]
    (cam0, a0, m0, g0, w0), (cam1, a1, m1, g1, w1) = steps[0], steps[1]
    hist = (w0[0], w0[1], w0[2], g0)
    got, _ = _device_reproject(r, cam1, cam0, W, H, 2, a1, m1, g1, hist)
    *ref, info = T.reproject(cam1, cam0, W, H, 2, a1, m1, g1, hist)
    assert info["blended"] > 0 and info["miss"] > 0
    for g, w_, f_, what in zip(got, w1, ref, ("colour", "moments", "length", "variance")):
        same(g, w_, f"{name}: pt_reproject of rendered frames, {what}")
        same(g, f_, f"{name}: the restatement on rendered frames, {what}")


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_history_coverage(name):
    """After eight frames at 2 degree steps at least 0.90 of the last frame's
    first-hit pixels carry history (a float64 prototype on CPU frames gave
    0.964 for the box and 0.990 for the sphere at 64x64), and no length exceeds
    the 16 samples rendered."""
    _, steps = _loop(name)
    _, _, _, guide, want = steps[-1]
    hit = guide[..., 3] < 1e30
    share = np.count_nonzero(want[2][hit] > 2) / np.count_nonzero(hit)
    print(f"temporal {name}: {np.count_nonzero(hit)} first-hit pixels, {share:.4f} with history, "
          f"longest {want[2].max():.0f} samples")
    assert share >= 0.90
    assert want[2].max() <= 16 and want[2].min() == 2


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_temporal_denoise_equals_the_host_filter(name):
    W, H = SIZE[name]
    r, steps = _loop(name)
    _, _, _, guide, want = steps[-1]
    for params in (None, (2, 0.75, 0.5, 0.25)):
        ref = ptamd.denoise_var_plane_host(want[0], want[3], guide, W, H, params)
        same(ref, T.atrous_var_plane(want[0], want[3], guide, W, H, (4, 1.5, 1.0, 1.0) if params is None else params),
             f"{name}: host filter against the restatement")
        for staged in (0, 1):
            r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            same(r.temporal_denoise(params), ref, f"{name}: {params}, staged {staged}")
        dst = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert r.temporal_denoise(params, dst.data_ptr()) is None
        r.synchronize()
        same(dst.cpu().numpy(), ref, f"{name}: caller-owned destination")
    same(r.read_temporal()[0], want[0], "the temporal colour after the filter")
    L = ptamd.lib()
    assert L.pt_temporal_denoise(r._c, None, dst.data_ptr() + 4) == PT_ERR_INVALID          # misaligned
    assert L.pt_temporal_denoise(r._c, None, r.temporal_ptr(0)) == PT_ERR_INVALID           # onto its source
    assert L.pt_temporal_denoise(r._c, ctypes.byref(ptamd.DenoiseVarParams(7, 1.5, 1.0, 1.0)), None) == PT_ERR_INVALID


def test_disocclusion_on_the_box():
    """A second frame 60 degrees on: a face whose normal faces away from the
    previous camera (dot(n_p, P - pos_prev) >= 0) is perpendicular to every
    face that camera saw, so the normals' dot is 0 < normal_min = 0.5 and no
    tap is valid: out_len == n on every such pixel (a prototype had 600)."""
    name, n = "box", 2
    W, H = SIZE[name]
    r = _renderer(name)
    cam0, cam1 = _orbit(name, 0), _orbit(name, 60)
    r.temporal_advance(cam0, n)
    r.temporal_advance(cam1, n)
    _, _, length = r.read_temporal()
    guide = r.read_guide()
    pos, dirs = T.D.guide_rays(cam1, W, H)
    hit = guide[..., 3] < 1e30
    P = pos.astype(np.float64) + dirs.astype(np.float64) * guide[..., 3:4].astype(np.float64)
    away = hit & (np.sum(guide[..., :3].astype(np.float64) * (P - cam0[0:3].astype(np.float64)), axis=-1) >= 0)
    print(f"disocclusion: {np.count_nonzero(away)} pixels face away from the previous camera, "
          f"{np.count_nonzero(length[hit & ~away] > n)} of the other {np.count_nonzero(hit & ~away)} found history")
    assert np.count_nonzero(away) > 100
    assert np.all(length[away] == F(n))
    assert np.any(length > n)


def test_what_forgets_the_history():
    name, n = "box", 2
    W, H = SIZE[name]
    r = _renderer(name)
    cams = [_orbit(name, 2 * k) for k in range(3)]

    def warm():
        r.temporal_advance(cams[0], n)
        r.temporal_advance(cams[1], n)
        assert np.any(r.read_temporal()[2] > n) and r.temporal_info()[0] >= 2

    def forgotten(what):
        r.temporal_advance(cams[2], n)
        assert np.all(r.read_temporal()[2] == F(n)), what
        assert r.temporal_info() == (1, n), what

    warm()
    r.temporal_reset()
    assert r.temporal_info() == (0, 0) and r.temporal_ptr(0) is None
    forgotten("pt_temporal_reset")
    for what, act in (("scene upload", lambda: r.upload_scene(*scene(name))),
                      ("light upload", lambda: r.upload_lights(scenes.REFERENCE_LIGHT)),
                      ("pt_set_params", lambda: r.set_params(4, 3)),
                      ("resize", lambda: (r.resize_and_clear(W + 3, H), r.resize_and_clear(W, H)))):
        warm()
        act()
        forgotten(what)
    # the camera, a plain render, a dispatch and the progressive calls do not
    r.temporal_reset()
    warm()
    before = r.read_temporal()
    r.set_camera(cams[2])
    r.render(0, 3)
    r.dispatch(3)
    r.progressive_camera(cams[0])
    r.progressive_advance(2)
    r.render_guide()
    for a, b in zip(r.read_temporal(), before):
        same(a, b, "the temporal result after unrelated renders")
    r.temporal_advance(cams[2], n)
    assert np.any(r.read_temporal()[2] > 2 * n)                # two frames of history behind it
    assert r.temporal_info() == (3, 3 * n)


def test_error_paths():
    L = ptamd.lib()
    cam = np.ascontiguousarray(CUR, F)
    adv = lambda r_, n=2: L.pt_temporal_advance(r_._c, cam.ctypes.data, n)
    r = ptamd.Renderer(0)
    assert adv(r) == PT_ERR_INVALID                             # moments off
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    assert adv(r) == PT_ERR_INVALID                             # no scene
    r.upload_scene(*scene("box"))
    assert adv(r) == PT_ERR_INVALID                             # no lights
    r.upload_lights(scenes.REFERENCE_LIGHT)
    assert adv(r) == PT_ERR_INVALID                             # no frame
    assert L.pt_read_temporal(r._c, None, None, None) == PT_ERR_INVALID
    assert L.pt_temporal_denoise(r._c, None, None) == PT_ERR_INVALID
    r.resize_and_clear(20, 12)
    assert adv(r, 0) == PT_ERR_INVALID and adv(r, 65537) == PT_ERR_INVALID
    assert L.pt_temporal_advance(r._c, None, 2) == PT_ERR_INVALID
    assert adv(r) == PT_OK
    assert r.read_temporal()[0].shape == (12, 20, 4)
    r.set_option(ptamd.PT_OPT_MOMENTS, 0)
    assert adv(r) == PT_ERR_INVALID
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    r.set_partition(2, 0)
    assert adv(r) == PT_ERR_UNSUPPORTED                         # a two-rank partition
    r.set_partition(1, 0)
    r.set_stats_mode(True)
    assert adv(r) == PT_ERR_UNSUPPORTED
    r.set_stats_mode(False)
    r.set_option(ptamd.PT_OPT_COUNT_TRACED, 1)
    assert adv(r) == PT_ERR_UNSUPPORTED
    r.set_option(ptamd.PT_OPT_COUNT_TRACED, 0)
    assert adv(r) == PT_OK
    g = ptamd.Renderer(devices=[0, 0])                          # a multi-device context, both members on device 0
    assert adv(g) == PT_ERR_UNSUPPORTED
    assert L.pt_temporal_reset(g._c) == PT_ERR_UNSUPPORTED and L.pt_temporal_denoise(g._c, None, None) == PT_ERR_UNSUPPORTED
    assert g.temporal_ptr(0) is None
    # pt_reproject: parameters, misaligned and aliased pointers
    W, H = 16, 16
    bufs = [torch.zeros(W * H * k + 4, dtype=torch.float32, device="cuda") for k in (4, 2, 4, 4, 2, 1, 4, 4, 2, 1, 1)]
    torch.cuda.synchronize()
    keys = [k for k, _ in ptamd.ReprojectImages._fields_]

    def call(r_=r, params=None, n=2, **over):
        im = ptamd.ReprojectImages(*[b.data_ptr() for b in bufs])
        for k, v in over.items():
            setattr(im, k, v)
        p = None if params is None else ctypes.byref(ptamd.TemporalParams(*params))
        return L.pt_reproject(r_._c, cam.ctypes.data, cam.ctypes.data, W, H, n, ctypes.byref(im), p)

    assert call() == PT_OK
    assert call(g) == PT_ERR_UNSUPPORTED
    for bad in [(0, 0.0, 0.5, 0.05), (65537, 0.0, 0.5, 0.05), (64, 1.5, 0.5, 0.05), (64, 0.0, 2.0, 0.05),
                (64, 0.0, 0.5, 0.0), (64, 0.0, 0.5, float("nan"))]:
        assert call(params=bad) == PT_ERR_INVALID, bad
    assert call(n=0) == PT_ERR_INVALID and call(n=65537) == PT_ERR_INVALID
    for k, b in zip(keys, bufs):
        assert call(**{k: b.data_ptr() + 4}) == (PT_OK if k in ("hist_length", "out_length", "out_variance") else PT_ERR_INVALID), k
        assert call(**{k: b.data_ptr() + 2}) == PT_ERR_INVALID, k
    assert call(out_color=bufs[0].data_ptr()) == PT_ERR_INVALID                    # an output is an input
    assert call(out_moments=bufs[4].data_ptr()) == PT_ERR_INVALID
    assert call(out_variance=bufs[9].data_ptr()) == PT_ERR_INVALID                 # two outputs alike
    assert call(hist_guide=None) == PT_ERR_INVALID                                  # three history images
    r.synchronize()


@pytest.mark.parametrize("denoise", [False, True])
def test_pt_render_temporal_flag(tmp_path, denoise):
    W, H, spp, K = 64, 48, 2, 4
    exe = os.path.join(PKG, "pt_render")
    out = str(tmp_path / "f.pfm")
    res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(W), "-h", str(H), "-spp", str(spp),
                          "-temporal", str(K), "-o", out] + (["-denoise-var"] if denoise else []),
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    # the tool's cameras: the default one rotated k times by the float32 step x' = x*c + z*s, z' = z*c - x*s
    c2, s2 = F(0.99939083), F(0.0348995)
    cam = np.array(scenes.DEFAULT_CAMERA, F)
    r = _renderer("box", W, H)
    for k in range(K):
        if k:
            for o in (0, 4):
                x, z = cam[o], cam[o + 2]
                cam[o], cam[o + 2] = x * c2 + z * s2, z * c2 - x * s2
        r.temporal_advance(cam, spp)
    want = r.temporal_denoise() if denoise else r.read_temporal()[0]
    same(read_pfm(out), want[..., :3], f"pt_render -temporal, denoise {denoise}")


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_quality(name):
    """64x64, eight frames of 2 spp at 2 degree steps, against 256 spp of the
    last view rendered at seed base 1000, over the first-hit pixels.  The
    temporal frame's error must be below 0.5 of the raw last frame's (the ideal
    is 1/8; a float64 prototype's worst case over both scenes, also at 1 spp per
    frame, was 0.26), and pt_temporal_denoise's below both the temporal frame's
    and pt_denoise_var's of the raw last frame (prototype: 0.024 / 0.046 of raw
    against 0.098 / 0.117 and 0.16 / 0.29).
    Measured on an MI355X: see DESIGN.md section 9b."""
    W = H = 64
    n, frames = 2, 8
    r = _renderer(name, W, H)
    for k in range(frames):
        r.temporal_advance(_orbit(name, 2 * k), n)
    temporal = r.read_temporal()[0]
    filtered = r.temporal_denoise()
    raw = r.read_accum().reshape(H, W, 4)
    raw_filtered = r.denoise_var()                               # the raw 2-spp frame through pt_denoise_var
    hit = r.read_guide()[..., 3] < 1e30
    q = _renderer(name, W, H, moments=0)
    q.set_camera(_orbit(name, 2 * (frames - 1)))
    q.set_option(ptamd.PT_OPT_SEED_BASE, 1000)
    q.render(0, 256)
    ref = q.read_accum().reshape(H, W, 4)
    e_raw, e_t, e_f, e_rf = (mse(x, ref, hit) for x in (raw, temporal, filtered, raw_filtered))
    print(f"temporal quality {name} 64x64, {np.count_nonzero(hit)} first-hit pixels: mse raw = {e_raw:.4e}, "
          f"temporal = {e_t:.4e} ({e_t / e_raw:.3f} of raw), pt_temporal_denoise = {e_f:.4e} ({e_f / e_raw:.3f}), "
          f"pt_denoise_var of raw = {e_rf:.4e} ({e_rf / e_raw:.3f})")
    for x in (temporal, filtered):
        assert np.all(np.isfinite(x))
    assert e_t < 0.5 * e_raw
    assert e_f < e_t and e_f < e_rf
