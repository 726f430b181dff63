"""GPU: the spatial variance estimate of pixels with a short history.
spatial_var_kernel against the host's run of the same header code
(pt_spatial_variance_host) and the independent numpy restatement
(tests/spatial_var_ref.py), bit for bit; pt_temporal_denoise_spatial against
the host filter fed with the host's estimate; that it is pt_temporal_denoise
when no pixel is short; the error paths; the pt_render flag; and what the
estimate buys in error at one sample per frame."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import ptamd
import scenes
import spatial_var_ref as S
from support import PKG, bits, dev, mse, read_device, read_pfm, renderer, same, scene

pytestmark = pytest.mark.gpu

F = np.float32
PT_OK, PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 0, -1, -5
START = {"box": (0.0, 0.0, 5.0), "sphere": (3.0, 2.0, 4.0)}
SIZE = {"box": (64, 48), "sphere": (67, 45)}                  # the frame sizes of test_gpu_temporal.py
SEED_BASE, REF_SEED_BASE, REF_SPP = 1000, 1000 + (1 << 20), 256


def _orbit(name, degrees):
    x, y, z = START[name]
    a = np.deg2rad(degrees)
    return scenes.camera((x * np.cos(a) + z * np.sin(a), y, z * np.cos(a) - x * np.sin(a)))


def _renderer(name, moments=1, seed_base=SEED_BASE, size=None):
    return renderer(scene(name), _orbit(name, 0), size=size or SIZE[name],
                    options=[(ptamd.PT_OPT_MOMENTS, moments), (ptamd.PT_OPT_SEED_BASE, seed_base)])


def _inputs():
    for W, H in [(16, 16), (37, 23), (64, 48)]:
        yield W, H, "", S.make_inputs(W, H, 100 * W + H)
    for only in ("none", "corner"):
        yield 16, 16, only, S.make_inputs(16, 16, 7, only)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_device_matches_host_and_restatement(radius):
    r = ptamd.Renderer(0)
    for W, H, tag, d in _inputs():
        keys = ("moments", "length", "variance", "guide")
        ins = [dev(d[k]) for k in keys]
        for params in (None if radius == 1 else (2, radius, 1.0, 1.0), (4, radius, 0.5, 0.25), (65536, radius, 0.25, 1.0),
                       (1, radius, 1.0, 1.0)):
            out = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda")        # the sentinel
            torch.cuda.synchronize()
            r.spatial_variance(*[t.data_ptr() for t in ins], W, H, out.data_ptr(), params)
            r.synchronize()
            got = out.cpu().numpy()
            host = ptamd.spatial_variance_host(*[d[k] for k in keys], W, H, params)
            ref = S.spatial_variance(*[d[k] for k in keys], W, H, S.DEFAULTS if params is None else params)
            same(got, host, f"{W}x{H} {tag} {params}: device against host")
            same(got, ref, f"{W}x{H} {tag} {params}: device against the restatement")
            if params is not None and params[0] == 1:
                same(got, d["variance"], "below 1: the variance itself")
        for t, k in zip(ins, keys):
            same(t.cpu().numpy(), d[k], f"input {k} after the calls")


@functools.lru_cache(maxsize=None)
def _reference(name, degrees):
    W, H = SIZE[name]
    q = _renderer(name, moments=0, seed_base=REF_SEED_BASE)
    q.set_camera(_orbit(name, degrees))
    q.render(0, REF_SPP)
    ref = q.read_accum().reshape(H, W, 4).copy()
    q.close()
    return ref


def _capture(r, name, degrees, n):
    """The temporal result r holds, both filters' images of it from the device
    and what the host makes of the same planes."""
    W, H = SIZE[name]
    c, m, l = r.read_temporal()
    v = read_device(r, r.temporal_ptr(3), (H, W))
    guide = r.read_guide()
    raw = r.read_accum().reshape(H, W, 4)
    plain = r.temporal_denoise()
    spatial = {}
    for staged in (0, 1):
        r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
        spatial[staged] = r.temporal_denoise_spatial()
    dst = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert r.temporal_denoise_spatial(None, None, dst.data_ptr()) is None
    r.synchronize()
    after = r.read_temporal() + (read_device(r, r.temporal_ptr(3), (H, W)),)
    return {"c": c, "m": m, "l": l, "v": v, "guide": guide, "raw": raw, "plain": plain, "spatial": spatial,
            "spatial_dst": dst.cpu().numpy(), "after": after, "degrees": degrees, "n": n}


@functools.lru_cache(maxsize=None)
def _captures(name, n=1):
    """first: the first frame; jump: a second frame 60 degrees on; orbit: the
    eighth frame at 2 degree steps.  n samples per frame, seed base 1000."""
    r = _renderer(name)
    r.temporal_advance(_orbit(name, 0), n)
    out = {"first": _capture(r, name, 0, n)}
    r.temporal_advance(_orbit(name, 60), n)
    out["jump"] = _capture(r, name, 60, n)
    r.temporal_reset()
    for k in range(8):
        r.temporal_advance(_orbit(name, 2 * k), n)
    out["orbit"] = _capture(r, name, 14, n)
    r.close()
    return out


@pytest.mark.parametrize("case", ["first", "jump"])
@pytest.mark.parametrize("name", ["box", "sphere"])
def test_temporal_denoise_spatial_equals_the_host(name, case):
    W, H = SIZE[name]
    s = _captures(name)[case]
    assert np.any(s["l"] == 1)
    assert np.all(s["l"] == 1) == (case == "first")
    plane = ptamd.spatial_variance_host(s["m"], s["l"], s["v"], s["guide"], W, H)
    same(plane, S.spatial_variance(s["m"], s["l"], s["v"], s["guide"], W, H), f"{name} {case}: host estimate")
    assert np.any(plane[s["l"] == 1] > 0) and np.all(s["v"][s["l"] == 1] == 0)
    want = ptamd.denoise_var_plane_host(s["c"], plane, s["guide"], W, H)
    for staged in (0, 1):
        same(s["spatial"][staged], want, f"{name} {case}: staged {staged}")
    same(s["spatial_dst"], want, f"{name} {case}: caller-owned destination")
    for a, b, what in zip(s["after"], (s["c"], s["m"], s["l"], s["v"]), ("colour", "moments", "length", "variance")):
        same(a, b, f"{name} {case}: the temporal {what} after the calls")
    assert np.any(bits(s["spatial"][1]) != bits(s["plain"]))             # the estimate changes the image


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_two_samples_and_below_two_is_temporal_denoise(name):
    """At 2 spp no length is below 2: no pixel is short."""
    r = _renderer(name)
    for degrees in (0, 2, 62):
        r.temporal_advance(_orbit(name, degrees), 2)
        assert r.read_temporal()[2].min() == 2
        for filt in (None, (2, 0.75, 0.5, 0.25)):
            same(r.temporal_denoise_spatial(filt, (2, 3, 0.5, 0.5)), r.temporal_denoise(filt), f"{name} {degrees} {filt}")
    # and with a threshold above 2 it is not
    assert np.any(bits(r.temporal_denoise_spatial(None, (3, 1, 1.0, 1.0))) != bits(r.temporal_denoise()))


def test_error_paths():
    L = ptamd.lib()
    W, H = SIZE["box"]
    sp = lambda *p: ctypes.byref(ptamd.SpatialVarParams(*p))
    r = _renderer("box")
    assert L.pt_temporal_denoise_spatial(r._c, None, None, None) == PT_ERR_INVALID                  # no temporal result
    assert L.pt_temporal_denoise_spatial(None, None, None, None) == PT_ERR_INVALID
    r.temporal_advance(_orbit("box", 0), 1)
    assert L.pt_temporal_denoise_spatial(r._c, None, None, None) == PT_OK
    dst = torch.zeros(W * H * 4 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert L.pt_temporal_denoise_spatial(r._c, None, None, dst.data_ptr()) == PT_OK
    assert L.pt_temporal_denoise_spatial(r._c, None, None, dst.data_ptr() + 4) == PT_ERR_INVALID    # misaligned
    assert L.pt_temporal_denoise_spatial(r._c, None, None, r.temporal_ptr(0)) == PT_ERR_INVALID     # onto its source
    assert L.pt_temporal_denoise_spatial(r._c, ctypes.byref(ptamd.DenoiseVarParams(7, 1.5, 1.0, 1.0)), None, None) == PT_ERR_INVALID
    for bad in [(65537, 1, 1.0, 1.0), (2, 0, 1.0, 1.0), (2, 4, 1.0, 1.0), (2, 1, 0.0, 1.0), (2, 1, 1.0, float("nan")),
                (2, 1, float("inf"), 1.0), (2, 1, 1.0, 1e-30)]:
        assert L.pt_temporal_denoise_spatial(r._c, None, sp(*bad), None) == PT_ERR_INVALID, bad
    for good in [(0, 1, 1.0, 1.0), (65536, 3, 0.25, 0.25)]:
        assert L.pt_temporal_denoise_spatial(r._c, None, sp(*good), None) == PT_OK, good
    r.temporal_reset()
    assert L.pt_temporal_denoise_spatial(r._c, None, None, None) == PT_ERR_INVALID                  # forgotten
    # pt_spatial_variance: null, misaligned and aliased pointers, parameters
    bufs = [torch.zeros(W * H * k + 4, dtype=torch.float32, device="cuda") for k in (2, 1, 1, 4, 1)]
    torch.cuda.synchronize()

    def call(r_=r, params=None, w=W, h=H, **over):
        a = dict(zip(("m", "l", "v", "g", "out"), (b.data_ptr() for b in bufs)))
        a.update(over)
        return L.pt_spatial_variance(r_._c, a["m"], a["l"], a["v"], a["g"], w, h, None if params is None else sp(*params),
                                     a["out"])

    assert call() == PT_OK
    for k, b in zip(("m", "l", "v", "g", "out"), bufs):
        assert call(**{k: None}) == PT_ERR_INVALID, k
        assert call(**{k: b.data_ptr() + 2}) == PT_ERR_INVALID, k
        assert call(**{k: b.data_ptr() + 4}) == (PT_OK if k in ("l", "v", "out") else PT_ERR_INVALID), k
    assert call(m=bufs[0].data_ptr() + 8) == PT_OK
    for k, b in zip(("m", "l", "v", "g"), bufs):
        assert call(out=b.data_ptr()) == PT_ERR_INVALID, k                                           # out is an input
    assert call(w=0) == PT_ERR_INVALID and call(h=-1) == PT_ERR_INVALID
    for bad in [(65537, 1, 1.0, 1.0), (2, 0, 1.0, 1.0), (2, 4, 1.0, 1.0), (2, 1, -1.0, 1.0), (2, 1, 1.0, 0.0)]:
        assert call(params=bad) == PT_ERR_INVALID, bad
    r.synchronize()
    g = ptamd.Renderer(devices=[0, 0])                          # a multi-device context, both members on device 0
    assert call(g) == PT_ERR_UNSUPPORTED
    assert L.pt_temporal_denoise_spatial(g._c, None, None, None) == PT_ERR_UNSUPPORTED


def test_pt_render_temporal_spatial_flag(tmp_path):
    W, H, spp, K = 64, 48, 1, 3
    exe = os.path.join(PKG, "pt_render")
    out = str(tmp_path / "f.pfm")
    res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(W), "-h", str(H), "-spp", str(spp),
                          "-temporal", str(K), "-temporal-spatial", "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    # the tool's cameras: the default one rotated k times by the float32 step x' = x*c + z*s, z' = z*c - x*s
    c2, s2 = F(0.99939083), F(0.0348995)
    cam = np.array(scenes.DEFAULT_CAMERA, F)
    r = _renderer("box", seed_base=0, size=(W, H))
    for k in range(K):
        if k:
            for o in (0, 4):
                x, z = cam[o], cam[o + 2]
                cam[o], cam[o + 2] = x * c2 + z * s2, z * c2 - x * s2
        r.temporal_advance(cam, spp)
    want = r.temporal_denoise_spatial()
    same(read_pfm(out), want[..., :3], "pt_render -temporal 3 -spp 1 -temporal-spatial")
    assert np.any(bits(want) != bits(r.temporal_denoise()))
    res = subprocess.run([exe, scenes.BOX_OBJ, "-temporal-spatial"], capture_output=True, text=True)   # needs -temporal K
    assert res.returncode == 2


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_quality(name):
    """One sample per frame at seed base 1000, mean squared rgb error against
    256 spp of the same view (another seed base) over first-hit pixels.  On the
    first frame (every pixel short), and on the pixels without history after a
    60 degree jump, pt_temporal_denoise_spatial's error is below both the raw
    frame's and pt_temporal_denoise's; on the eighth frame of a 2 degree orbit
    (few short pixels) it is not above pt_temporal_denoise's.  A float64
    prototype on CPU frames of the box gave raw / pt_temporal_denoise / spatial
    4.008 / 4.008 / 0.812 (first frame, all pixels), 3.094 / 2.759 / 0.742
    (jump, all first-hit pixels) and 0.221 / 0.100 / 0.075 (orbit).
    Measured on an MI355X: see DESIGN.md section 9c."""
    caps = _captures(name)
    err = {}
    for case, s in caps.items():
        ref = _reference(name, s["degrees"])
        hit = s["guide"][..., 3] < 1e30
        mask = hit & (s["l"] == 1) if case == "jump" else hit
        assert np.count_nonzero(mask) > 50
        for img in (s["plain"], s["spatial"][1]):
            assert np.all(np.isfinite(img))
        e = tuple(mse(x, ref, mask) for x in (s["raw"], s["plain"], s["spatial"][1]))
        err[case] = e
        print(f"spatial variance quality {name} {case}: {np.count_nonzero(mask)} pixels "
              f"({np.count_nonzero(hit & (s['l'] == 1))} of {np.count_nonzero(hit)} first-hit pixels short), mse raw = "
              f"{e[0]:.4e}, pt_temporal_denoise = {e[1]:.4e} ({e[1] / e[0]:.3f} of raw), pt_temporal_denoise_spatial = "
              f"{e[2]:.4e} ({e[2] / e[0]:.3f})")
    for case in ("first", "jump"):
        raw, plain, spatial = err[case]
        assert spatial < raw and spatial < plain, (case, err[case])
    assert err["orbit"][2] <= err["orbit"][1], err["orbit"]
