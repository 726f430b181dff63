"""Guide-driven upsampling on the GPU: upsample_kernel against the host's run of
the same header code (pt_upsample_host) bit for bit, on seeded and hostile
images handed in as device memory from torch; pt_upsample on rendered frames,
its full-size guide against a second renderer's at that size; the guide cache;
the fused pt_upsample_display byte for byte against pt_display_host of the
host's upsampled image, with and without metering; and the error paths.
133x65 at scale 2 is 266x130: 17 tile columns and 9 rows, ragged both ways."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import display_ref as R
import ptamd
import scenes
import upsample_ref as U
from display_ref import same_bytes, same_float
from support import PKG, dev, read_device, read_pfm, renderer, same, same_nan, scene

pytestmark = pytest.mark.gpu

PT_OK, PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 0, -1, -5
F = np.float32
CAM_324 = scenes.camera((3, 2, 4))
SHAPES = U.SHAPES + [(133, 65, 2)]
CAMERAS = {"box": scenes.DEFAULT_CAMERA, "sphere": CAM_324}
OPERATORS = [R.CLAMP, R.REINHARD, R.ACES]
LW, LH = 32, 24                                   # the render size of the context-level tests


def _image(H, W):
    t = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t


def _device(a):
    t = dev(a)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("w,h,s", SHAPES)
def test_images_match_host(w, h, s):
    rgba, guide, _ = U.seeded(w, h, s)
    W, H = s * w, s * h
    src, g, dst = _device(rgba), _device(guide), _image(H, W)
    r = ptamd.Renderer(0)                          # no scene, no camera, no frame
    for params in (s, (s, 1.0, 0.5)):
        want = ptamd.upsample_host(rgba, w, h, guide, params)
        got = r.upsample_images(src.data_ptr(), w, h, g.data_ptr(), None, params)
        same(got, want, f"library-owned {w}x{h} {params}")
        assert r.upsample_info()["size"] == (W, H) and r.upsampled_ptr()
        assert r.upsample_images(src.data_ptr(), w, h, g.data_ptr(), dst.data_ptr(), params) is None
        r.synchronize()
        same(dst.cpu().numpy(), want, f"caller-owned {w}x{h} {params}")
    assert np.array_equal(src.cpu().numpy().view(np.uint32), rgba.view(np.uint32))       # the inputs are only read
    assert np.array_equal(g.cpu().numpy().view(np.uint32), guide.view(np.uint32))


@pytest.mark.parametrize("kind", ["extremes", "nonfinite"])
def test_hostile_images_match_host(kind):
    r = ptamd.Renderer(0)
    s = U.HOSTILE_SCALE
    n = 0
    for w, h, seed, plane in U.hostile_cases(kind):
        color, guide = U.hostile_images(kind, w, h, seed, plane)
        src, g = _device(color), _device(guide)
        got = r.upsample_images(src.data_ptr(), w, h, g.data_ptr(), None, s)
        same_nan(got, ptamd.upsample_host(color, w, h, guide, s), f"{kind} {w}x{h} seed {seed} plane {plane}")
        n += 1
    assert n >= 20


@pytest.fixture(scope="module", params=sorted(CAMERAS))
def rendered(request):
    """(name, a renderer at LW x LH after two batches, its accumulation image, pt_denoise's image on the
    device and on the host)."""
    name = request.param
    r = renderer(scene(name), CAMERAS[name], size=(LW, LH))
    if name == "sphere":
        assert r.wide_info()[0] > 0, r.wide_info()
    r.render(0, 2)
    accum = r.read_accum().reshape(LH, LW, 4)
    dn = _image(LH, LW)
    r.denoise(None, None, dn.data_ptr())
    r.synchronize()
    return name, r, accum, dn, dn.cpu().numpy()


_GUIDES = {}


def _full_guide(name, s):
    """The guide a second renderer gives at the full size (pinned to the oracle by tests/test_gpu_denoise.py)."""
    if (name, s) not in _GUIDES:
        r = renderer(scene(name), CAMERAS[name], size=(s * LW, s * LH))
        r.render_guide()
        _GUIDES[name, s] = r.read_guide()
    return _GUIDES[name, s]


@pytest.mark.parametrize("s", [2, 4])
def test_context_upsample(rendered, s):
    name, r, accum, dn, filtered = rendered
    W, H = s * LW, s * LH
    got = r.upsample(s)
    info = r.upsample_info()
    assert info["scale"] == s and info["guide_size"] == (W, H) and info["size"] == (W, H)
    guide = read_device(r, r.upsample_guide_ptr(), (H, W, 4))
    hits = int(np.count_nonzero(guide[..., 3] < 1e30))
    assert 0 < hits < W * H
    same(guide, _full_guide(name, s), "the kept guide against a renderer at the full size")
    r.render_guide()
    same(guide[::s, ::s], r.read_guide(), "its stride-s subsample against the context's own guide")
    same(got, ptamd.upsample_host(accum, LW, LH, guide, s), "the accumulation image")
    assert np.array_equal(got[::s, ::s], accum)                                   # the lattice identity
    same(r.read_accum().reshape(LH, LW, 4), accum, "the source is only read")
    # pt_denoise's image as the source, into the caller's image
    dst = _image(H, W)
    assert r.upsample(s, dn.data_ptr(), dst.data_ptr()) is None
    r.synchronize()
    same(dst.cpu().numpy(), ptamd.upsample_host(filtered, LW, LH, guide, s), "pt_denoise's image")
    same(dn.cpu().numpy(), filtered, "pt_denoise's image is only read")
    same(r.read_guide(), guide[::s, ::s], "the context's own guide is not touched")


def _fresh(name, cam, w, h, s):
    r = renderer(scene(name), cam, size=(w, h))
    r.render(0, 2)
    return r.upsample(s)


def test_guide_cache():
    r = renderer(scene("box"), scenes.DEFAULT_CAMERA, size=(LW, LH))
    r.render(0, 2)
    launches = lambda: r.upsample_info()["guide_launches"]
    assert launches() == 0 and not r.upsample_guide_ptr() and r.upsample_info()["scale"] == 0
    first = r.upsample(2)
    assert launches() == 1 and r.upsample_guide_ptr()
    same(first, _fresh("box", scenes.DEFAULT_CAMERA, LW, LH, 2), "a fresh context")
    # nothing changed: no guide launch, the same image -- nor after the same camera and size again
    same(r.upsample(2), first, "an unchanged call")
    r.set_camera(scenes.DEFAULT_CAMERA)
    r.upsample_display(2)
    assert launches() == 1

    def again(name, cam, w, h, s, what, n):
        r.resize_and_clear(w, h)
        r.render(0, 2)
        same(r.upsample(s), _fresh(name, cam, w, h, s), what)
        assert launches() == n, what
        r.upsample(s)
        assert launches() == n, what + ", repeated"

    r.set_camera(CAM_324)
    assert not r.upsample_guide_ptr() and r.upsample_info()["scale"] == 0
    again("box", CAM_324, LW, LH, 2, "a changed camera", 2)
    r.upload_scene(*scene("sphere"))
    assert not r.upsample_guide_ptr()
    again("sphere", CAM_324, LW, LH, 2, "a second scene", 3)
    again("sphere", CAM_324, LW + 8, LH, 2, "a resize", 4)
    again("sphere", CAM_324, LW + 8, LH, 4, "a changed scale", 5)
    again("sphere", CAM_324, LW + 8, LH, 2, "the scale changed back", 6)


@pytest.mark.parametrize("s", [2, 4])
def test_upsample_display(rendered, s):
    name, r, accum, dn, filtered = rendered
    W, H = s * LW, s * LH
    guide = _full_guide(name, s)
    up = ptamd.upsample_host(accum, LW, LH, guide, s)
    up_dn = ptamd.upsample_host(filtered, LW, LH, guide, s)
    dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def expected(image, params, scale):
        """pt_display_host of the upsampled image at exposure * scale, metering off: the fused kernel's product."""
        tonemap, exposure, _, key, white, adapt = params
        return ptamd.display_host(image, W, H, (tonemap, float(F(exposure) * F(scale)), 0, key, white, adapt))[0]

    for tonemap in OPERATORS:
        fixed = (tonemap, 1.5, 0, 0.18, 2.0, 1.0)
        want = ptamd.display_host(up, W, H, fixed)[0]
        same_bytes(r.upsample_display(s, fixed), want, f"library-owned, operator {tonemap}")
        assert r.upsample_info()["display_size"] == (W, H) and r.display_upsampled_ptr()
        assert r.upsample_display(s, fixed, None, dst.data_ptr()) is None
        r.synchronize()
        same_bytes(dst.cpu().numpy().view(np.uint8).reshape(H, W, 4), want, f"caller-owned, operator {tonemap}")
        # metering: of the rendered pixels
        auto = (tonemap, 1.5, 1, 0.18, 2.0, 1.0)
        scale = ptamd.display_host(accum, LW, LH, auto)[1]
        r.display_reset()
        same_bytes(r.upsample_display(s, auto), expected(up, auto, scale), f"metering, operator {tonemap}")
        got_scale, got_n = r.display_exposure()
        same_float(got_scale, scale, "pt_display_exposure's scale: the low image's")
        assert got_n == R.meter(accum, LW, LH)[1] and got_n > 0
    assert want[..., :3].any() and np.all(want[..., 3] == 255)
    # two calls in a row adapt as the host chain does, and pt_display carries on from them
    slow = (R.REINHARD, 1.0, 1, 0.18, 4.0, 0.25)
    r.display_reset()
    s1 = ptamd.display_host(accum, LW, LH, slow, auto_scale=0.0)[1]
    s2 = ptamd.display_host(filtered, LW, LH, slow, auto_scale=s1)[1]
    want3, s3 = ptamd.display_host(accum, LW, LH, slow, auto_scale=s2)
    assert len({s1, s2, s3}) == 3
    same_bytes(r.upsample_display(s, slow), expected(up, slow, s1), "the first call")
    same_float(r.display_exposure()[0], s1, "the first scale")
    same_bytes(r.upsample_display(s, slow, dn.data_ptr()), expected(up_dn, slow, s2), "the second call")
    same_float(r.display_exposure()[0], s2, "the second scale")
    same_bytes(r.display(slow), want3, "pt_display after them")
    same_float(r.display_exposure()[0], s3, "the third scale")
    same(r.read_accum().reshape(LH, LW, 4), accum, "the source is only read")


def test_error_paths():
    L = ptamd.lib()
    w, h, s = 8, 6, 2
    src, g, dst = _device(np.ones((h, w, 4), F)), _device(np.ones((s * h, s * w, 4), F)), _image(s * h, s * w)
    words = torch.zeros(s * s * w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    buf = np.zeros(s * s * w * h * 4, F)
    r = ptamd.Renderer(0)
    up = lambda *a: L.pt_upsample(r._c, *a)
    images = lambda *a: L.pt_upsample_images(r._c, *a)
    # pt_upsample needs a scene, a camera and a frame; pt_upsample_images none of them
    assert up(None, None, None) == PT_ERR_INVALID and L.pt_upsample_display(r._c, None, None, None, None) == PT_ERR_INVALID
    assert images(None, src.data_ptr(), w, h, g.data_ptr(), dst.data_ptr()) == PT_OK
    assert L.pt_read_upsampled(r._c, buf.ctypes.data, buf.size) == PT_ERR_INVALID      # no library-owned image yet
    assert r.upsampled_ptr() is None and r.display_upsampled_ptr() is None and r.upsample_guide_ptr() is None
    r.upload_scene(*scene("box"))
    assert up(None, None, None) == PT_ERR_INVALID                                       # no camera
    r.set_camera(scenes.DEFAULT_CAMERA)
    assert up(None, None, None) == PT_ERR_INVALID                                       # no frame
    r.resize_and_clear(w, h)
    assert up(None, None, None) == PT_OK and L.pt_upsample_display(r._c, None, None, None, None) == PT_OK
    assert L.pt_read_upsampled(r._c, buf.ctypes.data, buf.size - 1) == PT_ERR_INVALID
    assert L.pt_read_upsampled(r._c, None, buf.size) == PT_ERR_INVALID
    assert L.pt_read_display_upsampled(r._c, buf.ctypes.data, s * s * w * h * 4 - 1) == PT_ERR_INVALID
    assert L.pt_read_upsampled(r._c, buf.ctypes.data, buf.size) == PT_OK
    # parameters
    inf, nan = float("inf"), float("nan")
    for bad in [(1, 0.35, 0.25), (9, 0.35, 0.25), (0, 0.35, 0.25), (2, 0.0, 0.25), (2, nan, 0.25), (2, 1e30, 0.25),
                (2, 0.35, -1.0), (2, 0.35, inf), (2, 0.35, 1e-30)]:
        p = ctypes.byref(ptamd.UpsampleParams(*bad))
        assert up(p, None, None) == PT_ERR_INVALID, bad
        assert images(p, src.data_ptr(), w, h, g.data_ptr(), None) == PT_ERR_INVALID, bad
        assert L.pt_upsample_display(r._c, p, None, None, None) == PT_ERR_INVALID, bad
    bad_display = ctypes.byref(ptamd.DisplayParams(3, 1.0, 0, 0.18, 4.0, 1.0))
    assert L.pt_upsample_display(r._c, None, bad_display, None, None) == PT_ERR_INVALID
    # images: null, misaligned, identical, too large
    assert images(None, None, w, h, g.data_ptr(), None) == PT_ERR_INVALID
    assert images(None, src.data_ptr(), w, h, None, None) == PT_ERR_INVALID
    assert images(None, src.data_ptr() + 4, w, h, g.data_ptr(), None) == PT_ERR_INVALID
    assert images(None, src.data_ptr(), w, h, g.data_ptr() + 8, None) == PT_ERR_INVALID
    assert images(None, src.data_ptr(), w, h, g.data_ptr(), dst.data_ptr() + 4) == PT_ERR_INVALID
    assert images(None, src.data_ptr(), w, h, g.data_ptr(), g.data_ptr()) == PT_ERR_INVALID
    assert images(None, dst.data_ptr(), w, h, g.data_ptr(), dst.data_ptr()) == PT_ERR_INVALID
    for bw, bh in [(0, h), (w, 0), (-1, h), (32768, 32768)]:
        assert images(None, src.data_ptr(), bw, bh, g.data_ptr(), None) == PT_ERR_INVALID
    assert up(None, src.data_ptr() + 4, None) == PT_ERR_INVALID
    assert up(None, None, dst.data_ptr() + 4) == PT_ERR_INVALID
    assert up(None, dst.data_ptr(), dst.data_ptr()) == PT_ERR_INVALID
    assert up(None, None, r.accum_ptr()) == PT_ERR_INVALID
    assert L.pt_upsample_display(r._c, None, None, None, words.data_ptr() + 2) == PT_ERR_INVALID
    assert L.pt_upsample_display(r._c, None, None, src.data_ptr() + 4, None) == PT_ERR_INVALID
    assert L.pt_upsample_display(r._c, None, None, None, r.accum_ptr()) == PT_ERR_INVALID
    assert up(None, None, dst.data_ptr()) == PT_OK and L.pt_upsample_display(r._c, None, None, None, words.data_ptr()) == PT_OK
    r.synchronize()
    assert L.pt_upsample(None, None, None, None) == PT_ERR_INVALID and L.pt_upsample_info(r._c, None) == PT_ERR_INVALID


def test_multi_device_context_is_unsupported():
    L = ptamd.lib()
    g = ptamd.Renderer(devices=[0, 0])
    buf = np.zeros(64, F)
    info = (ctypes.c_int * 8)()
    assert L.pt_upsample(g._c, None, None, None) == PT_ERR_UNSUPPORTED
    assert L.pt_upsample_images(g._c, None, None, 1, 1, None, None) == PT_ERR_UNSUPPORTED
    assert L.pt_upsample_display(g._c, None, None, None, None) == PT_ERR_UNSUPPORTED
    assert L.pt_read_upsampled(g._c, buf.ctypes.data, buf.size) == PT_ERR_UNSUPPORTED
    assert L.pt_read_display_upsampled(g._c, buf.ctypes.data, buf.nbytes) == PT_ERR_UNSUPPORTED
    assert L.pt_upsample_info(g._c, info) == PT_ERR_UNSUPPORTED
    assert g.upsampled_ptr() is None and g.upsample_guide_ptr() is None and g.display_upsampled_ptr() is None


def test_pt_render_upsample_flag(tmp_path):
    """The driver renders batch by batch at -w / -h and writes the full-size frame."""
    s, spp = 2, 2
    exe = os.path.join(PKG, "pt_render")
    r = renderer(scene("box"), scenes.DEFAULT_CAMERA, size=(LW, LH))
    r.render(0, spp)

    def run(*flags):
        res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(LW), "-h", str(LH), "-spp", str(spp),
                              "-upsample", str(s)] + [str(f) for f in flags], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]

    def png(rgba8):
        path = tmp_path / "want.png"
        ptamd.write_png8(path, rgba8, s * LW, s * LH)
        return path.read_bytes()

    pfm, shown = tmp_path / "up.pfm", tmp_path / "up.png"
    run("-o", pfm, "-png", shown, "-display", "aces", "-auto-exposure", "0.25")
    same(read_pfm(pfm), r.upsample(s)[..., :3], "pt_render -upsample")
    assert shown.read_bytes() == png(r.upsample_display(s, (R.ACES, 1.0, 1, 0.25, 4.0, 1.0)))
    run("-denoise", "-o", pfm)
    dn = _image(LH, LW)
    r.denoise(None, None, dn.data_ptr())
    same(read_pfm(pfm), r.upsample(s, dn.data_ptr())[..., :3], "pt_render -denoise -upsample")
