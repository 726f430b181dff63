"""The display transform on the GPU: pt_display against pt_display_host byte for
byte on the hostile images of tests/display_ref.py (handed in as device memory
from torch) and on rendered frames, the metering state across calls, the 8-bit
readback, and the error paths.  265x259 is 17x17 tiles with ragged edges: the
smallest frame at which a lane of the metering's second stage adds more than one
tile partial; 37x23 has 851 pixels, no multiple of a wave or of four."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import display_ref as R
import ptamd
import scenes
from support import PKG, renderer, scene
from display_ref import same_bytes, same_float

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_UNSUPPORTED = -1, -5
F = np.float32
SIZES = [(16, 16), (37, 23), (64, 48), (265, 259)]
OPERATORS = [R.CLAMP, R.REINHARD, R.ACES]


def _frame(W, H):
    """A context with a W x H frame: the transform needs no scene."""
    r = ptamd.Renderer(0)
    r.resize_and_clear(W, H)
    return r


def _device(img):
    t = torch.from_numpy(np.ascontiguousarray(img, F)).cuda()
    torch.cuda.synchronize()
    return t


def _words(t, W, H):
    """A caller-owned destination (int32 words) as (H, W, 4) bytes."""
    return t.cpu().numpy().view(np.uint8).reshape(H, W, 4)


@pytest.mark.parametrize("kind", ["specials", "thresholds", "dark"])
@pytest.mark.parametrize("W,H", SIZES)
def test_device_matches_host(W, H, kind):
    img = R.image(kind, W, H)
    src = _device(img)
    dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r = _frame(W, H)
    n_metered = R.meter(img, W, H)[1]
    for tonemap in OPERATORS:
        for auto in (0, 1):
            params = (tonemap, 1.5, auto, 0.18, 2.0, 1.0)
            want, scale = ptamd.display_host(img, W, H, params)
            r.display_reset()
            same_bytes(r.display(params, src.data_ptr()), want, f"library-owned, operator {tonemap}, metering {auto}")
            if auto:
                got_scale, got_n = r.display_exposure()
                same_float(got_scale, scale, "pt_display_exposure's scale")
                assert got_n == n_metered
            r.display_reset()
            assert r.display(params, src.data_ptr(), dst.data_ptr()) is None
            r.synchronize()
            same_bytes(_words(dst, W, H), want, f"caller-owned, operator {tonemap}, metering {auto}")
    assert np.array_equal(src.cpu().numpy().view(np.uint32), img.view(np.uint32))   # the source is only read
    # the accumulation image as the source: zeros after the clear, nothing metered, no previous scale
    r.display_reset()
    assert not r.display((R.ACES, 1.0, 1, 0.18, 4.0, 1.0))[..., :3].any()
    assert r.display_exposure() == (1.0, 0)


@pytest.mark.parametrize("W,H", [(37, 23), (265, 259)])
def test_adaptation_across_calls(W, H):
    params = (R.REINHARD, 1.0, 1, 0.18, 4.0, 0.25)
    r = _frame(W, H)
    with np.errstate(over="ignore"):
        imgs = [R.image(kind, W, H, seed=k) * F(4.0 ** k) for k, kind in enumerate(["specials", "thresholds", "specials"])]
    srcs = [_device(i) for i in imgs]

    def chain(prev):
        out = []
        for img in imgs:
            want, prev = ptamd.display_host(img, W, H, params, auto_scale=prev)
            out.append((want, prev))
        return out

    for k, (want, scale) in enumerate(chain(0.0)):
        same_bytes(r.display(params, srcs[k].data_ptr()), want, f"call {k}")
        same_float(r.display_exposure()[0], scale, f"the scale of call {k}")
    # a call without metering neither reads nor moves the state
    fixed = (R.REINHARD, 1.0, 0, 0.18, 4.0, 0.25)
    same_bytes(r.display(fixed, srcs[0].data_ptr()), ptamd.display_host(imgs[0], W, H, fixed)[0], "no metering")
    same_float(r.display_exposure()[0], chain(0.0)[2][1], "the state after a call without metering")
    # pt_display_reset forgets: the next call is a first one again
    r.display_reset()
    assert r.display_exposure() == (1.0, 0)
    first = chain(0.0)[0]
    same_bytes(r.display(params, srcs[0].data_ptr()), first[0], "after the reset")
    same_float(r.display_exposure()[0], first[1], "the scale after the reset")
    # so does a resize, there and back
    r.resize_and_clear(W + 1, H)
    assert r.display_exposure() == (1.0, 0) and r.display_ptr() is None
    r.resize_and_clear(W, H)
    second_as_first = ptamd.display_host(imgs[1], W, H, params, auto_scale=0.0)
    same_bytes(r.display(params, srcs[1].data_ptr()), second_as_first[0], "after the resize")
    same_float(r.display_exposure()[0], second_as_first[1], "the scale after the resize")


@pytest.fixture(scope="module")
def rendered():
    W, H = 64, 48
    r = renderer(scene("box"), scenes.DEFAULT_CAMERA, size=(W, H))
    r.render(0, 4)
    return r, r.read_accum().reshape(H, W, 4), W, H


def test_rendered_frame_and_its_filtered_image(rendered, tmp_path):
    r, accum, W, H = rendered
    for params in [None, (R.REINHARD, 0.5, 1, 0.18, 4.0, 1.0), (R.ACES, 2.0, 0, 0.18, 4.0, 1.0)]:
        r.display_reset()
        same_bytes(r.display(params), ptamd.display_host(accum, W, H, params)[0], f"the accumulation image, {params}")
    filtered = r.denoise()
    dn = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.denoise(None, None, dn.data_ptr())
    for params in [None, (R.REINHARD, 0.5, 1, 0.18, 4.0, 1.0)]:
        r.display_reset()
        same_bytes(r.display(params, dn.data_ptr()), ptamd.display_host(filtered, W, H, params)[0], f"pt_denoise's image, {params}")
    # the default parameters: the bytes pt_write_image encodes
    got = r.display()
    assert np.array_equal(got[..., :3], R.srgb8(accum[..., :3])) and np.all(got[..., 3] == 255)
    assert got[..., :3].any()
    a, b = tmp_path / "bytes.png", tmp_path / "floats.png"
    ptamd.write_png8(a, got, W, H)
    ptamd.write_image(b, accum, W, H, "png")
    assert a.read_bytes() == b.read_bytes()
    assert np.array_equal(r.read_accum().reshape(H, W, 4).view(np.uint32), accum.view(np.uint32))
    assert r.display_ptr() is not None


def test_display_readback(rendered):
    r, accum, W, H = rendered
    params = (R.ACES, 1.0, 0, 0.18, 4.0, 1.0)
    want = r.display(params)
    t1 = r.display_readback_begin(params)
    same_bytes(r.display_readback_end(t1), want, "the readback against pt_read_display")
    L = ptamd.lib()
    buf = np.zeros(W * H * 4, np.uint8)
    assert L.pt_display_readback_end(r._c, t1, buf.ctypes.data, buf.size) == PT_ERR_INVALID   # collected once
    # three begins: the third recycles the oldest slot, whose ticket is then unknown
    img = R.image("specials", W, H)
    src = _device(img)
    ta = r.display_readback_begin(params)
    tb = r.display_readback_begin(None, src.data_ptr())
    tc = r.display_readback_begin(params)
    assert len({t1, ta, tb, tc}) == 4
    assert L.pt_display_readback_end(r._c, ta, buf.ctypes.data, buf.size) == PT_ERR_INVALID
    same_bytes(r.display_readback_end(tb), ptamd.display_host(img, W, H)[0], "a caller's source")
    same_bytes(r.display_readback_end(tc), want, "the third")
    assert L.pt_display_readback_end(r._c, tc, buf.ctypes.data, buf.size) == PT_ERR_INVALID
    assert L.pt_display_readback_end(r._c, 0, buf.ctypes.data, buf.size) == PT_ERR_INVALID
    t = r.display_readback_begin(params)
    assert L.pt_display_readback_end(r._c, t, buf.ctypes.data, buf.size - 1) == PT_ERR_INVALID   # too small; still pending
    same_bytes(r.display_readback_end(t), want, "after the refused collection")
    # the float readback's tickets are its own
    tf = r.readback_begin()
    assert np.array_equal(r.readback_end(tf).view(np.uint32), accum.reshape(-1).view(np.uint32))


def test_error_paths():
    L = ptamd.lib()
    W, H = 16, 16
    buf = np.zeros(W * H * 4, np.uint8)
    t = ctypes.c_int(0)
    r = ptamd.Renderer(0)   # no frame yet
    assert L.pt_display(r._c, None, None, None) == PT_ERR_INVALID
    assert L.pt_display_readback_begin(r._c, None, None, ctypes.byref(t)) == PT_ERR_INVALID
    assert L.pt_read_display(r._c, buf.ctypes.data, buf.size) == PT_ERR_INVALID
    assert r.display_ptr() is None and r.display_exposure() == (1.0, 0)
    r.resize_and_clear(W, H)
    assert L.pt_read_display(r._c, buf.ctypes.data, buf.size) == PT_ERR_INVALID   # nothing displayed yet
    src = _device(R.image("specials", W, H))
    dst = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bad = ptamd.DisplayParams(3, 1.0, 0, 0.18, 4.0, 1.0)
    assert L.pt_display(r._c, ctypes.byref(bad), None, None) == PT_ERR_INVALID
    assert L.pt_display_readback_begin(r._c, ctypes.byref(bad), None, ctypes.byref(t)) == PT_ERR_INVALID
    assert L.pt_display(r._c, None, src.data_ptr() + 4, None) == PT_ERR_INVALID              # misaligned
    assert L.pt_display(r._c, None, None, dst.data_ptr() + 2) == PT_ERR_INVALID
    assert L.pt_display(r._c, None, src.data_ptr(), src.data_ptr()) == PT_ERR_INVALID        # in place
    assert L.pt_display(r._c, None, None, r.accum_ptr()) == PT_ERR_INVALID
    assert L.pt_display(None, None, None, None) == PT_ERR_INVALID
    assert L.pt_display_readback_begin(r._c, None, None, None) == PT_ERR_INVALID
    r.display()
    assert L.pt_read_display(r._c, buf.ctypes.data, buf.size - 1) == PT_ERR_INVALID
    assert L.pt_read_display(r._c, None, buf.size) == PT_ERR_INVALID
    assert L.pt_display_exposure(None, None, None) == PT_ERR_INVALID and L.pt_display_reset(None) == PT_ERR_INVALID


def test_multi_device_context_is_unsupported():
    L = ptamd.lib()
    g = ptamd.Renderer(devices=[0, 0])
    buf = np.zeros(64 * 48 * 4, np.uint8)
    t, s, n = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_uint32(0)
    assert L.pt_display(g._c, None, None, None) == PT_ERR_UNSUPPORTED
    assert L.pt_read_display(g._c, buf.ctypes.data, buf.size) == PT_ERR_UNSUPPORTED
    assert L.pt_display_exposure(g._c, ctypes.byref(s), ctypes.byref(n)) == PT_ERR_UNSUPPORTED
    assert L.pt_display_reset(g._c) == PT_ERR_UNSUPPORTED
    assert L.pt_display_readback_begin(g._c, None, None, ctypes.byref(t)) == PT_ERR_UNSUPPORTED
    assert L.pt_display_readback_end(g._c, 1, buf.ctypes.data, buf.size) == PT_ERR_UNSUPPORTED
    assert g.display_ptr() is None


def test_pt_render_display_flags(rendered, tmp_path):
    """The driver renders batch by batch (4 dispatches): the frame `rendered` holds."""
    r, accum, W, H = rendered
    exe = os.path.join(PKG, "pt_render")

    def run(name, *flags):
        path = tmp_path / name
        res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(W), "-h", str(H), "-spp", "4",
                              "-png", str(path)] + list(flags), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        return path.read_bytes()

    def png(rgba8):
        path = tmp_path / "want.png"
        ptamd.write_png8(path, rgba8, W, H)
        return path.read_bytes()

    plain = tmp_path / "plain.png"
    ptamd.write_image(plain, accum, W, H, "png")
    assert run("a.png") == plain.read_bytes()                        # no flag: pt_write_image, as ever
    assert run("b.png", "-display", "clamp") == plain.read_bytes()   # the default transform: the same bytes
    want = ptamd.display_host(accum, W, H, (R.ACES, 0.5, 1, 0.25, 4.0, 1.0))[0]
    assert run("c.png", "-display", "aces", "-exposure", "0.5", "-auto-exposure", "0.25") == png(want)
    want = ptamd.display_host(r.denoise(), W, H, (R.REINHARD, 1.0, 0, 0.18, 4.0, 1.0))[0]
    assert run("d.png", "-denoise", "-display", "reinhard") == png(want)
