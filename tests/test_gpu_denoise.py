"""The guide image and the a-trous denoiser on the GPU: guide_kernel against
the oracle's traceRay on every walk the kernel has, atrous_kernel against the
host's run of the same header code (pt_denoise_host) and against the
independent numpy restatement (tests/denoise_ref.py) -- all bit for bit --
and the behaviour around them: staleness of the guide, caller-owned images,
multi-device contexts, the pt_render flags, and that the filter lowers the
error of a low-sample frame."""
import os
import subprocess

import numpy as np
import pytest
import torch

import denoise_ref as R
import oracle_lib as O
import ptamd
import scenes
from support import PKG, bits, built, mse, read_pfm, renderer, same, scene

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_UNSUPPORTED = -1, -5
MISS = np.array([0.0, 0.0, 0.0, 1e30], np.float32)
CAM_324 = scenes.camera((3, 2, 4))


@pytest.fixture(scope="module")
def box():
    return scene("box")


def _sphere(subdiv):
    return built(*scenes.displaced_sphere(subdiv=subdiv))


@pytest.fixture(scope="module")
def sphere3():
    return _sphere(3)


def _renderer(mesh, cam, W, H):
    return renderer(mesh, cam, size=(W, H))


def _oracle_guide(mesh, cam, W, H):
    """The guide the header defines, from oracle_lib.trace of pt_guide_ray."""
    v, i, n = mesh
    out = np.zeros((H, W, 4), np.float32)
    for y in range(H):
        for x in range(W):
            o, d = ptamd.guide_ray(cam, W, H, x, y)
            hit, t, _, nrm, _ = O.trace(v, i, n.reshape(-1), o, d)
            out[y, x] = np.concatenate([nrm, [np.float32(t)]]) if hit else MISS
    return out


@pytest.fixture(scope="module")
def box_guide(box):
    return _oracle_guide(box, scenes.DEFAULT_CAMERA, 64, 48)


@pytest.fixture(scope="module")
def sphere_guide(sphere3):
    return _oracle_guide(sphere3, CAM_324, 67, 45)


def test_guide_box_matches_oracle(box, box_guide):
    W, H = 64, 48
    r = _renderer(box, scenes.DEFAULT_CAMERA, W, H)
    r.render_guide()
    got = r.read_guide()
    # the x = W/2 column has a zero direction component: the wide walk hands it to the exact walk
    assert ptamd.guide_ray(scenes.DEFAULT_CAMERA, W, H, W // 2, 7)[1][0] == 0.0
    hits = int(np.count_nonzero(got[..., 3] < 1e30))
    assert 0 < hits < W * H and np.any(got[:, W // 2, 3] < 1e30)
    same(got, box_guide, "box guide")


def test_guide_sphere_matches_oracle(sphere3, sphere_guide):
    W, H = 67, 45
    r = _renderer(sphere3, CAM_324, W, H)
    r.render_guide()
    got = r.read_guide()
    hits = int(np.count_nonzero(got[..., 3] < 1e30))
    assert 0 < hits < W * H
    same(got, sphere_guide, "sphere guide")


def test_guide_walk_parity_wide_tree(sphere3, sphere_guide):
    W, H = 67, 45
    r = _renderer(sphere3, CAM_324, W, H)
    assert r.wide_info()[0] > 0, r.wide_info()
    for key, value in [(ptamd.PT_OPT_WIDE, 1), (ptamd.PT_OPT_WIDE_NODE, 128), (ptamd.PT_OPT_WIDE, 0)]:
        r.set_option(key, value)
        r.render_guide()
        same(r.read_guide(), sphere_guide, f"option {key} = {value}")


def test_guide_walk_parity_box(box, box_guide):
    W, H = 64, 48
    r = _renderer(box, scenes.DEFAULT_CAMERA, W, H)
    for opts in [{ptamd.PT_OPT_SCENE_IN_LDS: 0},                        # as the default, scene not in LDS
                 {ptamd.PT_OPT_WIDE: 0, ptamd.PT_OPT_SCENE_IN_LDS: 1},   # the exact walk from LDS
                 {ptamd.PT_OPT_WIDE: 0, ptamd.PT_OPT_SCENE_IN_LDS: 0}]:  # ... from device memory
        for key, value in opts.items():
            r.set_option(key, value)
        r.render_guide()
        same(r.read_guide(), box_guide, f"options {opts}")


@pytest.mark.parametrize("W,H", [(67, 45), (20, 12)])
def test_device_filter_matches_host_and_restatement(box, W, H):
    r = _renderer(box, scenes.DEFAULT_CAMERA, W, H)
    r.render(0, 2)
    accum = r.read_accum().reshape(H, W, 4)
    r.render_guide()
    guide = r.read_guide()
    for iterations in (1, 5, 6):
        params = (iterations, 0.6, 0.35, 0.25)
        ref = R.atrous(accum, guide, W, H, params)
        same(ptamd.denoise_host(accum, guide, W, H, params), ref, f"host, {iterations} passes")
        for staged in (0, 1):
            r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            same(r.denoise(params), ref, f"device, {iterations} passes, staged {staged}")
    same(r.read_accum().reshape(H, W, 4), accum, "the accumulation image after the filter")


def test_device_filter_caller_images(box):
    W, H = 67, 45
    r = _renderer(box, scenes.DEFAULT_CAMERA, W, H)
    r.render(0, 2)
    accum = r.read_accum().reshape(H, W, 4)
    rgba, _ = R.make_images(W, H, seed=5)          # a source that is not the accumulation image
    src = torch.from_numpy(rgba).cuda()
    dst = torch.zeros_like(src)
    torch.cuda.synchronize()
    params = (5, 0.6, 0.35, 0.25)
    assert r.denoise(params, src.data_ptr(), dst.data_ptr()) is None
    r.synchronize()
    guide = r.read_guide()                         # pt_denoise rendered it
    same(dst.cpu().numpy(), R.atrous(rgba, guide, W, H, params), "caller-owned destination")
    same(src.cpu().numpy(), rgba, "caller-owned source")
    same(r.read_accum().reshape(H, W, 4), accum, "the accumulation image")
    L = ptamd.lib()
    assert L.pt_denoise(r._c, None, src.data_ptr(), src.data_ptr()) == PT_ERR_INVALID      # in place
    assert L.pt_denoise(r._c, None, src.data_ptr() + 4, dst.data_ptr()) == PT_ERR_INVALID  # misaligned
    assert L.pt_denoise(r._c, None, None, r.accum_ptr()) == PT_ERR_INVALID                 # accum onto itself


def test_guide_staleness(box, sphere3):
    W, H = 67, 45
    r = _renderer(box, scenes.DEFAULT_CAMERA, W, H)
    r.render(0, 2)
    params = (5, 0.6, 0.35, 0.25)
    first = r.denoise(params)
    old_guide = r.read_guide()
    assert r.guide_ptr()
    r.set_camera(scenes.DEFAULT_CAMERA)            # the same camera keeps the guide
    assert r.guide_ptr()
    r.set_camera(CAM_324)
    assert not r.guide_ptr()
    r.render(0, 2)
    second = r.denoise(params)
    fresh = _renderer(box, CAM_324, W, H)          # the new camera's guide from a context of its own
    fresh.render_guide()
    new_guide = fresh.read_guide()
    assert not np.array_equal(bits(new_guide), bits(old_guide))
    same(second, R.atrous(r.read_accum(), new_guide, W, H, params), "after the camera moved")
    assert not np.array_equal(bits(first), bits(second))
    # the other inputs the guide depends on
    assert r.guide_ptr()
    assert r.progressive_camera(scenes.DEFAULT_CAMERA) and not r.guide_ptr()
    r.render_guide()
    r.resize_and_clear(W, H)                       # same size: still the guide
    assert r.guide_ptr()
    r.resize_and_clear(20, 12)
    assert not r.guide_ptr()
    r.render_guide()
    r.upload_scene(*sphere3)
    assert not r.guide_ptr()
    assert ptamd.lib().pt_read_guide(r._c, np.zeros(20 * 12 * 4, np.float32).ctypes.data, 20 * 12 * 4) == PT_ERR_INVALID


def test_calls_without_inputs_are_invalid(box):
    L = ptamd.lib()
    r = ptamd.Renderer(0)
    buf = np.zeros(64, np.float32)
    assert L.pt_render_guide(r._c) == PT_ERR_INVALID           # no scene
    assert L.pt_denoise(r._c, None, None, None) == PT_ERR_INVALID
    r.upload_scene(*box)
    r.set_camera(scenes.DEFAULT_CAMERA)
    assert L.pt_render_guide(r._c) == PT_ERR_INVALID           # no image
    assert L.pt_denoise(r._c, None, None, None) == PT_ERR_INVALID
    r.resize_and_clear(4, 4)
    assert L.pt_read_denoised(r._c, buf.ctypes.data, buf.size) == PT_ERR_INVALID   # nothing denoised yet
    bad = ptamd.DenoiseParams(0, 0.6, 0.35, 0.25)
    assert L.pt_denoise(r._c, bad, None, None) == PT_ERR_INVALID
    assert r.denoise().shape == (4, 4, 4)


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_it_denoises(box, name):
    """8 spp filtered with the default parameters is closer to 256 spp than
    8 spp is.  The printed errors are the ones include/pathtracer.h quotes."""
    W = H = 256
    mesh, cam = (box, scenes.DEFAULT_CAMERA) if name == "box" else (_sphere(4), CAM_324)
    r = _renderer(mesh, cam, W, H)
    r.render(0, 8)
    raw = r.read_accum().reshape(H, W, 4)
    den = r.denoise()
    r.clear()
    r.render(0, 256)
    ref = r.read_accum().reshape(H, W, 4)
    e_raw, e_den = mse(raw, ref), mse(den, ref)
    print(f"denoise {name} 256x256: mse(8 spp) = {e_raw:.4e}, mse(8 spp denoised) = {e_den:.4e}")
    assert np.all(np.isfinite(den))
    assert e_den < e_raw


def test_multi_device_context_is_unsupported():
    L = ptamd.lib()
    g = ptamd.Renderer(devices=[0, 0])
    buf = np.zeros(64, np.float32)
    assert L.pt_render_guide(g._c) == PT_ERR_UNSUPPORTED
    assert L.pt_read_guide(g._c, buf.ctypes.data, buf.size) == PT_ERR_UNSUPPORTED
    assert L.pt_denoise(g._c, None, None, None) == PT_ERR_UNSUPPORTED
    assert L.pt_read_denoised(g._c, buf.ctypes.data, buf.size) == PT_ERR_UNSUPPORTED
    assert not L.pt_guide_device_ptr(g._c)


def test_pt_render_denoise_and_guide_flags(box, box_guide, tmp_path):
    W, H, spp = 64, 48, 2
    exe = os.path.join(PKG, "pt_render")
    out, gpath = str(tmp_path / "f.pfm"), str(tmp_path / "g.pfm")
    res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(W), "-h", str(H), "-spp", str(spp),
                          "-denoise", "-o", out, "-guide", gpath], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    r = _renderer(box, scenes.DEFAULT_CAMERA, W, H)
    r.render(0, spp)
    same(read_pfm(out), r.denoise()[..., :3], "pt_render -denoise")
    same(read_pfm(gpath), box_guide[..., :3], "pt_render -guide")
