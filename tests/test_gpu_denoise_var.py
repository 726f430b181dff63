"""GPU: the variance-guided a-trous filter (pt_denoise_var) on rendered frames
and their moments: the pass kernels against the host's run of the same header
code (pt_denoise_var_host) and the independent numpy restatement
(tests/denoise_var_ref.py), bit for bit, on both kernel shapes and into a
caller-owned image; the pt_render flag; and that the filter lowers the error of
a frame at 8 and at 32 samples, where pt_denoise's fixed colour sigma does not."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import denoise_var_ref as R
import ptamd
import scenes
from support import PKG, bits, mse, read_pfm, renderer, same, scene

pytestmark = pytest.mark.gpu

PT_OK, PT_ERR_INVALID = 0, -1
CAM_324 = scenes.camera((3, 2, 4))
FRAMES = {"box": (scenes.DEFAULT_CAMERA, 64, 48), "sphere": (CAM_324, 67, 45)}   # edge tiles in both directions


def _renderer(name, W=None, H=None, moments=1):
    cam, w, h = FRAMES[name]
    return renderer(scene(name), cam, size=(W or w, H or h), options=[(ptamd.PT_OPT_MOMENTS, moments)])


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_device_filter_matches_host_and_restatement(name):
    _, W, H = FRAMES[name]
    r = _renderer(name)
    r.render(0, 8)
    accum = r.read_accum().reshape(H, W, 4)
    moments, n = r.read_moments()
    assert n == 8
    r.render_guide()
    guide = r.read_guide()
    assert np.any(moments[..., 1] > moments[..., 0] * moments[..., 0])
    for params in (None, (1, 1.5, 0.35, 0.25), (3, 0.75, 0.5, 0.25), (6, 4.0, 0.35, 0.5)):
        ref = R.atrous_var(accum, moments, n, guide, W, H, R.DEFAULTS if params is None else params)
        assert np.all(np.isfinite(ref))
        same(ptamd.denoise_var_host(accum, moments, n, guide, W, H, params), ref, f"{name}: host, {params}")
        for staged in (0, 1):
            r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            same(r.denoise_var(params), ref, f"{name}: device, {params}, staged {staged}")
    same(r.read_accum().reshape(H, W, 4), accum, "the accumulation image after the filter")
    same(r.read_moments()[0], moments, "the moments after the filter")
    assert not np.array_equal(bits(ref[..., :3]), bits(accum[..., :3]))


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_caller_owned_destination(name):
    _, W, H = FRAMES[name]
    r = _renderer(name)
    r.render(0, 8)                                  # the guide is rendered by the call
    want = r.denoise_var()
    dst = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert r.denoise_var(None, dst.data_ptr()) is None
    r.synchronize()
    same(dst.cpu().numpy(), want, f"{name}: caller-owned destination")
    L = ptamd.lib()
    assert L.pt_denoise_var(r._c, None, dst.data_ptr() + 4) == PT_ERR_INVALID      # misaligned
    assert L.pt_denoise_var(r._c, None, r.accum_ptr()) == PT_ERR_INVALID           # accum onto itself
    for bad in [(0, 1.5, 0.35, 0.25), (7, 1.5, 0.35, 0.25), (5, 0.0, 0.35, 0.25), (5, float("nan"), 0.35, 0.25),
                (5, 1.5, float("inf"), 0.25), (5, 1.5, 0.35, 1e-30)]:
        assert L.pt_denoise_var(r._c, ptamd.DenoiseVarParams(*bad), None) == PT_ERR_INVALID, bad


def test_calls_without_inputs_are_invalid():
    L = ptamd.lib()
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    assert L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID     # no scene
    r.upload_scene(*scene("box"))
    assert L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID     # no camera
    r.set_camera(scenes.DEFAULT_CAMERA)
    assert L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID     # no frame
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.resize_and_clear(20, 12)
    assert L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID     # no moments yet
    r.render(0, 2)
    assert r.denoise_var().shape == (12, 20, 4)


def test_pt_render_denoise_var_flag(tmp_path):
    W, H, spp = 64, 48, 4
    exe = os.path.join(PKG, "pt_render")
    out = str(tmp_path / "f.pfm")
    res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(W), "-h", str(H), "-spp", str(spp),
                          "-denoise-var", "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    r = _renderer("box")
    r.render(0, spp)
    same(read_pfm(out), r.denoise_var()[..., :3], "pt_render -denoise-var")


@functools.lru_cache(maxsize=None)
def _converged(name):
    r = _renderer(name, 96, 96, moments=0)
    r.render(0, 256)
    return r.read_accum().reshape(96, 96, 4)


@pytest.mark.parametrize("spp", [8, 32])
@pytest.mark.parametrize("name", ["box", "sphere"])
def test_it_denoises_at_every_sample_count(name, spp):
    """96x96, default parameters, against 256 spp of the same view: the
    variance-guided frame is closer than the raw one at 8 and at 32 spp.
    pt_denoise's figures are printed beside them (at 32 spp its fixed
    sigma_color makes the frame worse than raw)."""
    W = H = 96
    ref = _converged(name)
    r = _renderer(name, W, H)
    r.render(0, spp)
    raw = r.read_accum().reshape(H, W, 4)
    var = r.denoise_var()
    fixed = r.denoise()
    e_raw, e_var, e_fixed = mse(raw, ref), mse(var, ref), mse(fixed, ref)
    print(f"denoise_var {name} 96x96 {spp} spp: mse raw = {e_raw:.4e}, pt_denoise_var = {e_var:.4e} "
          f"({e_var / e_raw:.3f} of raw), pt_denoise = {e_fixed:.4e} ({e_fixed / e_raw:.3f} of raw)")
    assert np.all(np.isfinite(var))
    assert e_var < e_raw
