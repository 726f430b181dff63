"""GPU: the seed base (PT_OPT_SEED_BASE).  With base B batch b draws from the
seed ((b + B) * H + py) * W + px and still folds with weight b: a one-sample
render at base B is the oracle's lone batch B before its division by B + 1;
fused launches fold like one-sample renders; every kernel path gives the same
bits; and dispatch and the progressive loop follow."""
import functools

import numpy as np
import pytest

import denoise_var_ref as V
import oracle_lib as O
import ptamd
import scenes
from support import bits, renderer, same, scene

pytestmark = pytest.mark.gpu

F = np.float32
CAM_324 = scenes.camera((3, 2, 4))
FRAMES = {"box": (scenes.DEFAULT_CAMERA, 64, 48), "sphere": (CAM_324, 67, 45)}   # edge tiles in both directions
LANES, MIX = ptamd.PT_OPT_SAMPLE_LANES, ptamd.PT_OPT_MIXED_LANES


def _renderer(name, options=(), moments=0):
    cam, W, H = FRAMES[name]
    return renderer(scene(name), cam, size=(W, H), options=[(ptamd.PT_OPT_MOMENTS, moments)] + list(options))


def _frame(r, base, n):
    r.set_option(ptamd.PT_OPT_SEED_BASE, base)
    r.clear()
    r.render(0, n)
    return r.read_accum().reshape(r.height, r.width, 4)


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_one_sample_at_base_b_is_the_oracles_batch_b(name):
    cam, W, H = FRAMES[name]
    v, i, n = scene(name)
    r = _renderer(name)
    for B in (0, 1, 3, 7):
        want, _ = O.render(v, i, n.reshape(-1), cam, scenes.REFERENCE_LIGHT, W, H, first_batch=B, n_batches=1)
        got = _frame(r, B, 1)
        # the oracle's last operation on a zero image: (0 * B + c) / float(B + 1)
        same(got / F(B + 1), want, f"{name}: base {B}")
    assert ptamd.lib().pt_set_option(r._c, ptamd.PT_OPT_SEED_BASE, -1) == -1   # PT_ERR_INVALID
    r.set_option(ptamd.PT_OPT_SEED_BASE, 2**31 - 1)


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_fused_launch_folds_like_one_sample_renders(name):
    _, W, H = FRAMES[name]
    r = _renderer(name, moments=1)
    singles = [_frame(r, 5 + j, 1) for j in range(4)]
    acc = np.zeros((H, W, 4), F)
    mom = np.zeros((H, W, 2), F)
    for j, c in enumerate(singles):
        acc = ((acc * F(j) + c) / F(j + 1)).astype(F)
        mom = V.fold_moments(mom, c, j)
    got = _frame(r, 5, 4)
    same(got, acc, f"{name}: render(0, 4) at base 5")
    m, n = r.read_moments()
    assert n == 4
    same(m, mom, f"{name}: moments at base 5")
    assert not np.array_equal(bits(got), bits(_frame(r, 0, 4)))             # another base, another frame


BOX_PATHS = {
    "lanes 1": [(MIX, 0), (LANES, 1)],
    "lanes 2": [(MIX, 0), (LANES, 2)],
    "lanes 4": [(MIX, 0), (LANES, 4)],
    "lanes 8": [(MIX, 0), (LANES, 8)],
    "mixed lanes": [(MIX, 50)],
    "sweep on": [(ptamd.PT_OPT_SMALL_SWEEP, 1)],
    "sweep off": [(ptamd.PT_OPT_SMALL_SWEEP, 0)],
    "sweep without hull faces": [(ptamd.PT_OPT_SWEEP_HULL, 0)],
    "scene not in LDS": [(ptamd.PT_OPT_SCENE_IN_LDS, 0)],
    "primary cull off": [(ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "wavefront, wide walk": [(ptamd.PT_OPT_KERNEL, 3)],
    "wavefront, threaded walk": [(ptamd.PT_OPT_KERNEL, 3), (ptamd.PT_OPT_WIDE, 0)],
    "wavefront, one batch per chunk": [(ptamd.PT_OPT_KERNEL, 3), (ptamd.PT_OPT_WF_PATHS, 1)],
}
SPHERE_PATHS = {
    "path-recursive, lanes 4": [(ptamd.PT_OPT_KERNEL, 1), (LANES, 4)],
    "scene not in LDS": [(ptamd.PT_OPT_SCENE_IN_LDS, 0)],
    "primary cull off": [(ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "wavefront, wide walk": [(ptamd.PT_OPT_KERNEL, 3)],
    "wavefront, threaded walk": [(ptamd.PT_OPT_KERNEL, 3), (ptamd.PT_OPT_WIDE, 0)],
    "wavefront, one batch per chunk": [(ptamd.PT_OPT_KERNEL, 3), (ptamd.PT_OPT_WF_PATHS, 1)],
}


@functools.lru_cache(maxsize=None)
def _reference_frames(name):
    r = _renderer(name)
    return {B: _frame(r, B, 4) for B in (5, 2**31 - 1)}


@pytest.mark.parametrize("name,path", [("box", p) for p in BOX_PATHS] + [("sphere", p) for p in SPHERE_PATHS])
def test_every_kernel_path_gives_the_same_frame(name, path):
    want = _reference_frames(name)
    r = _renderer(name, (BOX_PATHS if name == "box" else SPHERE_PATHS)[path])
    for B in (5, 2**31 - 1):
        same(_frame(r, B, 4), want[B], f"{name}, {path}: base {B}")
    assert not np.array_equal(bits(want[5]), bits(want[2**31 - 1]))


@pytest.mark.parametrize("mode", ["stats", "counting", "group"])
@pytest.mark.parametrize("name", ["box", "sphere"])
def test_stats_counting_and_group_members_follow(name, mode):
    """Stats mode (the reference-exhaustive walk), the counting kernels and a
    multi-device context (both members on device 0; it forwards the option)."""
    cam, W, H = FRAMES[name]
    want = _reference_frames(name)
    r = ptamd.Renderer(devices=[0, 0]) if mode == "group" else ptamd.Renderer(0)
    if mode == "counting":
        r.set_option(ptamd.PT_OPT_COUNT_TRACED, 1)
    r.upload_scene(*scene(name))
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_camera(cam)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    if mode == "stats":
        r.set_stats_mode(True)
    for B in (5, 2**31 - 1):
        same(_frame(r, B, 4), want[B], f"{name}, {mode}: base {B}")


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_dispatch_and_progressive_follow(name):
    cam, W, H = FRAMES[name]
    want = _reference_frames(name)[5]
    r = _renderer(name)
    r.set_option(ptamd.PT_OPT_SEED_BASE, 5)
    r.clear()
    for b in range(4):
        r.dispatch(b)
    same(r.read_accum(), want, f"{name}: dispatch")
    r.clear()
    assert r.progressive_camera(cam)
    assert r.progressive_advance(3) == (0, 3)
    assert r.progressive_advance(8, limit=4) == (3, 1)
    same(r.read_accum(), want, f"{name}: progressive")
