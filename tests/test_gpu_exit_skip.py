"""GPU: the exit skip (PT_OPT_EXIT_SKIP, csrc/pt_isect.h exit_skip, DESIGN.md
section 4) on every fast path tracer.

After a hit whose stored normal is axis-pure, at a point that lies (offset
along the normal) beyond the root box's face on that side, the bounce ray
misses the root box whatever its hemisphere draws, and the kernels end the path
instead of sampling and tracing it.  The frame cannot show whether they did:
each case renders with the option on and off and both frames must be the
oracle's bit for bit.  Counting mode (PT_OPT_COUNT_TRACED) shows it: the walks
not started.

Scenes: box.obj (every hit from outside fires); the same cube rotated by 0.05
rad about (1, 2, 3) (no axis-pure normal: the host never sets the flag);
floor_and_cloud (the floor is the root's lo face with its normal pointing up,
into the root: evaluated, never true on the floor); the same with the floor's
winding reversed (normal down: fires); flat_quad (lo.z == hi.z).  Frames are
64x48 at 3 spp in two launches; each oracle frame is computed once.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import ptamd
import scenes
from support import lit_pixels, oracle_frame, renderer, same, scene

pytestmark = pytest.mark.gpu

W, H, NB = 64, 48, 3
ALL_TAIL, NO_TAIL = 1 << 30, 1
EXIT = ptamd.PT_OPT_EXIT_SKIP


def _box_arrays():
    return scene("box")[:2]


def _rotated_cube():
    v, i = _box_arrays()
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    a = 0.05
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    return (v.reshape(-1, 3).astype(np.float64) @ R.T).astype(np.float32).reshape(-1), i


def _floor_reversed():
    v, i = scenes.floor_and_cloud()
    t = i.reshape(-1, 3).copy()
    t[-2:] = t[-2:, [0, 2, 1]]
    return v, t.reshape(-1)


CLOUD_CAM = scenes.camera((0.3, 0.4, 2.2))
SCENES = {   # name: (vertices and indices, camera, fits in LDS)
    "box": (_box_arrays, scenes.DEFAULT_CAMERA, True),
    "rotated_cube": (_rotated_cube, scenes.DEFAULT_CAMERA, True),
    "floor_and_cloud": (scenes.floor_and_cloud, CLOUD_CAM, False),
    "floor_reversed": (_floor_reversed, CLOUD_CAM, False),
    "flat_quad": (scenes.flat_quad, scenes.DEFAULT_CAMERA, True),
}


MAKERS = {name: make for name, (make, _, _) in SCENES.items()}


def _scene(name):
    return scene(name, MAKERS) + SCENES[name][1:]


@functools.lru_cache(maxsize=None)
def _oracle(name, depth=4, sss=3):
    ref = oracle_frame(scene(name, MAKERS), SCENES[name][1], scenes.REFERENCE_LIGHT, W, H, 0, NB, depth, sss, nthreads=8)
    lit = lit_pixels(ref)
    assert lit >= 100, f"{name}: the oracle's frame shows {lit} lit pixels"
    return ref


K, LDS, SWEEP, HULL = ptamd.PT_OPT_KERNEL, ptamd.PT_OPT_SCENE_IN_LDS, ptamd.PT_OPT_SMALL_SWEEP, ptamd.PT_OPT_SWEEP_HULL
WIDE, TAIL = ptamd.PT_OPT_WIDE, ptamd.PT_OPT_WF_TAIL
# name: (options, needs the scene in LDS, kernel)
VARIANTS = {
    "sweep_hull": ({K: 1, SWEEP: 1, HULL: 1}, True, ptamd.KERNEL_RECURSIVE),
    "sweep_plain": ({K: 1, SWEEP: 1, HULL: 0}, True, ptamd.KERNEL_RECURSIVE),
    "lds_threaded": ({K: 1, SWEEP: 0, LDS: 2}, True, ptamd.KERNEL_RECURSIVE),
    "device_memory": ({K: 1, LDS: 0}, False, ptamd.KERNEL_RECURSIVE),
    "wf_threaded": ({K: 3, LDS: 0, WIDE: 0}, False, ptamd.KERNEL_WAVEFRONT),
    "wf_wide": ({K: 3, LDS: 0, WIDE: 1, TAIL: NO_TAIL}, False, ptamd.KERNEL_WAVEFRONT),
    "wf_tail": ({K: 3, LDS: 0, WIDE: 1, TAIL: ALL_TAIL}, False, ptamd.KERNEL_WAVEFRONT),
}
# the counting kernels run the threaded walk: the sweep variants have none
COUNTING = ["lds_threaded", "device_memory", "wf_threaded", "wf_wide", "wf_tail"]
CASES = [(s, k) for s in SCENES for k in VARIANTS if SCENES[s][2] or not VARIANTS[k][1]]


def _renderer(name, variant, exit_skip, depth=4, sss=3, lights=scenes.REFERENCE_LIGHT, count=False):
    v, i, n, cam, _ = _scene(name)
    opts, _, _ = VARIANTS[variant]
    r = renderer((v, i, n), cam, lights, depth, sss,
                 options=list(opts.items()) + [(EXIT, exit_skip)] + ([(ptamd.PT_OPT_COUNT_TRACED, 1)] if count else []))
    if variant.startswith("sweep") and not count:
        assert r.sweep_info()[1] == i.size // 3, r.sweep_info()
    if opts.get(WIDE) == 1:
        assert r.wide_info()[0] > 0, r.wide_info()
    return r


@pytest.mark.parametrize("name,variant", CASES, ids=[f"{s}-{k}" for s, k in CASES])
def test_frames_equal_the_oracle(name, variant):
    ref = _oracle(name)
    for exit_skip in (1, 0):
        r = _renderer(name, variant, exit_skip)
        r.resize_and_clear(W, H)
        r.render(0, 1)
        r.render(1, NB - 1)
        same(r.read_accum(), ref, f"{name} {variant}, PT_OPT_EXIT_SKIP {exit_skip}")
        assert r.last_kernel() == VARIANTS[variant][2]
        r.close()


def _counts(name, variant, exit_skip, depth, sss, ref, lights=scenes.REFERENCE_LIGHT, nan_ok=False):
    r = _renderer(name, variant, exit_skip, depth, sss, lights, count=True)
    r.resize_and_clear(W, H)
    r.reset_stats()
    r.render(0, 1)
    r.render(1, NB - 1)
    gpu = r.read_accum()
    if nan_ok:   # NaNs as NaN (their sign and payload are the platform's), every other float bitwise
        nan_g, nan_r = np.isnan(gpu), np.isnan(ref)
        assert np.array_equal(nan_g, nan_r)
        gpu, ref = np.where(nan_g, 0, gpu).astype(np.float32), np.where(nan_r, 0, ref).astype(np.float32)
    same(gpu, ref, f"counting: {name} {variant}, PT_OPT_EXIT_SKIP {exit_skip}")
    t = r.traced()
    r.close()
    return t


STARTED = ("closest_walks", "shadow_walks", "primaries")


def _same_work(variant, on, off):
    """The same walks started; on the path-recursive kernels also the same node visits and triangle
    tests (a wavefront list's order, and with it what the culled wide walk visits, varies from run to run)."""
    if VARIANTS[variant][2] == ptamd.KERNEL_RECURSIVE:
        return on == off
    return all(on[k] == off[k] for k in STARTED)


def test_box_every_bounce_skipped():
    """max_depth 2, sss_bounces 0: the only closest walks beside the primaries
    are the bounce rays of the depth-0 hits, all of which leave the cube."""
    ref = _oracle("box", 2, 0)
    on = {k: _counts("box", k, 1, 2, 0, ref) for k in COUNTING}
    off = {k: _counts("box", k, 0, 2, 0, ref) for k in COUNTING}
    first_on, first_off = on[COUNTING[0]], off[COUNTING[0]]
    for k in COUNTING:
        print(k, "on", on[k], "off", off[k])
        assert on[k]["primaries"] > 0
        assert on[k]["closest_walks"] == on[k]["primaries"], (k, on[k])
        assert off[k]["closest_walks"] > off[k]["primaries"], (k, off[k])
        for key in STARTED:
            assert on[k][key] == first_on[key] and off[k][key] == first_off[key], (k, key, on[k], off[k])
        assert on[k]["shadow_walks"] == off[k]["shadow_walks"] and on[k]["primaries"] == off[k]["primaries"]


def test_box_full_depth_counts_agree():
    """4 bounces, 3 SSS steps (the benchmark's): fewer closest walks with the
    option on, the same on every kernel."""
    ref = _oracle("box")
    on = {k: _counts("box", k, 1, 4, 3, ref) for k in COUNTING}
    off = {k: _counts("box", k, 0, 4, 3, ref) for k in COUNTING}
    for k in COUNTING:
        print(k, "on", on[k], "off", off[k])
        for key in STARTED:
            assert on[k][key] == on[COUNTING[0]][key] and off[k][key] == off[COUNTING[0]][key], (k, key)
        assert on[k]["primaries"] < on[k]["closest_walks"] < off[k]["closest_walks"]


@pytest.mark.parametrize("variant", COUNTING)
def test_rotated_cube_counts_unchanged(variant):
    ref = _oracle("rotated_cube")
    on, off = _counts("rotated_cube", variant, 1, 4, 3, ref), _counts("rotated_cube", variant, 0, 4, 3, ref)
    assert _same_work(variant, on, off) and on["closest_walks"] > on["primaries"] > 0, (on, off)


@pytest.mark.parametrize("variant", ["device_memory", "wf_threaded", "wf_wide", "wf_tail"])
def test_floors(variant):
    """The floor with its normal up (into the root) never fires; reversed, every hit on it does."""
    ref = _oracle("floor_and_cloud")
    on, off = _counts("floor_and_cloud", variant, 1, 4, 3, ref), _counts("floor_and_cloud", variant, 0, 4, 3, ref)
    assert _same_work(variant, on, off), (on, off)
    ref = _oracle("floor_reversed")
    on, off = _counts("floor_reversed", variant, 1, 4, 3, ref), _counts("floor_reversed", variant, 0, 4, 3, ref)
    assert on["closest_walks"] < off["closest_walks"], (on, off)
    assert on["shadow_walks"] == off["shadow_walks"] and on["primaries"] == off["primaries"]


@pytest.mark.parametrize("variant", ["lds_threaded", "wf_tail"])
def test_non_finite_light_disables_the_skip(variant):
    """Condition 4: with an infinite intensity the host leaves the flag clear --
    the counts with the option on are those with it off -- and the frame is
    still the oracle's."""
    v, i, n, cam, _ = _scene("box")
    lights = np.concatenate([scenes.REFERENCE_LIGHT,
                             ptamd.pack_light([-2.5, 0.0, 0.5], [1, 0, 0], [np.inf, 1.0, 0.25], [0.5, 0.5])])
    ref, _ = O.render(v, i, n.reshape(-1), cam, lights, W, H, first_batch=0, n_batches=NB, max_depth=2, sss_bounces=0,
                      nthreads=8)
    on = _counts("box", variant, 1, 2, 0, ref, lights, nan_ok=True)
    off = _counts("box", variant, 0, 2, 0, ref, lights, nan_ok=True)
    assert _same_work(variant, on, off) and on["closest_walks"] > on["primaries"] > 0, (on, off)


def test_option_values():
    r = ptamd.Renderer(0)
    with pytest.raises(ptamd.PTError, match="PT_OPT_EXIT_SKIP"):
        r.set_option(EXIT, 2)
    r.close()
