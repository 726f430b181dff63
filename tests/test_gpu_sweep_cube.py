"""GPU: the straight-line sweep of a cube table (PT_OPT_SWEEP_CUBE: every box of
the table other than the root is a hull face, sweep_walk.h sweep_cands_cube)
against the hull walk it replaces (option 0), against the walk of a table
without codes (PT_OPT_SWEEP_HULL 0) and against the threaded walk
(PT_OPT_SMALL_SWEEP 0), bitwise.  The box, a cuboid of three different extents
off the origin, the same seen from inside and the same without its top face run
the cube walk; the cuboid beside a triangle inside it (a general box) and
grid_mesh(2) must report that they do not, and match the threaded walk.
pt_sweep_walk tells which walk a frame ran.
"""
import functools

import numpy as np
import pytest

import oracle_lib
import ptamd
import scenes
import test_sweep_cube
import test_sweep_hull
from test_gpu_sweep import TWO_LIGHTS, _same
from test_gpu_sweep_hull import CASES as HULL_CASES

pytestmark = pytest.mark.gpu

W, H, SPP = 256, 144, 2
THREADED, PLAIN, HULL, CUBE = 0, 1, 2, 3   # pt_sweep_walk


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "box":
        s = ptamd.Scene.load_obj(scenes.BOX_OBJ)
    elif name == "cuboid-inward":
        s = ptamd.Scene.from_arrays(*test_sweep_hull.cuboid(outward=False))
    elif name in test_sweep_cube.MESHES:
        s = ptamd.Scene.from_arrays(*test_sweep_cube.MESHES[name]())
    else:
        s = ptamd.Scene.from_arrays(*scenes.grid_mesh(int(name.split(":")[1])))
    v, i, n, _, _ = s.build_bvh().arrays()
    return v, i, n


# name -> (scene, camera, lights, the walk the default options run)
CASES = {
    "box": ("box",) + HULL_CASES["box"][1:3] + (CUBE,),
    "cuboid": ("cuboid",) + HULL_CASES["cuboid"][1:3] + (CUBE,),
    "cuboid-inside": ("cuboid-inward",) + HULL_CASES["cuboid-inside"][1:3] + (CUBE,),
    "cuboid-open": ("cuboid-open",) + HULL_CASES["cuboid"][1:3] + (CUBE,),       # seen through the missing top
    "cuboid+tri": ("cuboid+tri",) + HULL_CASES["cuboid"][1:3] + (HULL,),
    "grid:2": ("grid:2", scenes.camera((0.0, 0.0, 3.0)), TWO_LIGHTS, PLAIN),
}


def _frame(v, i, n, cam, lights, walk_wanted, sweep=1, hull=1, cube=1, lanes=0, moments=0):
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_SMALL_SWEEP, sweep)
    r.set_option(ptamd.PT_OPT_SWEEP_HULL, hull)
    r.set_option(ptamd.PT_OPT_SWEEP_CUBE, cube)
    r.set_option(ptamd.PT_OPT_SAMPLE_LANES, lanes)
    r.set_option(ptamd.PT_OPT_MOMENTS, moments)
    r.upload_scene(v, i, n)
    r.upload_lights(lights)
    r.set_camera(cam)
    r.set_params(4, 3)
    assert r.sweep_walk() == walk_wanted, f"pt_sweep_walk {r.sweep_walk()}, expected {walk_wanted}"
    assert (r.sweep_info()[1] == i.size // 3) == (walk_wanted != THREADED)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    out = r.read_accum()
    mom = r.read_moments()[0] if moments else None
    r.close()
    assert np.count_nonzero(np.any(out.reshape(-1, 4)[:, :3] != 0, axis=1)) >= 200, "the frame shows the scene lit"
    return (out, mom) if moments else out


@pytest.mark.parametrize("name", list(CASES))
def test_cube_on_off_hull_off_and_threaded_walk_bitwise(name):
    scene, cam, lights, walk = CASES[name]
    v, i, n = _scene(scene)
    st, info = test_sweep_cube.cube_check(v, i, n.reshape(-1), np.ones((1, 8), np.float32))
    assert info[3] == (walk == CUBE), f"{name}: SmallSweep::cube {info[3]}"
    on = _frame(v, i, n, cam, lights, walk)
    _same(_frame(v, i, n, cam, lights, min(walk, HULL), cube=0), on, f"{name}: PT_OPT_SWEEP_CUBE 0 against 1")
    _same(_frame(v, i, n, cam, lights, PLAIN, hull=0), on, f"{name}: PT_OPT_SWEEP_HULL 0 against the default walk")
    _same(_frame(v, i, n, cam, lights, THREADED, sweep=0), on, f"{name}: the threaded walk against the default walk")


@functools.lru_cache(maxsize=None)
def _box_frame():
    scene, cam, lights, _ = CASES["box"]
    return _frame(*_scene(scene), cam, lights, CUBE)


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_box_sample_lanes(lanes):
    scene, cam, lights, _ = CASES["box"]
    v, i, n = _scene(scene)
    on = _frame(v, i, n, cam, lights, CUBE, lanes=lanes)
    _same(on, _box_frame(), f"box: {lanes} sample lanes against the default")
    _same(_frame(v, i, n, cam, lights, HULL, cube=0, lanes=lanes), on, f"box: {lanes} lanes, PT_OPT_SWEEP_CUBE 0 against 1")


def test_box_moments():
    scene, cam, lights, _ = CASES["box"]
    v, i, n = _scene(scene)
    on, mom_on = _frame(v, i, n, cam, lights, CUBE, moments=1)
    off, mom_off = _frame(v, i, n, cam, lights, HULL, cube=0, moments=1)
    _same(on, _box_frame(), "box: the MOMENTS instantiation's accumulator against the plain one's")
    _same(off, on, "box with PT_OPT_MOMENTS: PT_OPT_SWEEP_CUBE 0 against 1")
    _same(mom_off.reshape(-1), mom_on.reshape(-1), "box: the moments, PT_OPT_SWEEP_CUBE 0 against 1")
    assert np.count_nonzero(mom_on) >= 200


def test_box_equals_oracle():
    scene, cam, lights, _ = CASES["box"]
    v, i, n = _scene(scene)
    ref, _ = oracle_lib.render(v, i, n.reshape(-1), cam, lights, W, H, n_batches=SPP)
    _same(_box_frame(), ref, "box on the cube walk against the oracle")


def test_option_range():
    r = ptamd.Renderer(0)
    for bad in (-1, 2):
        with pytest.raises(ptamd.PTError, match="PT_OPT_SWEEP_CUBE"):
            r.set_option(ptamd.PT_OPT_SWEEP_CUBE, bad)
    r.close()
