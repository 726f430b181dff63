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

import ptamd
import scenes
from support import TWO_LIGHTS, lit_pixels, oracle_frame, renderer, same, scene
from sweep_support import GPU_MAKERS as MAKERS, HULL_CASES, cube_check

pytestmark = pytest.mark.gpu

W, H, SPP = 256, 144, 2
THREADED, PLAIN, HULL, CUBE = 0, 1, 2, 3   # pt_sweep_walk


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
    r = renderer((v, i, n), cam, lights, options=[
        (ptamd.PT_OPT_SMALL_SWEEP, sweep), (ptamd.PT_OPT_SWEEP_HULL, hull), (ptamd.PT_OPT_SWEEP_CUBE, cube),
        (ptamd.PT_OPT_SAMPLE_LANES, lanes), (ptamd.PT_OPT_MOMENTS, moments)])
    assert r.sweep_walk() == walk_wanted, f"pt_sweep_walk {r.sweep_walk()}, expected {walk_wanted}"
    assert (r.sweep_info()[1] == i.size // 3) == (walk_wanted != THREADED)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    out = r.read_accum()
    mom = r.read_moments()[0] if moments else None
    r.close()
    assert lit_pixels(out) >= 200, "the frame shows the scene lit"
    return (out, mom) if moments else out


@pytest.mark.parametrize("name", list(CASES))
def test_cube_on_off_hull_off_and_threaded_walk_bitwise(name):
    mesh, cam, lights, walk = CASES[name]
    v, i, n = scene(mesh, MAKERS)
    st, info = cube_check(v, i, n.reshape(-1), np.ones((1, 8), np.float32))
    assert info[3] == (walk == CUBE), f"{name}: SmallSweep::cube {info[3]}"
    on = _frame(v, i, n, cam, lights, walk)
    same(_frame(v, i, n, cam, lights, min(walk, HULL), cube=0), on, f"{name}: PT_OPT_SWEEP_CUBE 0 against 1")
    same(_frame(v, i, n, cam, lights, PLAIN, hull=0), on, f"{name}: PT_OPT_SWEEP_HULL 0 against the default walk")
    same(_frame(v, i, n, cam, lights, THREADED, sweep=0), on, f"{name}: the threaded walk against the default walk")


@functools.lru_cache(maxsize=None)
def _box_frame():
    mesh, cam, lights, _ = CASES["box"]
    return _frame(*scene(mesh, MAKERS), cam, lights, CUBE)


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_box_sample_lanes(lanes):
    mesh, cam, lights, _ = CASES["box"]
    v, i, n = scene(mesh, MAKERS)
    on = _frame(v, i, n, cam, lights, CUBE, lanes=lanes)
    same(on, _box_frame(), f"box: {lanes} sample lanes against the default")
    same(_frame(v, i, n, cam, lights, HULL, cube=0, lanes=lanes), on, f"box: {lanes} lanes, PT_OPT_SWEEP_CUBE 0 against 1")


def test_box_moments():
    mesh, cam, lights, _ = CASES["box"]
    v, i, n = scene(mesh, MAKERS)
    on, mom_on = _frame(v, i, n, cam, lights, CUBE, moments=1)
    off, mom_off = _frame(v, i, n, cam, lights, HULL, cube=0, moments=1)
    same(on, _box_frame(), "box: the MOMENTS instantiation's accumulator against the plain one's")
    same(off, on, "box with PT_OPT_MOMENTS: PT_OPT_SWEEP_CUBE 0 against 1")
    same(mom_off.reshape(-1), mom_on.reshape(-1), "box: the moments, PT_OPT_SWEEP_CUBE 0 against 1")
    assert np.count_nonzero(mom_on) >= 200


def test_box_equals_oracle():
    mesh, cam, lights, _ = CASES["box"]
    v, i, n = scene(mesh, MAKERS)
    same(_box_frame(), oracle_frame(scene(mesh, MAKERS), cam, lights, W, H, nb=SPP), "box on the cube walk against the oracle")


def test_option_range():
    r = ptamd.Renderer(0)
    for bad in (-1, 2):
        with pytest.raises(ptamd.PTError, match="PT_OPT_SWEEP_CUBE"):
            r.set_option(ptamd.PT_OPT_SWEEP_CUBE, bad)
    r.close()
