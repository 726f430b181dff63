"""The cube table of the sweep walk (scene/small_sweep.h SmallSweep::cube,
csrc/sweep_walk.h sweep_cands_cube) on the CPU.

A table in which every box other than the root is a hull face of it -- no
general box, every flat box coded, one box per (axis, code): the box, a cuboid,
a cuboid without one face -- is walked straight-line: the root's six products,
its test, then the six faces with their axis and code fixed at compile time and
their under words handed in.  tests/sweep_cube_check.cpp compiles the header
for the host and compares, per ray, sweep_cands_cube's leaf mask and `none`
with sweep_cands<true> (the walk it replaces) and with
sweep_leaves(sweep_mask(...)), which goes through slab for every box; the
predicate with its definition; cube_under[] and cube_all with under[] by value.
At least 10^6 rays per scene: sweep_support.make_rays' families (origins inside
the root and on face planes, zero direction components, rays lying in face
planes) and, on the root's planes, direction components of 0, -0 and
subnormals, origins a few ulp to either side, and axis-parallel rays.
"""
import functools

import numpy as np
import pytest

from sweep_support import cube_check, make_rays, plane_rays, run_main, scene

N_RAYS = 1 << 20
CUBE_SCENES = {"box": 6, "cuboid": 6, "cuboid-open": 5}          # name -> faces
OTHER_SCENES = ["grid:2", "tri:4", "cuboid+tri", "cuboids-stacked"]


@functools.lru_cache(maxsize=None)
def rays_of(name):
    v, idx, _ = scene(name)
    V = v.reshape(-1, 3)
    half = N_RAYS // 2
    return np.concatenate([make_rays(v, idx, half, seed=len(name) * 263 + idx.size),
                           plane_rays(V.min(0), V.max(0), N_RAYS - half, seed=len(name) * 911 + 7)])


@pytest.mark.parametrize("name", list(CUBE_SCENES))
def test_cube_walk_equals_hull_walk_and_two_passes(name):
    v, idx, nodes = scene(name)
    rays = rays_of(name)
    assert len(rays) >= 10 ** 6
    st, (boxes, leaves, n_hull, cube, faces) = cube_check(v, idx, nodes, rays)
    first = int(st[3])
    where = f"{name}: first bad ray {first}: {rays[first % len(rays)]}"
    print(f"{name}: boxes {boxes} leaves {leaves} faces {faces}; differing masks {int(st[0])}, none {int(st[1])}, "
          f"two-pass {int(st[2])}; root pass {int(st[6])} fail {int(st[7])}, NaN products {int(st[10])}")
    assert leaves == idx.size // 3
    assert int(st[4]) == 0, f"{name}: SmallSweep::cube differs from its definition"
    assert cube == 1 and faces == CUBE_SCENES[name] and boxes == 1 + faces and n_hull == faces
    assert int(st[5]) == 0, f"{name}: cube_under[] / cube_all differ from under[]"
    assert int(st[11]) == len(rays)
    assert (int(st[0]), int(st[1])) == (0, 0), f"leaf mask / none differ from sweep_cands<true>: {st[:2]}; {where}"
    assert int(st[2]) == 0, f"leaf mask / none differ from sweep_leaves(sweep_mask): {st[2]}; {where}"
    # coverage, so that the pass means something
    assert int(st[8]) == (1 << leaves) - 1, f"{name}: leaf bits never set in a mask: {(1 << leaves) - 1 - int(st[8]):#x}"
    assert st[6] > 0 and st[7] > 0 and st[9] > 0, "rays passing the root box, rays failing it, candidates"
    assert st[10] > 0, "rays with a NaN among the root's products (0 * inf)"


@pytest.mark.parametrize("name", OTHER_SCENES)
def test_other_tables_are_not_cube_tables(name):
    v, idx, nodes = scene(name)
    st, (boxes, leaves, n_hull, cube, faces) = cube_check(v, idx, nodes, np.ones((1, 8), np.float32))
    assert leaves == idx.size // 3
    assert int(st[4]) == 0, f"{name}: SmallSweep::cube differs from its definition"
    assert cube == 0 and faces == 0, f"{name}: {boxes} boxes, {n_hull} coded"
    assert int(st[5]) == 0, f"{name}: cube_under[] / cube_all are not zero without a cube table"
    assert int(st[11]) == 0
    if name == "cuboid+tri":
        assert n_hull == 6 and boxes > 7, "the six faces keep their codes beside the general box"


def test_standalone_program():
    """The harness's own main builds and passes: a cuboid (six faces), the same without one face (five), and the
    whole one beside a triangle inside it (no cube table)."""
    out = run_main("sweep_cube_check", "SWEEP_CUBE_MAIN")
    lines = out.strip().splitlines()
    assert len(lines) == 3, out
    assert "boxes=7 leaves=12 hull_boxes=6 cube=1 faces=6 mask=0 none=0 two_pass=0 predicate=0 under=0" in lines[0], out
    assert "boxes=6 leaves=10 hull_boxes=5 cube=1 faces=5 mask=0 none=0 two_pass=0 predicate=0 under=0" in lines[1], out
    assert "boxes=8 leaves=13 hull_boxes=6 cube=0 faces=0 mask=0 none=0 two_pass=0 predicate=0 under=0" in lines[2], out
