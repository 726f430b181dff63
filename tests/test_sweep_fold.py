"""The one-pass sweep (csrc/sweep_walk.h sweep_cands: each box's record carries
the leaves it guards) against its two-pass restatement and the threaded walk,
on the CPU.

tests/sweep_fold_check.cpp compiles the header for the host and, from one
packed table, compares per ray: the leaf mask and `none` of sweep_cands with
those of sweep_leaves(sweep_mask(...)); the sweep past the root's test with
the two passes run without the early exit (what a lane computes that fails
the root while another lane of its wave passes); the closest hit and the
shadow answer taken from the new mask with the threaded walk's, bit for bit.
It also checks every box's under word against its definition from need[],
the table's order (root, general, x-, y-, z-flat boxes) against the boxes, and
the flat loops' slab test against slab on every ray and flat box.
The rays are sweep_support.make_rays': zero direction components (NaNs in the
slab test), origins inside the root and on face planes, and a family aimed at
every triangle.
"""
import numpy as np
import pytest

from sweep_support import fold_check, make_rays, run_main, scene

SCENES = ["box", "grid:2", "grid:3", "tri:1", "tri:3", "tri:8", "tri:32"]


@pytest.mark.parametrize("name", SCENES)
def test_fold_equals_two_passes_and_threaded_walk(name):
    v, idx, nodes = scene(name)
    rays = make_rays(v, idx, 6000, seed=len(name) * 131 + idx.size)
    st, boxes, leaves, slots, flat = fold_check(v, idx, nodes, rays)
    first = int(st[5])
    where = f"{name}: first bad ray {first}: {rays[first % len(rays)]}"
    assert leaves == idx.size // 3 and sorted(slots) == list(range(leaves))
    if name == "tri:32":
        assert boxes == 63, "the table past 32 boxes (64-bit need words) is in force"
    assert int(st[12]) == 0, f"{name}: {int(st[12])} boxes whose under word is not {{l : need[l] has the box's bit}}"
    assert (int(st[0]), int(st[1])) == (0, 0), f"leaf mask / none differ from sweep_leaves(sweep_mask): {st[:2]}; {where}"
    assert int(st[2]) == 0, f"the sweep past the root differs from the two passes without the early exit: {st[2]}; {where}"
    assert (int(st[3]), int(st[4])) == (0, 0), f"closest hit / shadow differ from the threaded walk: {st[3:5]}; {where}"
    assert int(st[15]) == 0, f"{name}: {int(st[15])} boxes out of the table's order root, general, x-, y-, z-flat"
    assert int(st[13]) == 0, f"{name}: sweep_slab_flat differs from slab on {int(st[13])} (ray, box) pairs"
    # every axis-aligned face is flat: the box's six, the quads of the grids; counted here from the
    # nodes' distinct boxes, the root's apart.  Rays lying in a vertex plane give them a NaN on the
    # flat axis (0 * inf)
    nd = np.ascontiguousarray(nodes, np.float32).reshape(-1, 8)
    distinct = {r[[0, 1, 2, 4, 5, 6]].tobytes(): bool((r[0:3].view(np.uint32) == r[4:7].view(np.uint32)).any())
                for r in nd[1:] if r[[0, 1, 2, 4, 5, 6]].tobytes() != nd[0][[0, 1, 2, 4, 5, 6]].tobytes()}
    assert len(distinct) == boxes - 1 and flat == sum(distinct.values())
    if name == "box":
        assert flat == 6
    if name.startswith(("box", "grid")):
        assert flat >= 4 and st[14] > 0, "flat boxes, and rays whose t on the flat axis is NaN"
    # coverage, so that the pass means something
    assert int(st[6]) == (1 << leaves) - 1, f"{name}: leaf bits never set in a mask: {(1 << leaves) - 1 - int(st[6]):#x}"
    assert st[7] > 0 and st[8] > 0, "rays failing the root box and rays passing it"
    assert st[9] > 0 and st[10] > 0 and st[11] > 0, "the rays reach the geometry"


def test_standalone_program():
    """The harness's own main (the program meant for host sanitizer runs)
    builds and passes on its built-in scene: a cube of flat face boxes plus a
    tilted triangle."""
    out = run_main("sweep_fold_check", "SWEEP_FOLD_MAIN")
    assert "leaves=13 flat_boxes=6 mask=0 none=0 riding=0 hit=0 shadow=0 under=0 flat=0 order=0" in out, out
