"""The hull faces of the sweep table (scene/small_sweep.h, csrc/sweep_walk.h
sweep_slab_hull) on the CPU.

A flat box of the table that is a face of the root box -- its flat coordinate
bitwise the root's lo or hi on that axis, its other four extents bitwise the
root's -- carries a code, and sweep_cands tests it with the slab products the
root's test formed instead of its own.  tests/sweep_hull_check.cpp compiles
the header for the host and compares, per ray, sweep_cands' leaf mask and
`none` with sweep_leaves(sweep_mask(...)), which goes through slab for every
box; the same for the table packed without codes (PT_OPT_SWEEP_HULL 0) and for
a lane riding along past a failed root test; sweep_slab_hull with slab on every
(ray, coded box); and every code with its definition by memcmp.  The rays are
sweep_support.make_rays': zero direction components (NaNs in the slab test),
origins inside the root and on face planes, rays lying in face planes.
"""
import pytest

from sweep_support import MOVED_BOXES, hull_check, make_rays, run_main, scene

# the flat quad's only box is the root
SCENES = ["box", "cuboid", "grid:2", "tri:4"] + MOVED_BOXES + ["flat_quad", "tri4:copies8"]


@pytest.mark.parametrize("name", SCENES)
def test_hull_faces_equal_slab(name):
    v, idx, nodes = scene(name)
    rays = make_rays(v, idx, 6000, seed=len(name) * 257 + idx.size)
    st, (boxes, leaves, flat, coded, n_hull) = hull_check(v, idx, nodes, rays)
    first = int(st[5])
    where = f"{name}: first bad ray {first}: {rays[first % len(rays)]}"
    assert leaves == idx.size // 3
    assert int(st[6]) == 0, f"{name}: codes that differ from their definition, or a table without codes that has one"
    assert coded == n_hull <= flat
    assert (int(st[0]), int(st[1])) == (0, 0), f"leaf mask / none differ from sweep_leaves(sweep_mask): {st[:2]}; {where}"
    assert int(st[2]) == 0, f"the table without codes differs from sweep_leaves(sweep_mask): {st[2]}; {where}"
    assert int(st[3]) == 0, f"the sweep past the root differs from the two passes without the early exit: {st[3]}; {where}"
    assert int(st[4]) == 0, f"sweep_slab_hull differs from slab on {int(st[4])} (ray, box) pairs; {where}"
    if name == "box" or name in MOVED_BOXES:
        assert (boxes, flat, coded) == (7, 6, 6), "the box's six face boxes are hull faces"
    if name == "flat_quad":
        assert (boxes, leaves, coded) == (1, 2, 0), "the root alone: nothing to share its products with"
    if name == "cuboid":
        assert coded >= 2, "the cuboid has hull faces"
    if name.startswith("tri"):
        assert coded == 0, "random triangles have no hull face"
    if coded:
        assert st[7] > 0, "rays whose product on a hull face's flat axis is NaN (0 * inf)"
    # coverage, so that the pass means something
    assert int(st[10]) == (1 << leaves) - 1, f"{name}: leaf bits never set in a mask: {(1 << leaves) - 1 - int(st[10]):#x}"
    assert st[8] > 0 and st[9] > 0 and st[11] > 0, "rays passing the root box, rays failing it, candidates"


def test_standalone_program():
    """The harness's own main (the program meant for host sanitizer runs)
    builds and passes: a cuboid alone (six hull faces) and the same cuboid
    beside a tilted triangle under a larger root (none)."""
    lines = run_main("sweep_hull_check", "SWEEP_HULL_MAIN").strip().splitlines()
    assert len(lines) == 2
    assert "leaves=12 flat_boxes=6 hull_boxes=6 mask=0 none=0 plain=0 riding=0 hull=0 codes=0" in lines[0], lines
    assert "leaves=13 flat_boxes=6 hull_boxes=0 mask=0 none=0 plain=0 riding=0 hull=0 codes=0" in lines[1], lines
