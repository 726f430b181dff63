"""The sweep walk of tiny scenes (csrc/sweep_walk.h, scene/small_sweep.h)
against the threaded walk it replaces, on the CPU.

tests/sweep_check.cpp compiles the sweep's own functions for the host, builds
the threaded and collapsed node arrays and the sweep table from oracle-built
nodes, and walks every ray both ways: the sequence of leaves whose triangles
are tested, the closest hit (t bits, triangle) and the shadow answer must be
equal.  The rays include origins inside the root box, directions with a zero
component (inv is infinite and the slab test sees NaNs) and rays lying in a
face plane.
"""
import pytest

from sweep_support import HOSTILE, HOSTILE_TABLES, check, info, make_rays, scene

SCENES = ["box", "grid:2", "grid:3", "grid:4", "tri:1", "tri:2", "tri:3", "tri:7", "tri:16", "tri:32"] + sorted(HOSTILE)


@pytest.mark.parametrize("name", SCENES)
def test_sweep_equals_threaded_walk(name):
    v, idx, nodes = scene(name)
    has, inf = info(v, idx, nodes)
    rays = make_rays(v, idx, 6000, seed=len(name) * 131 + idx.size)
    ok, st = check(v, idx, nodes, rays)
    assert ok and has
    # up to 32 distinct boxes the box mask is 32 bits wide, else 64 (tri:32 has 63)
    assert inf[1] == idx.size // 3 and 1 <= inf[0] <= min(64, inf[3])
    assert inf[2] == 0, "every need mask holds the root's bit"
    if name in HOSTILE_TABLES:
        assert (int(inf[0]), int(inf[1])) == HOSTILE_TABLES[name]
    assert (int(st[0]), int(st[1]), int(st[2])) == (0, 0, 0), \
        f"{name}: leaf sequence / closest / shadow mismatches {st[:3]}, first bad ray {int(st[3])}: {rays[int(st[3]) % len(rays)]}"
    # the rays do reach the geometry
    assert st[4] > 0 and st[5] > 0 and st[6] > 0


def test_box_has_at_most_nine_boxes():
    v, idx, nodes = scene("box")
    has, inf = info(v, idx, nodes)
    assert has
    assert inf[0] <= 9 and inf[1] == 12
    assert inf[2] == 0


def test_no_table_past_32_leaves():
    v, idx, nodes = scene("tri:33")
    has, inf = info(v, idx, nodes)
    assert not has and inf[0] == 0 and inf[1] == 0
    ok, _ = check(v, idx, nodes, make_rays(v, idx, 60, seed=1))
    assert not ok
