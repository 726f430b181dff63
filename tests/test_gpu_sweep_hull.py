"""GPU: the hull faces of the sweep walk (PT_OPT_SWEEP_HULL: a flat box that is
a face of the root box is tested with the root's slab products, sweep_walk.h
sweep_slab_hull) against the same walk reading a table without codes and
against the threaded walk (PT_OPT_SMALL_SWEEP 0), bitwise.  The box and a
cuboid of three different extents off the origin have six hull faces each, the
latter also seen from inside (every ray starts inside the root box);
grid_mesh(2) and four random triangles run the uncoded path of the same
kernel.
"""
import numpy as np
import pytest

import ptamd
from support import lit_pixels, renderer, same, scene
from sweep_support import GPU_MAKERS, HULL_CASES as CASES, hull_check

pytestmark = pytest.mark.gpu

W, H, SPP = 256, 144, 2


def _frame(v, i, n, cam, lights, sweep, hull):
    r = renderer((v, i, n), cam, lights, options=[(ptamd.PT_OPT_SMALL_SWEEP, sweep), (ptamd.PT_OPT_SWEEP_HULL, hull)])
    boxes, leaves = r.sweep_info()
    assert (leaves == i.size // 3 and boxes >= 1) if sweep else (boxes, leaves) == (0, 0)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    out = r.read_accum()
    r.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_hull_on_off_and_threaded_walk_bitwise(name):
    mesh, cam, lights, hull_faces = CASES[name]
    v, i, n = scene(mesh, GPU_MAKERS)
    st, info = hull_check(v, i, n.reshape(-1), np.ones((1, 8), np.float32))
    assert (info[3] == 6) if hull_faces else (info[3] == 0), f"{name}: {info[3]} hull faces in the table"
    on = _frame(v, i, n, cam, lights, 1, 1)
    assert lit_pixels(on) >= 200, "the frame shows the scene lit"
    same(_frame(v, i, n, cam, lights, 1, 0), on, f"{name}: PT_OPT_SWEEP_HULL 0 against 1")
    same(_frame(v, i, n, cam, lights, 0, 1), on, f"{name}: the threaded walk against the sweep with hull faces")


def test_option_range():
    r = ptamd.Renderer(0)
    with pytest.raises(ptamd.PTError, match="PT_OPT_SWEEP_HULL"):
        r.set_option(ptamd.PT_OPT_SWEEP_HULL, 2)
    r.close()
