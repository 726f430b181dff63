"""GPU: the one-pass sweep walk (sweep_walk.h sweep_cands; each box's record
carries the leaves it guards) against the oracle, bitwise, with the sweep
forced on and off as in test_gpu_sweep.py.  One kernel runs every table, so
the cases span them: general and flat boxes in one table, the 63 boxes and
leaf bit 31 of 32 random triangles, quads at three depths under two lights.
"""
import numpy as np
import pytest

import ptamd
import scenes
from support import TWO_LIGHTS, lit_pixels, oracle_frame, renderer, same, scene
from sweep_support import visit_order

pytestmark = pytest.mark.gpu

# beside the box, in the default camera's view, its geometric normal towards the reference light
TILTED = np.float32([[1.2, -0.9, 0.5], [1.4, 0.8, 0.8], [2.6, -0.3, -0.4]])


def _box_and_tilted():
    v, i, _ = scene("box")
    nv = v.size // 3
    return (np.concatenate([v.reshape(-1), TILTED.reshape(-1)]).astype(np.float32),
            np.concatenate([i.reshape(-1), [nv, nv + 1, nv + 2]]).astype(np.uint32))


MAKERS = {"box+tilted": _box_and_tilted}


def _oracle(name, cam, lights, W, H, first, nb, depth, sss):
    return oracle_frame(scene(name, MAKERS), cam, lights, W, H, first, nb, depth, sss)


def _both(name, cam, lights, W, H, first, nb, depth, sss):
    """Sweep on (in force, by pt_sweep_info) and off: both frames equal the oracle's."""
    v, i, n = scene(name, MAKERS)
    ref = _oracle(name, cam, lights, W, H, first, nb, depth, sss)
    assert lit_pixels(ref) >= 20, "the frame shows the scene lit"
    for sweep in (1, 0):
        r = renderer((v, i, n), cam, lights, depth, sss, options=[(ptamd.PT_OPT_SMALL_SWEEP, sweep)])
        boxes, leaves = r.sweep_info()
        if sweep:
            assert leaves == i.size // 3 and 1 <= boxes <= 2 * leaves - 1
        else:
            assert (boxes, leaves) == (0, 0)
        r.resize_and_clear(W, H)
        r.render(first, nb)
        same(r.read_accum(), ref, f"{name} sweep={sweep}")
        r.close()
    return ref


def test_box_and_a_tilted_triangle():
    """13 triangles: the box's flat face boxes and the tilted triangle's
    general one (and the root's) in one table."""
    v, i, n = scene("box+tilted", MAKERS)
    assert i.size // 3 == 13
    nd = n.reshape(-1, 8)
    flat = (nd[:, 0:3] == nd[:, 4:7]).any(1)
    assert flat.sum() >= 6 and (~flat).sum() >= 2
    ref = _both("box+tilted", scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, 64, 48, 0, 2, 4, 3)
    box_only = _oracle("box", scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, 64, 48, 0, 2, 4, 3)
    assert np.count_nonzero(np.any(ref.reshape(-1, 4) != box_only.reshape(-1, 4), axis=1)) >= 20, \
        "the tilted triangle shows"


def _aimed_and_lit(name, tri):
    """A camera 3 away from triangle `tri` (the focal distance) on its
    geometric normal, looking at its centroid through a 1 degree field of
    view, and a light on the same side, off the line of sight, facing it: the
    shader shades with the geometric normal, so the triangle is lit."""
    v, i, _ = scene(name, MAKERS)
    p = v.reshape(-1, 3)[i.reshape(-1, 3)[tri]].astype(np.float64)
    c = p.mean(0)
    d = np.cross(p[1] - p[0], p[2] - p[0])
    d /= np.linalg.norm(d)
    side = np.zeros(3)
    side[int(np.argmin(np.abs(d)))] = 1.0
    side = np.cross(d, side)
    side /= np.linalg.norm(side)
    cam = np.zeros(16, np.float32)
    cam[0:3] = c + 3.0 * d
    cam[4:7] = -d
    cam[8 + int(np.argmin(np.abs(d)))] = 1.0   # an up vector well off the view direction
    cam[12] = 1.0
    lpos = c + 2.0 * d + 1.0 * side
    ldir = (c - lpos) / np.linalg.norm(c - lpos)
    return cam, ptamd.pack_light(lpos, ldir, [10, 10, 10], [0.5, 0.5])


@pytest.mark.parametrize("leaf", [0, 31])
def test_32_triangles_first_and_last_leaf(leaf):
    """63 boxes, 32 leaves: the frame looks at the triangle of leaf 0 and at
    the one of leaf 31 (bit 31 of the masks), by the table's visit order."""
    v, i, n = scene("tri:32", MAKERS)
    slots = visit_order(v, i, n.reshape(-1))
    assert len(slots) == 32 and sorted(slots) == list(range(32))
    cam, light = _aimed_and_lit("tri:32", int(slots[leaf]))
    _both("tri:32", cam, light, 96, 64, 0, 2, 4, 3)


def test_grid_flat_leaf_boxes_two_lights():
    """grid_mesh(2): eight triangles in quads at constant z, so every leaf's box is flat."""
    _, i, n = scene("grid:2", MAKERS)
    nd = n.reshape(-1, 8)
    assert (nd[:, 2] == nd[:, 6]).sum() >= i.size // 3
    _both("grid:2", scenes.camera((0.0, 0.0, 3.0)), TWO_LIGHTS, 48, 48, 0, 2, 3, 2)
