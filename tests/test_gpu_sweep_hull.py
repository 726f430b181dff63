"""GPU: the hull faces of the sweep walk (PT_OPT_SWEEP_HULL: a flat box that is
a face of the root box is tested with the root's slab products, sweep_walk.h
sweep_slab_hull) against the same walk reading a table without codes and
against the threaded walk (PT_OPT_SMALL_SWEEP 0), bitwise.  The box and a
cuboid of three different extents off the origin have six hull faces each, the
latter also seen from inside (every ray starts inside the root box);
grid_mesh(2) and four random triangles run the uncoded path of the same
kernel.
"""
import functools

import numpy as np
import pytest

import ptamd
import scenes
import test_sweep_hull
from test_gpu_sweep import TWO_LIGHTS, _same

pytestmark = pytest.mark.gpu

W, H, SPP = 256, 144, 2
CENTRE = (test_sweep_hull.CUBOID_LO.astype(np.float64) + test_sweep_hull.CUBOID_HI) * 0.5


def _ubo(pos, at, fov=60.0, up=(0, 1, 0)):
    d = np.asarray(at, np.float64) - np.asarray(pos, np.float64)
    ubo = np.zeros(16, np.float32)
    ubo[0:3] = pos
    ubo[4:7] = d / np.linalg.norm(d)
    ubo[8:11] = up
    ubo[12] = fov
    return ubo


def _light(pos, at, size):
    d = np.asarray(at, np.float64) - np.asarray(pos, np.float64)
    return ptamd.pack_light(pos, d / np.linalg.norm(d), [10, 10, 10], size)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "box":
        s = ptamd.Scene.load_obj(scenes.BOX_OBJ)
    elif name.startswith("cuboid"):
        s = ptamd.Scene.from_arrays(*test_sweep_hull.cuboid(outward=name == "cuboid"))
    else:
        kind, n = name.split(":")
        s = ptamd.Scene.from_arrays(*(scenes.grid_mesh(int(n)) if kind == "grid" else scenes.random_triangles(int(n))))
    v, i, n, _, _ = s.build_bvh().arrays()
    return v, i, n


# name -> (scene, camera, lights, hull faces expected)
CASES = {
    "box": ("box", scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, True),
    "cuboid": ("cuboid", _ubo(CENTRE + [1.5, 1.25, 3.5], CENTRE, 40.0),
               np.concatenate([_light(CENTRE + [0.5, 2.0, 1.0], CENTRE, [2.0, 2.0]),
                               _light(CENTRE + [2.5, 0.25, 2.0], CENTRE, [1.0, 1.0])]), True),
    "cuboid-inside": ("cuboid-inward", _ubo(CENTRE + [0.0, 0.0, 0.5], CENTRE + [0.25, 0.125, -1.0], 90.0),
                      _light(CENTRE + [0.0, 0.2, 0.0], CENTRE + [0.0, -1.0, 0.0], [0.2, 0.2]), True),
    "grid:2": ("grid:2", scenes.camera((0.0, 0.0, 3.0)), TWO_LIGHTS, False),
    "tri:4": ("tri:4", scenes.camera((0.0, 0.0, 3.0), fov=50.0), TWO_LIGHTS, False),
}


def _frame(v, i, n, cam, lights, sweep, hull):
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_SMALL_SWEEP, sweep)
    r.set_option(ptamd.PT_OPT_SWEEP_HULL, hull)
    r.upload_scene(v, i, n)
    r.upload_lights(lights)
    r.set_camera(cam)
    r.set_params(4, 3)
    boxes, leaves = r.sweep_info()
    assert (leaves == i.size // 3 and boxes >= 1) if sweep else (boxes, leaves) == (0, 0)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    out = r.read_accum()
    r.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_hull_on_off_and_threaded_walk_bitwise(name):
    scene, cam, lights, hull_faces = CASES[name]
    v, i, n = _scene(scene)
    st, info = test_sweep_hull.hull_check(v, i, n.reshape(-1), np.ones((1, 8), np.float32))
    assert (info[3] == 6) if hull_faces else (info[3] == 0), f"{name}: {info[3]} hull faces in the table"
    on = _frame(v, i, n, cam, lights, 1, 1)
    assert np.count_nonzero(np.any(on.reshape(-1, 4)[:, :3] != 0, axis=1)) >= 200, "the frame shows the scene lit"
    _same(_frame(v, i, n, cam, lights, 1, 0), on, f"{name}: PT_OPT_SWEEP_HULL 0 against 1")
    _same(_frame(v, i, n, cam, lights, 0, 1), on, f"{name}: the threaded walk against the sweep with hull faces")


def test_option_range():
    r = ptamd.Renderer(0)
    with pytest.raises(ptamd.PTError, match="PT_OPT_SWEEP_HULL"):
        r.set_option(ptamd.PT_OPT_SWEEP_HULL, 2)
    r.close()
