"""GPU: the sweep walk of tiny scenes (PT_OPT_SMALL_SWEEP) against the oracle.

Every comparison is bitwise: each frame with the sweep on and with it off
equals the oracle's, hence each other.  pt_sweep_info tells which walk a
launch takes, so a case cannot pass by silently running the threaded walk.
"""
import numpy as np
import pytest

import oracle_lib as O
import ptamd
import scenes
from support import TWO_LIGHTS, lit_pixels, renderer, same, scene

pytestmark = pytest.mark.gpu


def _renderer(name, cam, lights, depth, sss, sweep):
    return renderer(scene(name), cam, lights, depth, sss, options=[(ptamd.PT_OPT_SMALL_SWEEP, sweep)])


def _both(name, cam, lights, W, H, first, nb, depth, sss, in_force=True, lanes=None):
    """Renders with the sweep on and off, checks pt_sweep_info and both frames
    against the oracle."""
    v, i, n = scene(name)
    ref, _ = O.render(v, i, n.reshape(-1), cam, lights, W, H, first_batch=first, n_batches=nb, max_depth=depth,
                      sss_bounces=sss)
    assert lit_pixels(ref) >= 20, "the frame shows the scene lit"
    for sweep in (1, 0):
        r = _renderer(name, cam, lights, depth, sss, sweep)
        if lanes:
            r.set_option(ptamd.PT_OPT_SAMPLE_LANES, lanes)
        boxes, leaves = r.sweep_info()
        if sweep and in_force:
            assert leaves == i.size // 3 and 1 <= boxes <= 2 * leaves - 1
        else:
            assert (boxes, leaves) == (0, 0)
        r.resize_and_clear(W, H)
        r.render(first, nb)
        same(r.read_accum(), ref, f"{name} sweep={sweep} lanes={lanes}")
        r.close()


@pytest.mark.parametrize("cam", [scenes.DEFAULT_CAMERA, scenes.camera((0, 0, 0.5)), scenes.camera((1.0, 0.0, 5.0))],
                         ids=["default", "inside", "face_plane"])
def test_box(cam):
    _both("box", cam, scenes.REFERENCE_LIGHT, 64, 48, 2, 3, 4, 3)


@pytest.mark.parametrize("n", [2, 4])
def test_grid_two_lights(n):
    _both(f"grid:{n}", scenes.camera((0.0, 0.0, 3.0)), TWO_LIGHTS, 48, 48, 0, 2, 3, 2)


def _facing_light(name):
    v, i, _ = scene(name)
    p = v.reshape(-1, 3)[i.reshape(-1, 3)].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    to_light = scenes.REFERENCE_LIGHT[0:3] - p.mean(1)
    cos = (nrm * to_light).sum(1) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(to_light, axis=1))
    return [int(t) for t in np.flatnonzero(cos > 0.2)]


def _aimed(name, tri):
    """A camera 3 away from triangle `tri` (the focal distance, so the
    aperture does not blur it) on its normal, on the side that faces the
    light, looking at its centroid through a 1 degree field of view: the
    generator's triangles are 0.02 across and fill a good part of such a
    frame."""
    v, i, _ = scene(name)
    p = v.reshape(-1, 3)[i.reshape(-1, 3)[tri]].astype(np.float64)
    c = p.mean(0)
    d = np.cross(p[1] - p[0], p[2] - p[0])
    d /= np.linalg.norm(d)
    if np.dot(d, scenes.REFERENCE_LIGHT[0:3] - c) < 0:
        d = -d
    ubo = np.zeros(16, np.float32)
    ubo[0:3] = c + 3.0 * d
    ubo[4:7] = -d
    ubo[8 + int(np.argmin(np.abs(d)))] = 1.0   # an up vector well off the view direction
    ubo[12] = 1.0
    return ubo


@pytest.mark.parametrize("n", [1, 3, 32, 33])
def test_random_triangles(n):
    """33 triangles get no table: the threaded walk, still exact.  Each frame
    looks at one triangle and must show it lit: the first, the middle and the
    last of the slots whose geometric normal faces the light (the shader
    shades with that normal whichever side is seen, so the others are black).
    n = 32 has 63 distinct boxes and runs the 64-bit box mask."""
    lit = _facing_light(f"tri:{n}")
    for tri in sorted({lit[0], lit[len(lit) // 2], lit[-1]}):
        _both(f"tri:{n}", _aimed(f"tri:{n}", tri), scenes.REFERENCE_LIGHT, 96, 64, 0, 2, 4, 3, in_force=n <= 32)


@pytest.mark.parametrize("lanes", [1, 4])
def test_sample_lanes(lanes):
    """The lanes-per-pixel mapping is independent of the walk."""
    _both("box", scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, 17, 13, 0, 5, 4, 3, lanes=lanes)


@pytest.mark.parametrize("name,boxes", [("box", 7), ("tri:8", 15), ("grid:3", 0), ("tri:16", 0), ("grid:4", 0),
                                        ("tri:33", 0)])
def test_default_takes_the_sweep_up_to_its_measured_bound(name, boxes):
    """PT_OPT_SMALL_SWEEP -1 (the default): the sweep for scenes of at most 15
    distinct boxes; 21 (grid_mesh(3), where the two walks measured within each
    other's scatter) and 31 (16 random triangles, grid_mesh(4), where the
    threaded walk measured faster) keep it (profiles/sweep/sweep_sizes.log)."""
    v, i, n = scene(name)
    r = ptamd.Renderer(0)
    r.upload_scene(v, i, n)
    assert r.sweep_info() == (boxes, i.size // 3 if boxes else 0)
    r.set_option(ptamd.PT_OPT_SCENE_IN_LDS, 0)   # walks from device memory never sweep
    assert r.sweep_info() == (0, 0)
    with pytest.raises(ptamd.PTError, match="PT_OPT_SMALL_SWEEP"):
        r.set_option(ptamd.PT_OPT_SMALL_SWEEP, 2)
    r.close()


def test_count_traced_keeps_the_threaded_walk():
    """The counting kernels run the threaded walk whatever the sweep option:
    same image bit for bit, same counts."""
    v, i, n = scene("box")
    ref, _ = O.render(v, i, n.reshape(-1), scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, 64, 48, first_batch=2,
                      n_batches=3)
    counts = []
    for sweep in (1, 0):
        r = _renderer("box", scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, 4, 3, sweep)
        r.set_option(ptamd.PT_OPT_COUNT_TRACED, 1)
        r.resize_and_clear(64, 48)
        r.reset_stats()
        r.render(2, 3)
        same(r.read_accum(), ref, f"count_traced sweep={sweep}")
        counts.append(r.traced())
        r.close()
    assert counts[0] == counts[1]
    assert counts[0]["closest_walks"] > 0 and counts[0]["nodes"] > 0 and counts[0]["tri_tests"] > 0
