"""Primary-ray culling (pt_primary_cull_rects): a pixel outside
every rectangle must have no primary ray that reaches the root box or a light.

CPU tests: the Box-Muller radius bound the rectangles rest on, extreme-ray
probes of culled pixels (aperture and jitter at their bounds), and oracle
renders whose culled pixels must come out exactly (0,0,0,1).
"""
import itertools

import numpy as np
import pytest

import oracle_lib
import ptamd
import scenes
from cull_support import CASE_IDS, CASES, culled_mask, light_hit, rays, ring_lights, slab_hit
from support import box_mesh, oracle_built

RG = 13.25   # Box-Muller radius bound used by the host code


@pytest.fixture(scope="module")
def box():
    return oracle_built(*box_mesh())


def test_gauss_radius_bound():
    # u1 = max(1e-38, u) (raytrace_comp.comp:220): the largest radius is at 1e-38
    lg = oracle_lib.math(0, np.array([1e-38, 2.0 ** -32, 0.5], np.float32))
    r = np.sqrt(np.float32(-2.0) * lg)
    assert r[0] < RG and r[0] > 13.2
    assert np.all(r[1:] < r[0])
    # |sin|, |cos| never exceed 1 on the shader's argument range [0, 2pi]
    th = np.linspace(0, 2 * np.pi, 200001, dtype=np.float32)
    assert np.all(np.abs(oracle_lib.math(2, th)) <= 1.0)
    assert np.all(np.abs(oracle_lib.math(3, th)) <= 1.0)


@pytest.mark.parametrize("name,cam,W,H,lights", CASES, ids=CASE_IDS)
def test_culled_pixels_have_no_reaching_primary_ray(name, cam, W, H, lights):
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)   # box.obj root
    rects = ptamd.primary_cull_rects(cam, W, H, lo, hi, lights)
    assert rects is not None
    culled = culled_mask(rects, W, H)
    assert culled.any() and not culled.all()
    rho, J = 0.02 * RG, RG
    probes = list(itertools.product((-rho, 0.0, rho), (-rho, 0.0, rho), (-J, 0.0, J), (-J, 0.0, J)))
    rnd = np.random.default_rng(7)
    L = np.asarray(lights, np.float32).reshape(-1, 16)
    ys, xs = np.nonzero(culled)
    pick = rnd.choice(len(xs), size=min(len(xs), 150), replace=False)
    for k in pick:
        px, py = int(xs[k]), int(ys[k])
        extra = [(rnd.uniform(-rho, rho), rnd.uniform(-rho, rho), rnd.uniform(-J, J), rnd.uniform(-J, J)) for _ in range(20)]
        for ox, oy, jx, jy in probes + extra:
            o, d = rays(cam, W, H, px, py, ox, oy, jx, jy)
            assert not slab_hit(o, d, lo.astype(np.float64), hi.astype(np.float64)), (name, px, py, ox, oy, jx, jy)
            for li in L:
                assert not light_hit(o, d, li), (name, px, py, ox, oy, jx, jy)


def test_cull_rects_are_tight_enough_to_matter():
    # box.obj at 1080p: the box and the light cover well under half the frame
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    rects = ptamd.primary_cull_rects(scenes.DEFAULT_CAMERA, 1920, 1080, lo, hi, scenes.REFERENCE_LIGHT)
    frac = culled_mask(rects, 1920, 1080).mean()
    assert frac > 0.5, frac


def test_cull_disabled_when_object_reaches_camera_plane():
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    inside = scenes.camera((0.0, 0.0, 0.5))
    assert ptamd.primary_cull_rects(inside, 64, 64, lo, hi, scenes.REFERENCE_LIGHT) is None
    behind = np.array([0, 0, 5, 0, 0, 0, 1, 0, 0, 1, 0, 0, 60, 0, 0, 0], np.float32)   # looking away
    assert ptamd.primary_cull_rects(behind, 64, 64, lo, hi, scenes.REFERENCE_LIGHT) is None
    degenerate = np.array([0, 0, 5, 0, 0, 1, 0, 0, 0, 1, 0, 0, 60, 0, 0, 0], np.float32)   # dir parallel to up
    assert ptamd.primary_cull_rects(degenerate, 64, 64, lo, hi, scenes.REFERENCE_LIGHT) is None
    many = np.tile(scenes.REFERENCE_LIGHT, 8)
    assert ptamd.primary_cull_rects(scenes.DEFAULT_CAMERA, 64, 64, lo, hi, many) is None


def test_seven_lights_fill_the_rectangle_table_and_eight_switch_culling_off():
    """The table holds 8 rectangles (kMaxCullRects): the root box and 7 lights."""
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    rects = ptamd.primary_cull_rects(scenes.DEFAULT_CAMERA, 64, 48, lo, hi, ring_lights(7))
    assert rects is not None and len(rects) == 8
    assert culled_mask(rects, 64, 48).any()
    for n in (8, 9):
        assert ptamd.primary_cull_rects(scenes.DEFAULT_CAMERA, 64, 48, lo, hi, ring_lights(n)) is None


@pytest.mark.parametrize("name,cam,W,H,lights", CASES[:4], ids=CASE_IDS[:4])
def test_oracle_renders_culled_pixels_as_background(box, name, cam, W, H, lights):
    v, idx, nodes = box
    lo = nodes.reshape(-1, 8)[0, 0:3]
    hi = nodes.reshape(-1, 8)[0, 4:7]
    rects = ptamd.primary_cull_rects(cam, W, H, lo, hi, lights)
    culled = culled_mask(rects, W, H)
    img, _ = oracle_lib.render(v, idx, nodes, cam, lights, W, H, 0, 4, max_depth=1, sss_bounces=0)
    img = img.reshape(H, W, 4)
    assert np.array_equal(img[culled].view(np.uint32),
                          np.tile(np.array([0, 0, 0, 1], np.float32), (int(culled.sum()), 1)).view(np.uint32))
