"""The tight cull rectangles (PT_OPT_CULL_TIGHT, csrc/pt_cull.h)
on the CPU.

render_kernel skips a sample of a pixel that lies inside a loose rectangle
(pt_primary_cull_rects: any Box-Muller radius) but outside every tight one
(pt_primary_cull_rects_r: radii of at most 4.25) when both of the sample's
radius draws u1 are at least kCullTightU0.  Two things make that exact:

* the radius guarantee: every float u in [kCullTightU0, 1] has the kernel's
  sqrt_(-2.0f * log_(fmax_(1e-38f, u))) at most 4.25.  tests/cull_radius_check.cpp
  evaluates all 1.1e8 of them with pt_math.h's host functions;
* the rectangles: a pixel outside the tight ones has no primary ray with radii
  of at most 4.25 that reaches the root box or a light -- probed with radii at
  the bound over a scan of both angles, and with the oracle's own samples
  (real seeds whose two draws pass the kernel's test), which must come out
  exactly (0,0,0).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import native
import oracle_lib
import ptamd
import scenes
from cull_support import CASE_IDS, CASES, culled_mask, light_hit, margin_mask, rays, rng_draws, skip_counts, slab_hit
from support import box_mesh, oracle_built

R_TIGHT = 4.25
U0_BITS = 0x38FAD897   # kCullTightU0 = 0x1.f5b12ep-14f


def _harness():
    return native.build("cull_radius_check", [os.path.join(native.TESTS, "cull_radius_check.cpp")],
                        ["-O2"] + native.COMMON + ["-I", native.CSRC], libs=["-lpthread"])


def test_radius_guarantee_over_every_float():
    """Every float in [kCullTightU0, 1] has its radius within the bound, the
    float below kCullTightU0 has not, and the library reports that constant."""
    out = subprocess.run([_harness()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    assert float(f["bound"]) == R_TIGHT and int(f["bits"], 16) == U0_BITS
    assert int(f["floats"]) == 0x3F800000 - U0_BITS + 1
    assert float(f["max_radius"]) <= R_TIGHT and f["above_bound"] == "0" and f["holds"] == "1"
    assert float(f["radius_below_u0"]) > R_TIGHT and f["least"] == "1"
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    _, u0 = ptamd.primary_cull_rects_r(scenes.DEFAULT_CAMERA, 64, 64, lo, hi, scenes.REFERENCE_LIGHT)
    assert np.float32(u0).view(np.uint32) == U0_BITS
    # the oracle's own log and sqrt agree at the threshold and next to it
    u = np.array([U0_BITS - 1, U0_BITS, U0_BITS + 1], np.uint32).view(np.float32)
    r = np.sqrt(np.float32(-2.0) * oracle_lib.math(0, u))
    assert r[0] > R_TIGHT and r[1] <= R_TIGHT and r[2] <= R_TIGHT


def _sets(cam, W, H, lights):
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)   # box.obj root
    loose = ptamd.primary_cull_rects(cam, W, H, lo, hi, lights)
    tight, u0 = ptamd.primary_cull_rects_r(cam, W, H, lo, hi, lights)
    zero, _ = ptamd.primary_cull_rects_r(cam, W, H, lo, hi, lights, 0.0)
    assert loose is not None and tight is not None and zero is not None
    return loose, tight, zero, np.float32(u0)


@pytest.mark.parametrize("name,cam,W,H,lights", CASES, ids=CASE_IDS)
def test_tight_rectangles_nest(name, cam, W, H, lights):
    """Per object: the R = 0 rectangle inside the tight one inside the loose
    one; the default bound of the new entry point is the loose derivation's."""
    loose, tight, zero, _ = _sets(cam, W, H, lights)
    assert loose.shape == tight.shape == zero.shape
    for l, t, z in zip(loose, tight, zero):
        assert l[0] <= t[0] <= z[0] and z[1] <= t[1] <= l[1], (name, l, t, z)
        assert l[2] <= t[2] <= z[2] and z[3] <= t[3] <= l[3], (name, l, t, z)
        assert t[0] > l[0] and t[1] < l[1] and t[2] > l[2] and t[3] < l[3], "the tight rectangle is smaller"
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    same, _ = ptamd.primary_cull_rects_r(cam, W, H, lo, hi, lights, 13.25)
    assert np.array_equal(same, loose)
    with pytest.raises(ptamd.PTError):
        ptamd.primary_cull_rects_r(cam, W, H, lo, hi, lights, 13.5)


def test_rng_restatement_equals_the_oracle():
    rnd = np.random.default_rng(5)
    seeds = np.concatenate([np.arange(0, 64), 2 ** 32 - 1 - np.arange(0, 64), 2 ** 31 + np.arange(-32, 32),
                            rnd.integers(0, 2 ** 32, 4000)]).astype(np.uint64)
    got = rng_draws(seeds, 4)
    want = np.stack([oracle_lib.rng(int(s), 4) for s in seeds])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(got)) > 0.99 * got.size


def test_skip_counts_of_the_gpu_test_frame():
    """The box at 320x180, default camera: 5,369 margin pixels; batches 0-7
    hold 12 margin samples with a radius draw below u0 (the kernel must trace
    them), batches 0-599 hold 767."""
    live, skipped, traced = skip_counts(scenes.DEFAULT_CAMERA, 320, 180, scenes.REFERENCE_LIGHT, 0, 8)
    assert skipped + traced == 5369 * 8 and traced == 12 and live > 5369
    _, skipped, traced = skip_counts(scenes.DEFAULT_CAMERA, 320, 180, scenes.REFERENCE_LIGHT, 0, 600)
    assert skipped + traced == 5369 * 600 and traced == 767


@pytest.mark.parametrize("name,cam,W,H,lights", CASES, ids=CASE_IDS)
def test_margin_pixels_reach_nothing_with_radii_at_the_bound(name, cam, W, H, lights):
    """Aperture and jitter radii both at the bound, both angles scanned (the
    worst angle of each lies within half a step of a scanned one; the margin
    the rectangles keep, a pixel and more, is far above what half a step of
    1/32 turn moves a ray), plus random radii below the bound."""
    loose, tight, _, _ = _sets(cam, W, H, lights)
    margin = margin_mask(loose, tight, W, H)
    assert margin.any(), "pixels between the two sets"
    lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    L = np.asarray(lights, np.float32).reshape(-1, 16)
    ang = np.arange(32) * (2 * np.pi / 32)
    rnd = np.random.default_rng(11)
    ys, xs = np.nonzero(margin)
    pick = rnd.choice(len(xs), size=min(len(xs), 24), replace=False)
    for k in pick:
        px, py = int(xs[k]), int(ys[k])
        probes = [(R_TIGHT, a, R_TIGHT, b) for a in ang for b in ang[::2]]
        probes += [(rnd.uniform(0, R_TIGHT), rnd.uniform(0, 2 * np.pi), rnd.uniform(0, R_TIGHT), rnd.uniform(0, 2 * np.pi))
                   for _ in range(32)]
        for ra, ta, rj, tj in probes:
            o, d = rays(cam, W, H, px, py, 0.02 * ra * np.cos(ta), 0.02 * ra * np.sin(ta), rj * np.cos(tj),
                                   rj * np.sin(tj))
            assert not slab_hit(o, d, lo, hi), (name, px, py, ra, ta, rj, tj)
            for li in L:
                assert not light_hit(o, d, li), (name, px, py, ra, ta, rj, tj)


@pytest.fixture(scope="module")
def box():
    return oracle_built(*box_mesh())


@pytest.mark.parametrize("name,cam,W,H,lights", CASES, ids=CASE_IDS)
def test_oracle_samples_the_kernel_skips_are_black(box, name, cam, W, H, lights):
    """The samples render_kernel skips -- margin pixels, real seeds whose two
    radius draws are at least kCullTightU0 -- rendered one batch at a time by
    the oracle: each is exactly (0,0,0).  Seeds the kernel does not skip (a
    draw below the threshold) are counted, so that the test says whether it
    met one."""
    v, idx, nodes = box
    lo, hi = nodes.reshape(-1, 8)[0, 0:3], nodes.reshape(-1, 8)[0, 4:7]
    loose = ptamd.primary_cull_rects(cam, W, H, lo, hi, lights)
    tight, u0 = ptamd.primary_cull_rects_r(cam, W, H, lo, hi, lights)
    u0 = np.float32(u0)
    margin = margin_mask(loose, tight, W, H)
    ys, xs = np.nonzero(margin)
    assert len(xs) > 0
    skipped = 0
    for batch in range(6):
        pixels = []
        for px, py in zip(xs, ys):
            seed = ((batch * H + int(py)) * W + int(px)) & 0xFFFFFFFF
            u = np.maximum(np.float32(1e-38), oracle_lib.rng(seed, 4))
            if u[0] >= u0 and u[2] >= u0:   # u1 of the aperture, u1 of the jitter
                pixels.append(int(py) * W + int(px))
        skipped += len(pixels)
        img, _ = oracle_lib.render_pixels(v, idx, nodes, cam, lights, W, H, pixels, first_batch=batch, n_batches=1,
                                          max_depth=4, sss_bounces=3)
        rgb = img.reshape(-1, 4)[pixels, :3]
        assert not rgb.any(), (name, batch, np.array(pixels)[rgb.any(1)][:5])
    assert skipped >= 0.99 * 6 * len(xs), "nearly every sample of a margin pixel is skipped"


@pytest.mark.parametrize("W,H,n_live,n_margin", [(320, 180, 326, 98), (1920, 1080, 9954, 2562)])
def test_blocks_in_the_margin(W, H, n_live, n_margin):
    """The box at the default camera: live 16x4 blocks (the wave footprint at
    one lane per pixel) and those wholly outside the tight rectangles, whose
    waves skip whole samples -- at the GPU test's size and at the benchmark's."""
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    loose = ptamd.primary_cull_rects(scenes.DEFAULT_CAMERA, W, H, lo, hi, scenes.REFERENCE_LIGHT)
    tight, _ = ptamd.primary_cull_rects_r(scenes.DEFAULT_CAMERA, W, H, lo, hi, scenes.REFERENCE_LIGHT)
    live = ~culled_mask(loose, W, H)
    inner = ~culled_mask(tight, W, H)
    by = -(-H // 4)
    pad = np.zeros((by * 4, W), bool)
    blocks = lambda m: np.where(np.arange(by * 4)[:, None] < H, np.vstack([m, pad[H:]]), False).reshape(by, 4, W // 16, 16)
    lb, ib = blocks(live).any((1, 3)), blocks(inner).any((1, 3))
    assert (int(lb.sum()), int((lb & ~ib).sum())) == (n_live, n_margin)
