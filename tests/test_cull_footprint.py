"""The cull footprints (PT_OPT_CULL_FOOTPRINT, csrc/pt_cull.h) on
the CPU.

With the option on, render_kernel's per-sample skip (PT_OPT_CULL_TIGHT) decides
by footprints instead of the tight rectangles: a pixel outside every footprint
traces a sample only if one of its two radius draws is below kCullTightU0.  A
footprint lies inside its object's tight rectangle, so the pixels that change
sides are those inside a tight rectangle and outside every footprint.  That
they reach nothing with radii of at most 4.25 is probed here as
test_cull_tight.py probes the rectangles' margin -- radii at the bound over a
scan of both angles -- and with the oracle's own samples, which must come out
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
from cull_foot_support import FOOT_CASES, FOOT_IDS, HI, LO, blocks, foot_mask, sure_masks
from cull_support import culled_mask, light_hit, rays, slab_hit
from support import box_mesh, oracle_built

R_TIGHT = 4.25


def _sets(cam, W, H, lights):
    loose = ptamd.primary_cull_rects(cam, W, H, LO, HI, lights)
    tight, u0 = ptamd.primary_cull_rects_r(cam, W, H, LO, HI, lights)
    foot = ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights)
    assert loose is not None and tight is not None and foot is not None
    assert len(loose) == len(tight) == len(foot)
    return loose, tight, foot, np.float32(u0)


def test_option_and_entry_points_are_declared():
    assert ptamd.PT_OPT_CULL_FOOTPRINT == 33
    with open(os.path.join(native.INCLUDE, "pathtracer.h")) as f:
        text = f.read()
    assert re.search(r"^#define PT_OPT_CULL_FOOTPRINT 33$", text, re.M)
    for name in ("pt_primary_cull_footprints", "pt_primary_cull_sure", "pt_cull_info"):
        assert name in ptamd.EXPORTS and re.search(r"\b%s\(" % name, text)


@pytest.mark.parametrize("name,cam,W,H,lights", FOOT_CASES, ids=FOOT_IDS)
def test_footprints_nest(name, cam, W, H, lights):
    """Per object: footprint(0) inside footprint(4.25) inside the public tight
    rectangle, footprint(13.25) inside the public loose rectangle -- as
    rectangles and as pixel sets."""
    loose, tight, foot, _ = _sets(cam, W, H, lights)
    zero = ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights, 0.0)
    wide = ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights, 13.25)
    assert zero.shape == foot.shape == wide.shape == (len(tight), 16)
    assert np.isfinite(foot).all() and np.isfinite(zero).all() and np.isfinite(wide).all()
    for r in range(len(tight)):
        for inner, outer in ((zero[r], foot[r]), (foot[r], tight[r]), (wide[r], loose[r]), (foot[r], wide[r])):
            assert outer[0] <= inner[0] <= inner[1] <= outer[1], (name, r, inner, outer)
            assert outer[2] <= inner[2] <= inner[3] <= outer[3], (name, r, inner, outer)
        z, f, w = foot_mask(zero[r], W, H), foot_mask(foot[r], W, H), foot_mask(wide[r], W, H)
        assert not (z & ~f).any() and not (f & ~w).any(), (name, r)
        assert not (f & culled_mask(tight[r:r + 1], W, H)).any(), (name, r)
        assert not (w & culled_mask(loose[r:r + 1], W, H)).any(), (name, r)
    assert foot_mask(foot, W, H).sum() < (~culled_mask(tight, W, H)).sum(), "the footprints are smaller"
    with pytest.raises(ptamd.PTError):
        ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights, 13.5)


def test_no_rectangles_no_footprints():
    """A camera for which the rectangles give no guarantee gives none here."""
    for cam, lights in ((scenes.camera((0.0, 0.0, 0.5)), scenes.REFERENCE_LIGHT),
                        (scenes.DEFAULT_CAMERA, np.tile(scenes.REFERENCE_LIGHT, 8))):
        assert ptamd.primary_cull_rects_r(cam, 64, 48, LO, HI, lights)[0] is None
        assert ptamd.primary_cull_footprints(cam, 64, 48, LO, HI, lights) is None


def _probe_pixels(mask, inside, rnd, n):
    """Up to n pixels of the mask: those that touch the footprints first (the
    nearest to what a ray could reach), then random ones."""
    near = np.zeros_like(inside)
    near[1:] |= inside[:-1]; near[:-1] |= inside[1:]; near[:, 1:] |= inside[:, :-1]; near[:, :-1] |= inside[:, 1:]
    ys, xs = np.nonzero(mask & near)
    first = rnd.permutation(len(xs))[:n // 2]
    picks = [(int(xs[k]), int(ys[k])) for k in first]
    ys, xs = np.nonzero(mask)
    picks += [(int(xs[k]), int(ys[k])) for k in rnd.permutation(len(xs))[:n - len(picks)]]
    return picks


@pytest.mark.parametrize("name,cam,W,H,lights", FOOT_CASES, ids=FOOT_IDS)
def test_pixels_outside_the_footprints_reach_nothing_with_radii_at_the_bound(name, cam, W, H, lights):
    """Pixels inside a tight rectangle but outside every footprint: aperture
    and jitter radii both at the bound over the angle scans of
    test_cull_tight.py, plus random radii below the bound.  No probe hits the
    root box's slab and none hits a light."""
    _, tight, foot, _ = _sets(cam, W, H, lights)
    inside = foot_mask(foot, W, H)
    mask = ~culled_mask(tight, W, H) & ~inside
    if name != "tiny":
        assert mask.any(), "pixels between the two sets"
    L = np.asarray(lights, np.float32).reshape(-1, 16)
    lo, hi = LO.astype(np.float64), HI.astype(np.float64)
    ang = np.arange(32) * (2 * np.pi / 32)
    rnd = np.random.default_rng(17)
    for px, py in _probe_pixels(mask, inside, rnd, 24):
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


@pytest.mark.parametrize("name,cam,W,H,lights", FOOT_CASES, ids=FOOT_IDS)
def test_oracle_samples_outside_the_footprints_are_black(box, name, cam, W, H, lights):
    """The samples the footprints let the kernel skip beyond those of the
    rectangles -- pixels inside a tight rectangle and outside every footprint,
    real seeds whose two radius draws are at least kCullTightU0 -- rendered one
    batch at a time by the oracle: each is exactly (0,0,0)."""
    v, idx, nodes = box
    lo, hi = nodes.reshape(-1, 8)[0, 0:3], nodes.reshape(-1, 8)[0, 4:7]
    assert np.array_equal(lo, LO) and np.array_equal(hi, HI)
    _, tight, foot, u0 = _sets(cam, W, H, lights)
    ys, xs = np.nonzero(~culled_mask(tight, W, H) & ~foot_mask(foot, W, H))
    if name != "tiny":
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
        if not pixels:
            continue
        img, _ = oracle_lib.render_pixels(v, idx, nodes, cam, lights, W, H, pixels, first_batch=batch, n_batches=1,
                                          max_depth=4, sss_bounces=3)
        rgb = img.reshape(-1, 4)[pixels, :3]
        assert not rgb.any(), (name, batch, np.array(pixels)[rgb.any(1)][:5])
    assert skipped > 0 or len(xs) == 0, "the test met samples the kernel skips"


def test_blocks_of_the_benchmark_frame():
    """1920x1080, default camera, reference light: at most 6600 blocks of 16x4
    intersect a footprint (7392 intersect a tight rectangle)."""
    W, H = 1920, 1080
    _, tight, foot, _ = _sets(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT)
    tb, fb = blocks(~culled_mask(tight, W, H), W, H), blocks(foot_mask(foot, W, H), W, H)
    print(f"blocks: tight {int(tb.sum())}, footprint rectangles "
          f"{int(blocks(~culled_mask(foot[:, :4], W, H), W, H).sum())}, footprints {int(fb.sum())}")
    assert int(tb.sum()) == 7392 and not (fb & ~tb).any()
    assert int(fb.sum()) <= 6600


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/cull_footprint_check.cpp with csrc/pt_cull.cpp under
    -fsanitize=address,undefined: the derivation over the cases and over
    degenerate inputs (a zero-size light, NaN in the camera, a light behind the
    camera, an object touching the camera plane, 7 and 8 lights), run once on
    the CPU as a program of its own (nothing is loaded into this process)."""
    exe = native.build("cull_footprint_check",
                       [os.path.join(native.TESTS, "cull_footprint_check.cpp"), os.path.join(native.CSRC, "pt_cull.cpp")],
                       ["-O1", "-g"] + native.COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                        "-fno-omit-frame-pointer", "-I", native.CSRC],
                       out_dir=tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.startswith("ok:")


# ---- the sure regions of the lights ------------------------------------------------------------------------

@pytest.mark.parametrize("name,cam,W,H,lights", FOOT_CASES, ids=FOOT_IDS)
def test_sure_regions_lie_inside_the_footprint_at_radius_zero(name, cam, W, H, lights):
    """A sure region lies inside its light's footprint(0), as a rectangle's
    pixel set; a light seen edge-on has none."""
    zero = ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights, 0.0)
    sure, n = ptamd.primary_cull_sure(cam, W, H, LO, HI, lights)
    assert sure.shape == (len(zero) - 1, 16) and 0 <= n <= len(sure)
    for l, reg in enumerate(sure):
        assert np.isfinite(reg).all()
        assert not (foot_mask(reg, W, H) & ~foot_mask(zero[l + 1], W, H)).any(), (name, l)
    if name == "edge_on":
        assert n == 0 and not any(m.any() for m in sure_masks(cam, W, H, lights))
    if name in ("default", "two_overlap"):
        assert n >= 1 and sure_masks(cam, W, H, lights)[0].any()


def test_no_sure_region_without_the_preconditions():
    """A non-finite intensity, a normal near the kernel's basis switch, a
    zero-size light, a light with a negative size component (which no ray
    ever hits): an empty region each; no footprints, no regions."""
    cam, W, H = scenes.DEFAULT_CAMERA, 96, 54
    inf = scenes.REFERENCE_LIGHT.copy()
    inf[9] = np.inf
    nan = scenes.REFERENCE_LIGHT.copy()
    nan[8] = np.nan
    switch = ptamd.pack_light([0, 2, 0], [0.0447, -0.999, 0.0], [3, 2, 1], [2.5, 2.5])
    zero = ptamd.pack_light([0, 2, 0], [0, -1, 0], [3, 2, 1], [0.0, 0.0])
    # a negative size: the kernel's half is the signed size * 0.5f and fabs(u) <= half never holds
    neg0, neg1, neg2 = (scenes.REFERENCE_LIGHT.copy() for _ in range(3))
    neg0[12], neg1[13], neg2[12:14] = -2.5, -2.5, -2.5
    for lights in (inf, nan, switch, zero, neg0, neg1, neg2):
        assert ptamd.primary_cull_footprints(cam, W, H, LO, HI, lights) is not None
        sure, n = ptamd.primary_cull_sure(cam, W, H, LO, HI, lights)
        assert n == 0 and not foot_mask(sure, W, H).any()
    assert ptamd.primary_cull_sure(scenes.camera((0.0, 0.0, 0.5)), W, H, LO, HI, scenes.REFERENCE_LIGHT) == (None, -1)


@pytest.mark.parametrize("name,cam,W,H,lights", FOOT_CASES, ids=FOOT_IDS)
def test_sure_pixels_hit_their_light_and_nothing_else(name, cam, W, H, lights):
    """The probes of the footprints' test from sure pixels, those on the
    region's rim first: every one hits that light, misses the root box's slab
    and misses every other light (two_overlap: two lights whose footprints
    overlap; a sure pixel of one there would show as a probe that hits the
    other)."""
    masks = sure_masks(cam, W, H, lights)
    L = np.asarray(lights, np.float32).reshape(-1, 16)
    lo, hi = LO.astype(np.float64), HI.astype(np.float64)
    ang = np.arange(32) * (2 * np.pi / 32)
    rnd = np.random.default_rng(23)
    for l, m in enumerate(masks):
        for px, py in _probe_pixels(m, ~m, rnd, 16):
            probes = [(R_TIGHT, a, R_TIGHT, b) for a in ang for b in ang[::2]]
            probes += [(rnd.uniform(0, R_TIGHT), rnd.uniform(0, 2 * np.pi), rnd.uniform(0, R_TIGHT), rnd.uniform(0, 2 * np.pi))
                       for _ in range(32)]
            for ra, ta, rj, tj in probes:
                o, d = rays(cam, W, H, px, py, 0.02 * ra * np.cos(ta), 0.02 * ra * np.sin(ta), rj * np.cos(tj),
                            rj * np.sin(tj))
                assert not slab_hit(o, d, lo, hi), (name, px, py, ra, ta, rj, tj)
                for k, li in enumerate(L):
                    assert light_hit(o, d, li) == (k == l), (name, l, k, px, py, ra, ta, rj, tj)


@pytest.mark.parametrize("name,cam,W,H,lights", FOOT_CASES, ids=FOOT_IDS)
def test_oracle_samples_of_sure_pixels_are_the_lights_intensity(box, name, cam, W, H, lights):
    """Sure pixels, real seeds whose two radius draws are at least
    kCullTightU0, rendered one batch at a time by the oracle over a cleared
    frame: each pixel is bitwise the running mean's step from zero with the
    sample (intensity, 1)."""
    v, idx, nodes = box
    _, _, _, u0 = _sets(cam, W, H, lights)
    L = np.asarray(lights, np.float32).reshape(-1, 16)
    for l, m in enumerate(sure_masks(cam, W, H, lights)):
        ys, xs = np.nonzero(m)
        want = np.array([L[l, 8], L[l, 9], L[l, 10], 1.0], np.float32)
        for batch in range(3):
            pixels = []
            for px, py in zip(xs, ys):
                seed = ((batch * H + int(py)) * W + int(px)) & 0xFFFFFFFF
                u = np.maximum(np.float32(1e-38), oracle_lib.rng(seed, 4))
                if u[0] >= u0 and u[2] >= u0:
                    pixels.append(int(py) * W + int(px))
            if not pixels:
                continue
            img, _ = oracle_lib.render_pixels(v, idx, nodes, cam, lights, W, H, pixels, first_batch=batch, n_batches=1,
                                              max_depth=4, sss_bounces=3)
            got = img.reshape(-1, 4)[pixels]
            # the image is the running mean after this one batch over a cleared frame (:467-469)
            mean = (np.float32(0.0) * np.float32(batch) + want) / np.float32(batch + 1)
            bad = (got.view(np.uint32) != mean.view(np.uint32)).any(1)
            assert not bad.any(), (name, l, batch, np.array(pixels)[bad][:5], got[bad][:2])


def test_sure_blocks_of_the_benchmark_frame():
    """1920x1080, default camera, reference light: at least 800 whole blocks
    of 16x4 are sure (every pixel of theirs skips with the light's intensity)."""
    W, H = 1920, 1080
    foot = ptamd.primary_cull_footprints(scenes.DEFAULT_CAMERA, W, H, LO, HI, scenes.REFERENCE_LIGHT)
    sure = sure_masks(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT)[0]
    inside = foot_mask(foot, W, H)
    whole = blocks(inside, W, H) & ~blocks(inside & ~sure, W, H)
    print(f"whole sure blocks: {int(whole.sum())}; blocks still traced: {int(blocks(inside & ~sure, W, H).sum())}")
    assert int(whole.sum()) >= 800
