"""GPU: the per-sample skip by footprints (PT_OPT_CULL_FOOTPRINT,
csrc/pt_cull.h): frames with the option on and off are bitwise equal and equal
to the oracle's, and the counting kernel skips exactly the samples the
header's definition says -- the image cannot show the predicate, the skipped
samples being black in the oracle too.

The frame is the box at 320x180: 228 of its 326 live 16x4 pixel blocks
intersect a tight rectangle, 210 a footprint, so whole waves change sides and
others do lane by lane (the light's footprint has two slanted edges).
"""
import functools

import numpy as np
import pytest

import ptamd
import scenes
from cull_foot_support import HI, LO, OVERLAP, blocks, foot_mask, foot_skip_counts, sure_masks
from cull_support import culled_mask, skip_counts
from support import oracle_frame, renderer, same, same_nan, scene

pytestmark = pytest.mark.gpu

W, H, DEPTH, SSS = 320, 180, 4, 3
FOOT = ptamd.PT_OPT_CULL_FOOTPRINT


@functools.lru_cache(maxsize=None)
def _oracle(first, nb, nranks=1, rank=0, two=False):
    return oracle_frame(scene("box"), scenes.DEFAULT_CAMERA, OVERLAP if two else scenes.REFERENCE_LIGHT, W, H, 0,
                        first + nb, DEPTH, SSS, nranks=nranks, rank=rank)


def _renderer(foot, lanes=1, cam=scenes.DEFAULT_CAMERA, lights=scenes.REFERENCE_LIGHT, count=False, more=()):
    return renderer(scene("box"), cam, lights=lights, depth=DEPTH, sss=SSS,
                    options=[(FOOT, foot), (ptamd.PT_OPT_SAMPLE_LANES, lanes)] +
                    ([(ptamd.PT_OPT_COUNT_TRACED, 1)] if count else []) + list(more))


def test_the_frame_has_blocks_that_change_sides():
    tight, _ = ptamd.primary_cull_rects_r(scenes.DEFAULT_CAMERA, W, H, LO, HI, scenes.REFERENCE_LIGHT)
    foot = ptamd.primary_cull_footprints(scenes.DEFAULT_CAMERA, W, H, LO, HI, scenes.REFERENCE_LIGHT)
    tb, fb = blocks(~culled_mask(tight, W, H), W, H), blocks(foot_mask(foot, W, H), W, H)
    assert (int(tb.sum()), int(fb.sum())) == (228, 210)
    assert np.any(foot[1, 4:6] != 0), "the light's footprint has a slanted edge"


def test_what_is_in_force():
    r = _renderer(-1)
    r.resize_and_clear(W, H)
    assert r.cull_info() == (2, 2, 1)
    for opts, want in (([(FOOT, 0)], (2, 0, 0)), ([(FOOT, -1), (ptamd.PT_OPT_COUNT_TRACED, 1)], (2, 0, 0)),
                       ([(FOOT, 1)], (2, 2, 1)), ([(ptamd.PT_OPT_COUNT_TRACED, 0), (ptamd.PT_OPT_CULL_TIGHT, 0)], (0, 0, 0)),
                       ([(ptamd.PT_OPT_CULL_TIGHT, 1), (ptamd.PT_OPT_PRIMARY_CULL, 0)], (0, 0, 0)),
                       ([(ptamd.PT_OPT_PRIMARY_CULL, 1)], (2, 2, 1))):
        for k, v in opts:
            r.set_option(k, v)
        assert r.cull_info() == want, opts
    r.set_camera(scenes.camera((0.0, 0.0, 0.5)))   # inside the box: nothing is derived
    assert r.cull_info() == (0, 0, 0)
    with pytest.raises(ptamd.PTError, match="PT_OPT_CULL_FOOTPRINT"):
        r.set_option(FOOT, 2)
    with pytest.raises(ptamd.PTError, match="PT_OPT_CULL_FOOTPRINT"):
        r.set_option(FOOT, -2)
    r.close()


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_footprints_on_and_off_equal_the_oracle(lanes):
    """A fresh accumulator (batches 0-3), then batches 4-7 on top of it (a
    non-zero accumulator), then -- with PT_OPT_FRESH_BATCH0 -- batches 0-3
    again over the stale frame."""
    frames = {}
    for foot in (-1, 0):
        r = _renderer(foot, lanes)
        r.resize_and_clear(W, H)
        assert r.cull_info() == ((2, 2, 1) if foot else (2, 0, 0))
        r.render(0, 4)
        a = r.read_accum()
        r.render(4, 4)
        b = r.read_accum()
        r.set_option(ptamd.PT_OPT_FRESH_BATCH0, 1)
        r.render(0, 4)
        c = r.read_accum()
        r.close()
        frames[foot] = (a, b, c)
    for k, what in enumerate(("batches 0-3", "batches 4-7 on top", "batches 0-3 over a stale frame")):
        same(frames[-1][k], frames[0][k], f"lanes={lanes} {what}: PT_OPT_CULL_FOOTPRINT -1 against 0")
    same(frames[-1][0], _oracle(0, 4), f"lanes={lanes} batches 0-3 against the oracle")
    same(frames[-1][1], _oracle(4, 4), f"lanes={lanes} batches 0-7 against the oracle")
    same(frames[-1][2], _oracle(0, 4), f"lanes={lanes} fresh restart against the oracle")


def test_moments():
    out = {}
    for foot in (-1, 0):
        r = _renderer(foot, more=[(ptamd.PT_OPT_MOMENTS, 1)])
        r.resize_and_clear(W, H)
        r.render(0, 4)
        r.render(4, 4)
        out[foot] = (r.read_accum(), r.read_moments())
        r.close()
    same(out[-1][0], out[0][0], "moments on: the frame, PT_OPT_CULL_FOOTPRINT -1 against 0")
    same(out[-1][0], _oracle(4, 4), "moments on: the frame against the oracle")
    assert out[-1][1][1] == out[0][1][1]
    same(out[-1][1][0], out[0][1][0], "the moments, PT_OPT_CULL_FOOTPRINT -1 against 0")


@pytest.mark.parametrize("rank", [0, 1])
def test_two_rank_share(rank):
    frames = {}
    for foot in (-1, 0):
        r = _renderer(foot)
        r.set_partition(2, rank)
        r.resize_and_clear(W, H)
        r.render(0, 4)
        frames[foot] = r.read_accum()
        r.close()
    same(frames[-1], frames[0], f"rank {rank} of 2: PT_OPT_CULL_FOOTPRINT -1 against 0")
    ref = _oracle(0, 4, 2, rank).reshape(-1, 4)
    own = ref[:, 3] != 0   # the oracle leaves the other rank's pixels untouched (0)
    assert own.any() and not own.all()
    same(frames[-1].reshape(-1, 4)[own], ref[own], f"rank {rank} of 2 against the oracle")


def test_wavefront_kernel():
    frames = {}
    for foot in (-1, 0):
        r = _renderer(foot, more=[(ptamd.PT_OPT_KERNEL, ptamd.KERNEL_WAVEFRONT)])
        r.resize_and_clear(W, H)
        r.render(0, 4)
        r.render(4, 2)
        assert r.last_kernel() == ptamd.KERNEL_WAVEFRONT
        frames[foot] = r.read_accum()
        r.close()
    same(frames[-1], frames[0], "wavefront: PT_OPT_CULL_FOOTPRINT -1 against 0")
    same(frames[-1], _oracle(4, 2), "wavefront against the oracle")


def test_two_lights_with_overlapping_footprints():
    foot = ptamd.primary_cull_footprints(scenes.DEFAULT_CAMERA, W, H, LO, HI, OVERLAP)
    assert (foot_mask(foot[1], W, H) & foot_mask(foot[2], W, H)).any(), "the lights' footprints overlap"
    frames = {}
    for f in (-1, 0):
        r = _renderer(f, lights=OVERLAP)
        r.resize_and_clear(W, H)
        assert r.cull_info()[:2] == (3, 3 if f else 0)
        r.render(0, 4)
        frames[f] = r.read_accum()
        r.close()
    same(frames[-1], frames[0], "two lights: PT_OPT_CULL_FOOTPRINT -1 against 0")
    same(frames[-1], _oracle(0, 4, two=True), "two lights against the oracle")


def test_sure_pixels_of_the_frame():
    """Whole waves and single lanes take the light's intensity: 16 of the
    frame's 16x4 blocks are sure throughout, others in part."""
    sure = sure_masks(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT)[0]
    whole = blocks(sure, W, H) & ~blocks(~sure, W, H)
    assert int(whole.sum()) == 16 and int(blocks(sure, W, H).sum()) > 16
    ov = sure_masks(scenes.DEFAULT_CAMERA, W, H, OVERLAP)
    assert ov[0].any() and ov[1].any(), "two lights, both with sure pixels, none shared"
    assert not (ov[0] & ov[1]).any()


@pytest.mark.parametrize("kernel", [ptamd.KERNEL_RECURSIVE, ptamd.KERNEL_WAVEFRONT])
def test_a_non_finite_light_gets_no_sure_region(kernel):
    """An infinite intensity: footprints, no sure region; the frames of both
    settings are equal (NaN where NaN) and equal the oracle's."""
    lights = scenes.REFERENCE_LIGHT.copy()
    lights[9] = np.inf
    frames = {}
    for foot in (-1, 0):
        r = _renderer(foot, lights=lights, more=[(ptamd.PT_OPT_KERNEL, kernel)])
        r.resize_and_clear(W, H)
        assert r.cull_info() == ((2, 2, 0) if foot else (2, 0, 0))
        r.render(0, 4)
        frames[foot] = r.read_accum()
        r.close()
    ref = oracle_frame(scene("box"), scenes.DEFAULT_CAMERA, lights, W, H, 0, 4, DEPTH, SSS)
    same_nan(frames[-1], frames[0], "non-finite light: PT_OPT_CULL_FOOTPRINT -1 against 0")
    same_nan(frames[-1], ref, "non-finite light against the oracle")


@pytest.mark.parametrize("kernel", [ptamd.KERNEL_RECURSIVE, ptamd.KERNEL_WAVEFRONT])
@pytest.mark.parametrize("size", [(-2.5, 2.5), (2.5, -2.5)], ids=["neg0", "neg1"])
def test_a_light_with_a_negative_size_gets_no_sure_region(kernel, size):
    """The kernel's half is the signed size * 0.5f, so intersectAreaLight
    never hits such a light, though it still lights the scene: the pixels that
    would be its sure region are black.  Footprints, no sure region; the frames
    of both settings are equal and equal the oracle's."""
    lights = scenes.REFERENCE_LIGHT.copy()
    lights[12:14] = size
    frames = {}
    for foot in (-1, 0):
        r = _renderer(foot, lights=lights, more=[(ptamd.PT_OPT_KERNEL, kernel)])
        r.resize_and_clear(W, H)
        assert r.cull_info() == ((2, 2, 0) if foot else (2, 0, 0))
        r.render(0, 4)
        frames[foot] = r.read_accum()
        r.close()
    ref = oracle_frame(scene("box"), scenes.DEFAULT_CAMERA, lights, W, H, 0, 4, DEPTH, SSS)
    would_be = sure_masks(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT)[0]
    assert not ref.reshape(H, W, 4)[would_be][:, :3].any(), "the light is never hit: black where it would be seen"
    assert ref.reshape(H, W, 4)[..., :3].any(), "... but it lights the box"
    same(frames[-1], frames[0], "negative-size light: PT_OPT_CULL_FOOTPRINT -1 against 0")
    same(frames[-1], ref, "negative-size light against the oracle")


def test_no_guarantee_no_skip():
    """A camera inside the box: no derivation gives anything, both settings
    trace every sample."""
    cam = scenes.camera((0.0, 0.0, 0.5))
    assert ptamd.primary_cull_footprints(cam, W, H, LO, HI, scenes.REFERENCE_LIGHT) is None
    frames = {}
    for foot in (1, 0):
        r = _renderer(foot, cam=cam, count=True)
        r.resize_and_clear(W, H)
        r.reset_stats()
        r.render(0, 2)
        frames[foot] = r.read_accum()
        assert r.traced()["primaries"] == W * H * 2 and r.cull_info() == (0, 0, 0)
        r.close()
    same(frames[1], frames[0], "camera inside the box: PT_OPT_CULL_FOOTPRINT 1 against 0")
    ref = oracle_frame(scene("box"), cam, scenes.REFERENCE_LIGHT, W, H, 0, 2, DEPTH, SSS)
    same(frames[1], ref, "camera inside the box against the oracle")


@pytest.mark.parametrize("kernel,lanes", [(ptamd.KERNEL_RECURSIVE, 1), (ptamd.KERNEL_WAVEFRONT, 1),
                                          (ptamd.KERNEL_RECURSIVE, 4)])
def test_skip_counts_are_exact(kernel, lanes):
    """With PT_OPT_COUNT_TRACED and the option at 1 the primaries are the
    samples of the live pixels minus those of pixels outside every footprint
    whose two radius draws are at least u0 (cull_foot_support.foot_skip_counts,
    from the new entry point and the shader's RNG); with the default -1 the
    counting pass keeps the rectangles, and its counts are those of option 0
    (cull_support.skip_counts).  Both kernels, so they agree."""
    nb = 8
    live, skipped, traced = foot_skip_counts(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT, 0, nb)
    live_r, skipped_r, _ = skip_counts(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT, 0, nb)
    assert live == live_r and skipped > skipped_r + 1000 and traced >= 5, "the footprints skip more, and not everything"
    counts, frames = {}, {}
    for foot in (1, -1, 0):
        r = _renderer(foot, lanes, count=True)
        r.set_option(ptamd.PT_OPT_KERNEL, kernel)
        r.resize_and_clear(W, H)
        r.reset_stats()
        r.render(0, nb)
        frames[foot] = r.read_accum()
        counts[foot] = r.traced()
        assert r.last_kernel() == kernel
        r.close()
    print(f"kernel {kernel} lanes {lanes}: primaries at 1 {counts[1]['primaries']}, at -1 {counts[-1]['primaries']}, "
          f"at 0 {counts[0]['primaries']}; live samples {live * nb}, skipped by footprints {skipped}, by rectangles {skipped_r}")
    same(frames[1], frames[0], "counting mode: PT_OPT_CULL_FOOTPRINT 1 against 0")
    same(frames[-1], frames[0], "counting mode: PT_OPT_CULL_FOOTPRINT -1 against 0")
    same(frames[1], _oracle(4, 4), "counting mode against the oracle")
    assert counts[1]["primaries"] == live * nb - skipped
    assert counts[0]["primaries"] == live * nb - skipped_r
    assert counts[-1] == counts[0]
    assert counts[1]["closest_walks"] < counts[0]["closest_walks"]
