"""GPU: the per-sample skip of the tight cull rectangles (PT_OPT_CULL_TIGHT,
csrc/pt_cull.h): frames with the option on and off are bitwise equal and equal
to the oracle's, and the counting kernel skips exactly the samples the
header's definition says (the image cannot show the predicate: the margin
samples the kernel must trace are black in the oracle too).

The frame is the box at 320x180, 4 spp: 98 of its 326 live 16x4 pixel blocks
lie wholly between the loose and the tight rectangles
(test_cull_tight.py, test_blocks_in_the_margin), so whole waves take the skip,
others take it lane by lane.
"""
import functools

import numpy as np
import pytest

import ptamd
import scenes
from cull_support import skip_counts
from support import oracle_frame, renderer, same, scene

pytestmark = pytest.mark.gpu

W, H, DEPTH, SSS = 320, 180, 4, 3


@functools.lru_cache(maxsize=None)
def _oracle(first, nb, nranks=1, rank=0):
    return oracle_frame(scene("box"), scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, W, H, 0, first + nb, DEPTH, SSS,
                        nranks=nranks, rank=rank)


def _renderer(tight, lanes=1, cam=scenes.DEFAULT_CAMERA, count=False):
    return renderer(scene("box"), cam, depth=DEPTH, sss=SSS,
                    options=[(ptamd.PT_OPT_CULL_TIGHT, tight), (ptamd.PT_OPT_SAMPLE_LANES, lanes)] +
                    ([(ptamd.PT_OPT_COUNT_TRACED, 1)] if count else []))


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_skip_on_and_off_equal_the_oracle(lanes):
    """A fresh accumulator (batches 0-3), then batches 4-7 on top of it (a
    non-zero accumulator), then -- with PT_OPT_FRESH_BATCH0 -- batches 0-3
    again over the stale frame."""
    frames = {}
    for tight in (1, 0):
        r = _renderer(tight, lanes)
        r.resize_and_clear(W, H)
        r.render(0, 4)
        a = r.read_accum()
        r.render(4, 4)
        b = r.read_accum()
        r.set_option(ptamd.PT_OPT_FRESH_BATCH0, 1)
        r.render(0, 4)
        c = r.read_accum()
        r.close()
        frames[tight] = (a, b, c)
    for k, what in enumerate(("batches 0-3", "batches 4-7 on top", "batches 0-3 over a stale frame")):
        same(frames[0][k], frames[1][k], f"lanes={lanes} {what}: PT_OPT_CULL_TIGHT 0 against 1")
    same(frames[1][0], _oracle(0, 4), f"lanes={lanes} batches 0-3 against the oracle")
    same(frames[1][1], _oracle(4, 4), f"lanes={lanes} batches 0-7 against the oracle")
    same(frames[1][2], _oracle(0, 4), f"lanes={lanes} fresh restart against the oracle")


@pytest.mark.parametrize("rank", [0, 1])
def test_two_rank_share(rank):
    frames = {}
    for tight in (1, 0):
        r = _renderer(tight)
        r.set_partition(2, rank)
        r.resize_and_clear(W, H)
        r.render(0, 4)
        frames[tight] = r.read_accum()
        r.close()
    same(frames[0], frames[1], f"rank {rank} of 2: PT_OPT_CULL_TIGHT 0 against 1")
    ref = _oracle(0, 4, 2, rank).reshape(-1, 4)
    own = ref[:, 3] != 0   # the oracle leaves the other rank's pixels untouched (0)
    assert own.any() and not own.all()
    same(frames[1].reshape(-1, 4)[own], ref[own], f"rank {rank} of 2 against the oracle")


@pytest.mark.parametrize("kernel", [ptamd.KERNEL_RECURSIVE, ptamd.KERNEL_WAVEFRONT])
def test_counting_mode_shows_skipped_primaries(kernel):
    counts, frames = {}, {}
    for tight in (1, 0):
        r = _renderer(tight, count=True)
        r.set_option(ptamd.PT_OPT_KERNEL, kernel)
        r.resize_and_clear(W, H)
        r.reset_stats()
        r.render(0, 4)
        frames[tight] = r.read_accum()
        counts[tight] = r.traced()
        assert r.last_kernel() == kernel
        r.close()
    same(frames[0], frames[1], "counting mode: PT_OPT_CULL_TIGHT 0 against 1")
    same(frames[1], _oracle(0, 4), "counting mode against the oracle")
    print(f"kernel {kernel}: primaries on {counts[1]['primaries']}, off {counts[0]['primaries']}")
    assert 0 < counts[1]["primaries"] < counts[0]["primaries"] <= W * H * 4
    assert counts[1]["closest_walks"] < counts[0]["closest_walks"]


@pytest.mark.parametrize("kernel,lanes", [(ptamd.KERNEL_RECURSIVE, 1), (ptamd.KERNEL_WAVEFRONT, 1),
                                          (ptamd.KERNEL_RECURSIVE, 4)])
def test_skip_counts_are_exact(kernel, lanes):
    """The image cannot show whether the kernel evaluates the skip predicate:
    every margin sample it must trace (a radius draw below kCullTightU0) is
    (0,0,0) in the oracle too (767 of 767 over batches 0-599), so a kernel that
    skipped every margin sample would render the same frame.  The counters
    can: with the option off every sample of a live pixel generates its
    primary ray, with it on exactly the margin samples whose two radius draws
    are at least u0 do not (cull_support.skip_counts, from the header's
    definition).  At 4 lanes the samples of one pixel sit in neighbouring
    lanes."""
    nb = 8
    live, skipped, traced = skip_counts(scenes.DEFAULT_CAMERA, W, H, scenes.REFERENCE_LIGHT, 0, nb)
    assert traced >= 5 and skipped > 1000, "the batches exercise both sides of the predicate"
    counts, frames = {}, {}
    for tight in (1, 0):
        r = _renderer(tight, lanes, count=True)
        r.set_option(ptamd.PT_OPT_KERNEL, kernel)
        r.resize_and_clear(W, H)
        r.reset_stats()
        r.render(0, nb)
        frames[tight] = r.read_accum()
        counts[tight] = r.traced()
        assert r.last_kernel() == kernel
        r.close()
    print(f"kernel {kernel} lanes {lanes}: primaries on {counts[1]['primaries']}, off {counts[0]['primaries']}; "
          f"expected off {live * nb}, skipped {skipped}, margin samples traced {traced}")
    same(frames[0], frames[1], "counting mode: PT_OPT_CULL_TIGHT 0 against 1")
    same(frames[1], _oracle(4, 4), "counting mode against the oracle")
    assert counts[0]["primaries"] == live * nb
    assert counts[0]["primaries"] - counts[1]["primaries"] == skipped
    assert 0 < counts[1]["primaries"] < counts[0]["primaries"] <= W * H * nb
    assert counts[1]["closest_walks"] < counts[0]["closest_walks"]


def test_no_guarantee_no_skip():
    """A camera inside the box: neither derivation gives rectangles, both
    settings trace every sample."""
    cam = scenes.camera((0.0, 0.0, 0.5))
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    assert ptamd.primary_cull_rects(cam, W, H, lo, hi, scenes.REFERENCE_LIGHT) is None
    assert ptamd.primary_cull_rects_r(cam, W, H, lo, hi, scenes.REFERENCE_LIGHT)[0] is None
    frames = {}
    for tight in (1, 0):
        r = _renderer(tight, cam=cam, count=True)
        r.resize_and_clear(W, H)
        r.reset_stats()
        r.render(0, 2)
        frames[tight] = r.read_accum()
        assert r.traced()["primaries"] == W * H * 2
        r.close()
    same(frames[0], frames[1], "camera inside the box: PT_OPT_CULL_TIGHT 0 against 1")


def test_option_range():
    r = ptamd.Renderer(0)
    with pytest.raises(ptamd.PTError, match="PT_OPT_CULL_TIGHT"):
        r.set_option(ptamd.PT_OPT_CULL_TIGHT, 2)
    r.close()
