"""GPU: adaptive sampling (pt_adaptive_begin / pt_adaptive_advance).  The
contract: after an adaptive render every 16x16 tile T has a count n_T, and its
pixels hold, in the accumulation image and in the moments image, the bits
pt_render(0, n_T) leaves there.  So the tests render the frame the ordinary
way at every count of the schedule, compose the expected images by tile and
ask for equal bits; simulate the whole loop in numpy from those renders and
ask for the same counts and the same live lists; do so on every kernel path;
check the device rule against the host's, the refusals, what ends the state,
and the filter of the result.

The frame is 72x40: 5 x 3 tiles, partial on both edges; min 2, step 3, max 9
gives the counts 2, 5, 8 and 9, so the cap is exercised."""
import ctypes
import functools

import numpy as np
import pytest

import adaptive_ref as A
import ptamd
import scenes
import sweep_support
from support import bits, dev, read_device, renderer, same, scene

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 72, 40
BX, BY = A.tiles(W, H)
# The threshold and the floor spread the tiles of this small frame.  A pixel that one of n samples hit has
# m1 = L / n and m2 = L * L / n, hence e_p = 1 whatever n unless the floor lifts its denominator: with a small
# floor every lit tile of the frame has E_T = 1 at every count.  At floor 1.5 and threshold 0.5 the box's tiles
# end at 2 (culled), 8 and 9, its rounds list 6, 6 and 4 of the 15 tiles, and no E_T of any round lies within
# 8 % of the threshold on either scene (profiles/adaptive/test_frame_errors.json holds them); both are exact floats
PARAMS = (2, 9, 3, 0.5, 1.5)
MOMENTS = [(ptamd.PT_OPT_MOMENTS, 1)]
UNSUPPORTED, INVALID = -5, -1

CUBOIDS_CAM = sweep_support.HULL_CASES["cuboid"][1]
CUBOIDS_LIGHTS = sweep_support.HULL_CASES["cuboid"][2]
SCENES = {
    "box": lambda: (scene("box"), scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT),
    "cuboids-stacked": lambda: (scene("cuboids-stacked", sweep_support.GPU_MAKERS), CUBOIDS_CAM, CUBOIDS_LIGHTS),
}


def _renderer(name="box", options=()):
    sc, cam, lights = SCENES[name]()
    return renderer(sc, cam, lights, size=(W, H), options=MOMENTS + list(options))


@functools.lru_cache(maxsize=None)
def uniform(name="box", base=0):
    """count -> (accumulator (H, W, 4), moments (H, W, 2)) of pt_render(0, count), for every count of the
    schedule, on the default kernel path.  Rendered once per scene and seed base, shared, read-only."""
    r = _renderer(name, [(ptamd.PT_OPT_SEED_BASE, base)])
    out = {}
    for n in A.schedule(PARAMS):
        r.clear()
        r.render(0, n)
        acc = r.read_accum().reshape(H, W, 4)
        mom, got_n = r.read_moments()
        assert got_n == n
        acc.setflags(write=False)
        mom.setflags(write=False)
        out[n] = (acc, mom)
    return out


def _accs(name="box", base=0):
    return {n: a for n, (a, _) in uniform(name, base).items()}


def _moms(name="box", base=0):
    return {n: m for n, (_, m) in uniform(name, base).items()}


def run(r, params=PARAMS, rounds=100):
    """An adaptive render to its end: (counts (BY, BX), accumulator, moments)."""
    r.adaptive_begin(params)
    r.adaptive_advance(rounds)
    counts, _ = r.adaptive_counts()
    acc = r.read_accum().reshape(H, W, 4)
    mom, n = r.read_moments()
    assert n == 0, "the moments of an adaptive render have no single n"
    return counts, acc, mom


def check_composition(counts, acc, mom, name="box", base=0, what=""):
    same(acc, A.compose(_accs(name, base), counts, W, H), f"{what}: accumulator")
    same(mom, A.compose(_moms(name, base), counts, W, H), f"{what}: moments")


def test_composition():
    r = _renderer()
    counts, acc, mom = run(r)
    e2 = A.select(_moms()[2], np.full(BX * BY, 2, np.uint32), W, H, PARAMS)[1]
    print("\nE_T at 2 samples:", np.sort(e2), "\ncounts:\n", counts)
    distinct = set(int(n) for n in counts.reshape(-1))
    assert distinct <= set(A.schedule(PARAMS)), distinct
    assert len(distinct) >= 3 and PARAMS[0] in distinct and PARAMS[1] in distinct, \
        f"the threshold must spread the tiles: counts {sorted(distinct)}"
    check_composition(counts, acc, mom, what="box")
    rounds, live, total = r.adaptive_info()
    tile_px = np.array([[min(16, W - 16 * x) * min(16, H - 16 * y) for x in range(BX)] for y in range(BY)])
    assert (rounds, live, total) == (3, 0, int(np.sum(counts.astype(np.int64) * tile_px)))
    assert total < PARAMS[1] * W * H


def test_counts_follow_the_rule():
    want, lives = A.simulate(_moms(), W, H, PARAMS)
    r = _renderer()
    counts, _, _ = run(r)
    assert np.array_equal(counts.reshape(-1), want), (counts, want.reshape(BY, BX))
    # round by round: the live list is the simulation's, ascending, with its batches
    r.adaptive_begin(PARAMS)
    first = r.adaptive_live()
    assert [tuple(e) for e in first] == [((b % BX) * 16, (b // BX) * 16, 0, PARAMS[0]) for b in range(BX * BY)]
    assert r.adaptive_info()[:2] == (0, BX * BY)
    for k, live in enumerate(lives):
        r.adaptive_advance(1)
        got = [tuple(int(v) for v in e) for e in r.adaptive_live()]
        assert got == [((b % BX) * 16, (b // BX) * 16, first_batch, nb) for b, first_batch, nb in live], (k, got, live)
        done, n_live, _ = r.adaptive_info()
        assert done == k + 1 and n_live == (len(live) if k + 1 < len(lives) else 0)
        sim_counts, _ = A.simulate(_moms(), W, H, PARAMS, rounds=k + 1)
        got_counts, got_err = r.adaptive_counts()
        assert np.array_equal(got_counts.reshape(-1), sim_counts)
        before = sim_counts - np.array([dict((b, nb) for b, _, nb in live).get(b, 0) for b in range(BX * BY)], np.uint32)
        same(got_err.reshape(-1), A.select(A.compose(_moms(), before, W, H), before, W, H, PARAMS)[1], f"round {k}: E_T")
    assert any(len(l) not in (0, BX * BY) for l in lives), "some round must list a part of the tiles"


LANES = ptamd.PT_OPT_SAMPLE_LANES
PATHS = {
    "lanes 1": [(LANES, 1)],
    "lanes 2": [(LANES, 2)],
    "lanes 4": [(LANES, 4)],
    "lanes 8": [(LANES, 8)],
    "sweep off": [(ptamd.PT_OPT_SMALL_SWEEP, 0)],
    "sweep on": [(ptamd.PT_OPT_SMALL_SWEEP, 1)],
    "sweep without hull faces": [(ptamd.PT_OPT_SWEEP_HULL, 0)],
    "sweep without the cube walk": [(ptamd.PT_OPT_SWEEP_CUBE, 0)],
    "device memory, no exit skip": [(ptamd.PT_OPT_SCENE_IN_LDS, 0), (ptamd.PT_OPT_EXIT_SKIP, 0)],
    "device memory, exit skip": [(ptamd.PT_OPT_SCENE_IN_LDS, 0), (ptamd.PT_OPT_EXIT_SKIP, 1)],
    "primary cull off": [(ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "tight cull off": [(ptamd.PT_OPT_CULL_TIGHT, 0)],
}


@pytest.mark.parametrize("path", list(PATHS))
def test_every_kernel_path(path):
    counts, acc, mom = run(_renderer("box", PATHS[path]))
    assert len(set(counts.reshape(-1).tolist())) >= 3
    check_composition(counts, acc, mom, what=path)


def test_seed_base():
    base = 12345
    counts, acc, mom = run(_renderer("box", [(ptamd.PT_OPT_SEED_BASE, base)]))
    check_composition(counts, acc, mom, base=base, what=f"seed base {base}")
    assert not np.array_equal(bits(acc), bits(A.compose(_accs(), counts, W, H)))   # another base, another frame


def test_a_scene_that_is_not_a_cube_table():
    r = _renderer("cuboids-stacked", [(ptamd.PT_OPT_SMALL_SWEEP, 1)])
    walk = ctypes.c_int(0)
    assert ptamd.lib().pt_sweep_walk(r._c, ctypes.byref(walk)) == 0 and walk.value in (1, 2), walk.value
    counts, acc, mom = run(r)
    print("\ncuboids counts:\n", counts)
    assert len(set(counts.reshape(-1).tolist())) >= 2
    check_composition(counts, acc, mom, name="cuboids-stacked", what="stacked cuboids")
    want, _ = A.simulate(_moms("cuboids-stacked"), W, H, PARAMS)
    assert np.array_equal(counts.reshape(-1), want)


@pytest.mark.parametrize("frame", ["crafted", "an ulp above"])
def test_device_select_against_host(frame):
    import torch
    m, _ = A.crafted() if frame == "crafted" else A.just_above_threshold()
    r = ptamd.Renderer(0)
    dm = dev(m)
    for counts in (np.full(6, 2, np.uint32), np.array([2, 5, 8, 5, 2, 8], np.uint32), np.full(6, 8, np.uint32),
                   np.full(6, 9, np.uint32)):
        dn = torch.from_numpy(counts.view(np.int32).copy()).cuda()
        dnext = torch.full((6,), -1, dtype=torch.int32, device="cuda")
        derr = torch.full((6,), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.adaptive_select(dm.data_ptr(), dn.data_ptr(), A.W0, A.H0, dnext.data_ptr(), derr.data_ptr(), A.PARAMS0)
        r.synchronize()
        want_n, want_e = ptamd.adaptive_select_host(m, counts, A.W0, A.H0, A.PARAMS0)
        assert np.array_equal(dnext.cpu().numpy().view(np.uint32), want_n), (frame, counts)
        same(derr.cpu().numpy(), want_e, f"{frame} {counts}: E_T")
        # in place: next_counts may be counts
        r.adaptive_select(dm.data_ptr(), dn.data_ptr(), A.W0, A.H0, dn.data_ptr(), derr.data_ptr(), A.PARAMS0)
        r.synchronize()
        assert np.array_equal(dn.cpu().numpy().view(np.uint32), want_n)
    rc = ptamd.lib().pt_adaptive_select(r._c, dm.data_ptr(), dn.data_ptr(), A.W0, A.H0, None, dn.data_ptr(), dn.data_ptr())
    assert rc == INVALID


def _begin_code(r, params=PARAMS):
    p = ptamd.AdaptiveParams(*params)
    return ptamd.lib().pt_adaptive_begin(r._c, ctypes.byref(p))


def test_refusals():
    L = ptamd.lib()
    sc, cam, lights = SCENES["box"]()
    cases = {
        "wavefront": lambda r: r.set_option(ptamd.PT_OPT_KERNEL, 3),
        "partition": lambda r: r.set_partition(2, 0),
        "stats": lambda r: r.set_stats_mode(True),
        "counting": lambda r: r.set_option(ptamd.PT_OPT_COUNT_TRACED, 1),
    }
    for name, set_up in cases.items():
        r = _renderer()
        assert L.pt_adaptive_advance(r._c, 1) == INVALID, "advance before begin"
        set_up(r)
        assert _begin_code(r) == UNSUPPORTED, name
        assert b"adaptive" in L.pt_last_error(), name
        assert L.pt_adaptive_advance(r._c, 1) == INVALID, name
    g = ptamd.Renderer(devices=[0, 0])
    assert _begin_code(g) == UNSUPPORTED and L.pt_adaptive_advance(g._c, 1) == UNSUPPORTED
    assert L.pt_adaptive_info(g._c, None, None, None) == UNSUPPORTED
    r = renderer(sc, cam, lights, size=(W, H))                       # PT_OPT_MOMENTS 0
    assert _begin_code(r) == INVALID and b"PT_OPT_MOMENTS" in L.pt_last_error()
    r = _renderer()
    for bad in [(1, 9, 3, 0.5, 0.01), (4, 3, 3, 0.5, 0.01), (2, 9, 0, 0.5, 0.01), (2, 9, 3, float("nan"), 0.01),
                (2, 9, 3, 0.5, 0.0)]:
        assert _begin_code(r, bad) == INVALID, bad
    # under auto the adaptive calls run the path-recursive kernel
    r.adaptive_begin(PARAMS)
    assert r.last_kernel() == ptamd.KERNEL_RECURSIVE


def test_state():
    L = ptamd.lib()
    r = _renderer()
    counts, acc, mom = run(r)
    # past the last round nothing changes
    r.adaptive_advance(5)
    counts2, _ = r.adaptive_counts()
    assert np.array_equal(counts, counts2) and r.adaptive_info()[0] == 3
    same(r.read_accum(), acc, "advance past the last round: accumulator")
    same(r.read_moments()[0], mom, "advance past the last round: moments")
    assert r.read_moments()[1] == 0 and not r.moments_ptr()
    with pytest.raises(ptamd.PTError):
        r.denoise_var()                                               # no single n
    # an ordinary render afterwards is the ordinary frame, and ends the state
    r.render(0, 4)
    fresh = _renderer()
    fresh.render(0, 4)
    same(r.read_accum(), fresh.read_accum(), "pt_render(0, 4) after an adaptive render")
    m4, n4 = r.read_moments()
    assert n4 == 4
    same(m4, fresh.read_moments()[0], "its moments")
    assert L.pt_adaptive_advance(r._c, 1) == INVALID and L.pt_adaptive_info(r._c, None, None, None) == INVALID
    assert not r.adaptive_ptr(0)
    # ... as do a clear, a resize, the uploads and the parameters
    sc, cam, lights = SCENES["box"]()
    enders = {
        "clear": lambda: r.clear(),
        "resize": lambda: r.resize_and_clear(W, H),
        "scene": lambda: r.upload_scene(*sc),
        "lights": lambda: r.upload_lights(lights),
        "params": lambda: r.set_params(4, 3),
    }
    for name, end in enders.items():
        r.clear()
        r.adaptive_begin(PARAMS)
        assert r.adaptive_ptr(0), name
        end()
        assert L.pt_adaptive_advance(r._c, 1) == INVALID, name
    # and a new begin starts over: the same result
    counts3, acc3, _ = run(r)
    assert np.array_equal(counts3, counts)
    same(acc3, acc, "a second adaptive render")


def test_denoise():
    r = _renderer()
    counts, acc, mom = run(r)
    got = r.adaptive_denoise()
    guide = r.read_guide()
    n_px = np.repeat(np.repeat(counts, 16, 0), 16, 1)[:H, :W].astype(np.uint32)
    with np.errstate(all="ignore"):
        var = (np.fmax(F(0), mom[..., 1] - mom[..., 0] * mom[..., 0]) / (n_px - np.uint32(1)).astype(F)).astype(F)
    same(read_device(r, r.adaptive_ptr(2), (H, W)), var, "the variance plane")
    same(got, ptamd.denoise_var_plane_host(acc, var, guide, W, H), "adaptive_denoise against the host's passes")
    assert not np.array_equal(bits(got), bits(acc))
    same(r.read_accum(), acc, "the filter leaves the accumulator")
    assert ptamd.lib().pt_adaptive_denoise(r._c, None, r.accum_ptr()) == INVALID
    r.clear()
    assert ptamd.lib().pt_adaptive_denoise(r._c, None, None) == INVALID   # no adaptive render
