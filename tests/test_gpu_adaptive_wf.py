"""GPU: adaptive sampling with its rounds on the wavefront pipeline
(PT_OPT_ADAPTIVE_WF 1).  The contract is test_gpu_adaptive.py's: after an
adaptive render every 16x16 tile T has a count n_T and holds, in the
accumulation image and in the moments image, the bits pt_render(0, n_T) leaves
there; the counts and every round's live list are those of the numpy
simulation.  The expected images are composed from uniform renders on the
default (path-recursive) path with the option off, so each test also holds the
wavefront rounds against the path-recursive kernel, bit for bit.

The frame is that file's, 72x40 (5 x 3 tiles, partial on both edges) at
(2, 9, 3, 0.5, 1.5); the box's tiles end at 2, 8 and 9 there.  The displaced
sphere (1280 triangles, too large for LDS: the culled wide walk) from
(3, 2, 4) ends at 2, 5, 8 and 9 with rounds of 5, 4 and 3 tiles."""
import ctypes
import functools

import numpy as np
import pytest

import adaptive_ref as A
import ptamd
import scenes
from support import bits, read_device, renderer, same, scene

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 72, 40
PARAMS = (2, 9, 3, 0.5, 1.5)
MOMENTS = [(ptamd.PT_OPT_MOMENTS, 1)]
ON = [(ptamd.PT_OPT_ADAPTIVE_WF, 1)]
UNSUPPORTED, INVALID = -5, -1

SCENES = {
    "box": lambda: (scene("box"), scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT),
    "sphere": lambda: (scene("sphere"), scenes.camera((3, 2, 4)), scenes.REFERENCE_LIGHT),
}


def _renderer(name="box", options=(), size=(W, H)):
    sc, cam, lights = SCENES[name]()
    return renderer(sc, cam, lights, size=size, options=MOMENTS + list(options))


@functools.lru_cache(maxsize=None)
def uniform(name="box", base=0, size=(W, H)):
    """count -> (accumulator (h, w, 4), moments (h, w, 2)) of pt_render(0, count) for every count of the schedule,
    on the default kernel path with the option off.  Rendered once per scene, seed base and size; read-only."""
    w, h = size
    r = _renderer(name, [(ptamd.PT_OPT_SEED_BASE, base)], size)
    out = {}
    for n in A.schedule(PARAMS):
        r.clear()
        r.render(0, n)
        assert r.last_kernel() == ptamd.KERNEL_RECURSIVE
        acc = r.read_accum().reshape(h, w, 4)
        mom, got_n = r.read_moments()
        assert got_n == n
        acc.setflags(write=False)
        mom.setflags(write=False)
        out[n] = (acc, mom)
    return out


def _accs(*key):
    return {n: a for n, (a, _) in uniform(*key).items()}


def _moms(*key):
    return {n: m for n, (_, m) in uniform(*key).items()}


def run(r, size=(W, H)):
    """An adaptive render to its end: (counts (by, bx), accumulator, moments)."""
    w, h = size
    r.adaptive_begin(PARAMS)
    assert r.last_kernel() == ptamd.KERNEL_WAVEFRONT
    r.adaptive_advance(100)
    counts, _ = r.adaptive_counts()
    acc = r.read_accum().reshape(h, w, 4)
    mom, n = r.read_moments()
    assert n == 0, "the moments of an adaptive render have no single n"
    return counts, acc, mom


def check_composition(counts, acc, mom, name="box", base=0, size=(W, H), what=""):
    w, h = size
    same(acc, A.compose(_accs(name, base, size), counts, w, h), f"{what}: accumulator")
    same(mom, A.compose(_moms(name, base, size), counts, w, h), f"{what}: moments")


def check_rounds(r, name, what):
    """Round by round: the live list is the simulation's, ascending, and its batches are the pair the host gave
    the round's launch (every live entry of a round holds the same one); the counts follow."""
    bx, by = A.tiles(W, H)
    lo, hi, step = PARAMS[:3]
    want, lives = A.simulate(_moms(name), W, H, PARAMS)
    r.adaptive_begin(PARAMS)
    first = r.adaptive_live()
    assert [tuple(e) for e in first] == [((b % bx) * 16, (b // bx) * 16, 0, lo) for b in range(bx * by)], what
    for k, live in enumerate(lives):
        r.adaptive_advance(1)
        host = (lo + k * step, min(step, hi - (lo + k * step)))   # launch_round's {first_batch, n_batches} of round k + 1
        got = [tuple(int(v) for v in e) for e in r.adaptive_live()]
        assert got == [((b % bx) * 16, (b // bx) * 16, fb, nb) for b, fb, nb in live], (what, k, got, live)
        assert all(e[2:] == host for e in got), (what, k, got, host)
        done, n_live, _ = r.adaptive_info()
        assert done == k + 1 and n_live == (len(live) if k + 1 < len(lives) else 0)
        sim_counts, _ = A.simulate(_moms(name), W, H, PARAMS, rounds=k + 1)
        assert np.array_equal(r.adaptive_counts()[0].reshape(-1), sim_counts), (what, k)
    counts, _ = r.adaptive_counts()
    assert np.array_equal(counts.reshape(-1), want), (what, counts, want.reshape(by, bx))
    acc = r.read_accum().reshape(H, W, 4)
    check_composition(counts, acc, r.read_moments()[0], name, what=what)
    distinct = set(int(n) for n in counts.reshape(-1))
    assert len(distinct) >= 3 and lo in distinct and hi in distinct, f"{what}: counts {sorted(distinct)}"
    assert any(len(l) not in (0, bx * by) for l in lives), f"{what}: some round must list a part of the tiles"
    return counts, lives


DEVICE = [(ptamd.PT_OPT_SCENE_IN_LDS, 0)]
FORMS = {
    "threaded walk from LDS": [],
    "threaded walk from device memory": DEVICE + [(ptamd.PT_OPT_WIDE, 0)],
    "wide walk": DEVICE,
    "hand-back": DEVICE + [(ptamd.PT_OPT_WIDE, 2)],
    "128-B nodes": DEVICE + [(ptamd.PT_OPT_WIDE_NODE, 128)],
    "no fused shadow walks": DEVICE + [(ptamd.PT_OPT_WF_FUSE, 0)],
    "tail never": DEVICE + [(ptamd.PT_OPT_WF_TAIL, 0)],
    "tail always": DEVICE + [(ptamd.PT_OPT_WF_TAIL, 2**31 - 1)],
    "exit skip 0": DEVICE + [(ptamd.PT_OPT_EXIT_SKIP, 0)],
    "exit skip 1": DEVICE + [(ptamd.PT_OPT_EXIT_SKIP, 1)],
    "primary cull off": [(ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "tight cull off": [(ptamd.PT_OPT_CULL_TIGHT, 0)],
    "primary cull off, wide walk": DEVICE + [(ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "PT_OPT_KERNEL 3": [(ptamd.PT_OPT_KERNEL, 3)],
}


@pytest.mark.parametrize("form", list(FORMS))
def test_box_on_every_wavefront_form(form):
    r = _renderer("box", ON + FORMS[form])
    if DEVICE[0] in FORMS[form] and (ptamd.PT_OPT_WIDE, 0) not in FORMS[form]:
        assert r.wide_info()[0] > 0, "a wide tree must be in force"
    counts, lives = check_rounds(r, "box", form)
    assert sorted(set(counts.reshape(-1).tolist())) == [2, 8, 9]


def test_seed_base():
    base = 12345
    counts, acc, mom = run(_renderer("box", ON + DEVICE + [(ptamd.PT_OPT_SEED_BASE, base)]))
    check_composition(counts, acc, mom, base=base, what=f"seed base {base}")
    assert not np.array_equal(bits(acc), bits(A.compose(_accs(), counts, W, H)))   # another base, another frame


@pytest.mark.parametrize("paths", [3840, 7680])
@pytest.mark.parametrize("wide", [0, 1])
def test_chunking(paths, wide):
    """PT_OPT_WF_PATHS 3840 = 15 tiles x 256: one batch per chunk; 7680: chunks of 2 + 1 batches in a step of 3."""
    r = _renderer("box", ON + [(ptamd.PT_OPT_WF_PATHS, paths)] + (DEVICE if wide else []))
    counts, acc, mom = run(r)
    assert np.array_equal(counts.reshape(-1), A.simulate(_moms(), W, H, PARAMS)[0])
    check_composition(counts, acc, mom, what=f"{paths} paths per chunk")


def test_sphere_on_the_wide_walk():
    r = _renderer("sphere", ON)
    assert r.wide_info()[0] > 0
    counts, lives = check_rounds(r, "sphere", "sphere")
    print("\nsphere counts:\n", counts, "\nlive tiles per round:", [len(l) for l in lives])
    assert sorted(set(counts.reshape(-1).tolist())) == [2, 5, 8, 9]
    assert [len(l) for l in lives] == [5, 4, 3]


def test_slots_outside_the_frame():
    """17x17: four tiles, three of them one pixel wide or high."""
    size = (17, 17)
    for options in ([], DEVICE):
        counts, acc, mom = run(_renderer("box", ON + options, size), size)
        check_composition(counts, acc, mom, size=size, what=f"17x17 {options}")


def _begin_code(r, params=PARAMS):
    p = ptamd.AdaptiveParams(*params)
    return ptamd.lib().pt_adaptive_begin(r._c, ctypes.byref(p))


def test_last_kernel_and_the_option():
    L = ptamd.lib()
    for kernel, want in [(0, ptamd.KERNEL_WAVEFRONT), (3, ptamd.KERNEL_WAVEFRONT), (1, ptamd.KERNEL_RECURSIVE)]:
        r = _renderer("box", ON + [(ptamd.PT_OPT_KERNEL, kernel)])
        r.adaptive_begin(PARAMS)
        assert r.last_kernel() == want, kernel
        r.adaptive_advance(100)
        counts, _ = r.adaptive_counts()
        check_composition(counts, r.read_accum().reshape(H, W, 4), r.read_moments()[0], what=f"PT_OPT_KERNEL {kernel}")
    r = _renderer()
    for bad in (2, -1):
        assert L.pt_set_option(r._c, ptamd.PT_OPT_ADAPTIVE_WF, bad) == INVALID
        assert b"PT_OPT_ADAPTIVE_WF" in L.pt_last_error()
    # off again: PT_OPT_KERNEL 3 is refused as before, and auto runs the path-recursive kernel
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, 1)
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, 0)
    r.adaptive_begin(PARAMS)
    assert r.last_kernel() == ptamd.KERNEL_RECURSIVE
    r.set_option(ptamd.PT_OPT_KERNEL, 3)
    assert _begin_code(r) == UNSUPPORTED and b"PT_OPT_KERNEL 3" in L.pt_last_error()


def test_the_option_can_change_between_rounds():
    """pt_adaptive_advance plans again per call: rounds of both kinds in one render, the same bits."""
    r = _renderer("box", DEVICE)
    r.adaptive_begin(PARAMS)                       # round 0 path-recursive
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, 1)
    r.adaptive_advance(2)                          # two rounds on the wavefront pipeline
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, 0)
    r.adaptive_advance(100)
    counts, _ = r.adaptive_counts()
    assert np.array_equal(counts.reshape(-1), A.simulate(_moms(), W, H, PARAMS)[0])
    check_composition(counts, r.read_accum().reshape(H, W, 4), r.read_moments()[0], what="mixed rounds")


def test_refusals():
    L = ptamd.lib()
    sc, cam, lights = SCENES["box"]()
    cases = {
        "partition": lambda r: r.set_partition(2, 0),
        "stats": lambda r: r.set_stats_mode(True),
        "counting": lambda r: r.set_option(ptamd.PT_OPT_COUNT_TRACED, 1),
    }
    for name, set_up in cases.items():
        r = _renderer("box", ON)
        set_up(r)
        assert _begin_code(r) == UNSUPPORTED, name
        assert b"adaptive" in L.pt_last_error(), name
        assert L.pt_adaptive_advance(r._c, 1) == INVALID, name
    g = ptamd.Renderer(devices=[0, 0])
    g.set_option(ptamd.PT_OPT_ADAPTIVE_WF, 1)
    assert _begin_code(g) == UNSUPPORTED and L.pt_adaptive_advance(g._c, 1) == UNSUPPORTED
    r = renderer(sc, cam, lights, size=(W, H), options=ON)             # PT_OPT_MOMENTS 0
    assert _begin_code(r) == INVALID and b"PT_OPT_MOMENTS" in L.pt_last_error()
    r = _renderer("box", ON)
    for bad in [(1, 9, 3, 0.5, 0.01), (4, 3, 3, 0.5, 0.01), (2, 9, 0, 0.5, 0.01), (2, 9, 3, float("nan"), 0.01)]:
        assert _begin_code(r, bad) == INVALID, bad


def test_state():
    r = _renderer("box", ON + DEVICE)
    counts, acc, mom = run(r)
    r.adaptive_advance(5)                                             # past the last round nothing changes
    assert np.array_equal(counts, r.adaptive_counts()[0]) and r.adaptive_info()[0] == 3
    same(r.read_accum(), acc, "advance past the last round: accumulator")
    same(r.read_moments()[0], mom, "advance past the last round: moments")
    # an ordinary render afterwards is the ordinary frame, and ends the state
    r.render(0, 5)
    same(r.read_accum(), _accs()[5], "pt_render(0, 5) after a wavefront adaptive render")
    m5, n5 = r.read_moments()
    assert n5 == 5
    same(m5, _moms()[5], "its moments")
    assert ptamd.lib().pt_adaptive_advance(r._c, 1) == INVALID
    # ... on the wavefront pipeline too, which shares the path buffers with the rounds
    r.set_option(ptamd.PT_OPT_KERNEL, 3)
    run(r)
    r.render(0, 8)
    assert r.last_kernel() == ptamd.KERNEL_WAVEFRONT
    same(r.read_accum(), _accs()[8], "a wavefront pt_render(0, 8) after a wavefront adaptive render")
    # and a new begin starts over: the same result
    counts3, acc3, mom3 = run(r)
    assert np.array_equal(counts3, counts)
    same(acc3, acc, "a second adaptive render")
    same(mom3, mom, "its moments")


def test_denoise():
    r = _renderer("box", ON + DEVICE)
    counts, acc, mom = run(r)
    check_composition(counts, acc, mom, what="before the filter")
    got = r.adaptive_denoise()
    guide = r.read_guide()
    n_px = np.repeat(np.repeat(counts, 16, 0), 16, 1)[:H, :W].astype(np.uint32)
    with np.errstate(all="ignore"):
        var = (np.fmax(F(0), mom[..., 1] - mom[..., 0] * mom[..., 0]) / (n_px - np.uint32(1)).astype(F)).astype(F)
    same(read_device(r, r.adaptive_ptr(2), (H, W)), var, "the variance plane")
    same(got, ptamd.denoise_var_plane_host(acc, var, guide, W, H), "adaptive_denoise against the host's passes")
    assert not np.array_equal(bits(got), bits(acc))
    same(r.read_accum(), acc, "the filter leaves the accumulator")
