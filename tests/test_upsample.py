"""Host side of guide-driven upsampling, without a GPU: pt_upsample_host (the
header code the kernels compile, csrc/pt_upsample.h upsample_pixel) against the
independent numpy-float32 restatement of tests/upsample_ref.py, bit for bit, on
seeded and on hostile images; the lattice identity; hits and misses that do not
mix; the fallback; the guide-ray identity the lattice argument rests on; the
defaults and the refusals."""
import ctypes

import numpy as np
import pytest

import oracle_lib
import ptamd
import scenes
import temporal_ref as T
import upsample_ref as U
from support import same, same_nan

PT_OK, PT_ERR_INVALID = 0, -1
F = np.float32
SYMBOLS = ("pt_upsample_default_params", "pt_upsample_host", "pt_upsample_images", "pt_upsample",
           "pt_upsampled_device_ptr", "pt_read_upsampled", "pt_upsample_guide_device_ptr", "pt_upsample_info",
           "pt_upsample_display", "pt_display_upsampled_device_ptr", "pt_read_display_upsampled")


def test_symbols_and_defaults():
    L = ptamd.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in ptamd.EXPORTS
    assert L.pt_abi_version() == 3
    p = ptamd.upsample_default_params()
    assert (p.scale, p.sigma_normal, p.sigma_depth) == (2, F(0.35), F(0.25))
    assert (p.scale, F(p.sigma_normal), F(p.sigma_depth)) == (U.DEFAULTS[0], F(U.DEFAULTS[1]), F(U.DEFAULTS[2]))
    assert L.pt_upsample_default_params(None) == PT_ERR_INVALID


@pytest.mark.parametrize("w,h,s", U.SHAPES)
def test_host_matches_restatement(w, h, s):
    rgba, guide, ref = U.seeded(w, h, s)
    got = ptamd.upsample_host(rgba, w, h, guide, s)               # the default sigmas at scale s
    assert got.shape == (s * h, s * w, 4) and np.all(np.isfinite(got))
    same(got, ref, f"{w}x{h} at scale {s}")
    same(ptamd.upsample_host(rgba, w, h, guide, (s, 0.35, 0.25)), ref, "the defaults spelt out")
    for params in ((s, 1.0, 0.5), (s, 0.05, 4.0)):
        same(ptamd.upsample_host(rgba, w, h, guide, params), U.upsample(rgba, guide, w, h, params), f"{w}x{h} {params}")
    same(got[..., 3], np.repeat(np.repeat(rgba[..., 3], s, 0), s, 1), "alpha is the cell's own")


@pytest.mark.parametrize("kind", ["extremes", "nonfinite"])
def test_host_matches_restatement_on_hostile_images(kind):
    n = 0
    for w, h, seed, plane in U.hostile_cases(kind):
        color, guide = U.hostile_images(kind, w, h, seed, plane)
        got = ptamd.upsample_host(color, w, h, guide, U.HOSTILE_SCALE)
        same_nan(got, U.hostile_reference(kind, w, h, seed, plane), f"{kind} {w}x{h} seed {seed} plane {plane}")
        n += 1
    assert n >= 20


def test_exp_of_minus_zero_is_one():
    """What the lattice identity rests on: the tap of a pixel with itself has the argument -0."""
    assert oracle_lib.math(1, np.array([-0.0, 0.0], F)).view(np.uint32).tolist() == [0x3f800000, 0x3f800000]


@pytest.mark.parametrize("w,h,s", U.SHAPES)
def test_lattice_identity(w, h, s):
    rgba, guide, _ = U.seeded(w, h, s)
    got = ptamd.upsample_host(rgba, w, h, guide, s)
    assert np.array_equal(got[::s, ::s], rgba)                    # in value
    # a cleared frame: -0 may come out +0, nothing else
    zero = np.full((h, w, 4), -0.0, F)
    assert not ptamd.upsample_host(zero, w, h, guide, s)[..., :3].any()
    # the hostile colours too, where they are finite: a non-finite neighbour does not reach a lattice point
    color = U.hostile_images("nonfinite", w, h, 3, "color")[0]
    fin = np.all(np.isfinite(color[..., :3]), axis=-1)
    assert w * h == 1 or not fin.all()
    out = ptamd.upsample_host(color, w, h, guide, s)[::s, ::s]
    assert np.array_equal(out[fin], color[fin])


@pytest.mark.parametrize("w,h,s", [(16, 12, 2), (16, 12, 4), (17, 12, 4), (9, 5, 3)])
def test_edges_do_not_mix(w, h, s):
    src, guide, miss = U.edge_images(w, h, s)
    assert miss.any() and not miss.all() and miss[::s, ::s].any()
    got = ptamd.upsample_host(src, w, h, guide, s)
    want = np.where(miss, F(4.0), F(0.25))
    wrong = int(np.count_nonzero(got[..., :3] != want[..., None]))
    assert wrong == 0, f"{wrong} channels are neither their own side's colour"
    ref, fell = U.upsample(src, guide, w, h, (s, 0.35, 0.25), fallbacks=True)
    assert not fell.any()                                         # every pixel found a tap of its own kind
    same(got, ref, "the restatement")


def test_fallback():
    w, h, s = 4, 3, 4
    rng = np.random.default_rng(5)
    src = rng.uniform(0.5, 2.0, (h, w, 4)).astype(F)
    guide = np.tile(U.MISS, (s * h, s * w, 1))
    X, Y = 6, 5                                                   # off the lattice, its four taps misses
    guide[Y, X] = np.array([0.0, 0.0, 1.0, 3.0], F)
    got = ptamd.upsample_host(src, w, h, guide, s)
    same(got[Y, X], src[Y // s, X // s], "a hit pixel among misses takes its cell's pixel")
    ref, fell = U.upsample(src, guide, w, h, (s, 0.35, 0.25), fallbacks=True)
    assert fell[Y, X] and np.count_nonzero(fell) == 1
    same(got, ref, "the restatement")
    # a pixel whose own guide holds NaN: every weight and the sum are NaN
    guide = U.make_images(w, h, s, 9)[1]
    for k in range(4):
        g = guide.copy()
        g[Y, X, k] = np.nan
        got = ptamd.upsample_host(src, w, h, g, s)
        same(got[Y, X], src[Y // s, X // s], f"NaN in guide component {k}")
        assert np.all(np.isfinite(got))


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_guide_ray_identity(s):
    """The premise of the lattice argument: pixel (i, j) of the w x h frame and pixel (s*i, s*j) of the
    (s*w) x (s*h) frame have the same guide ray, bit for bit."""
    w, h = 37, 23
    for cam in (scenes.DEFAULT_CAMERA, T.rotate_y(scenes.DEFAULT_CAMERA, 17.0)):
        for j in range(h):
            for i in range(w):
                o, d = ptamd.guide_ray(cam, w, h, i, j)
                O, D = ptamd.guide_ray(cam, s * w, s * h, s * i, s * j)
                assert o.tobytes() == O.tobytes() and d.tobytes() == D.tobytes(), (s, i, j)


def test_refusals():
    L = ptamd.lib()
    w, h, s = 3, 2, 2
    src = np.ones(w * h * 4, F)
    guide = np.ones(w * h * s * s * 4, F)
    out = np.zeros(guide.size, F)

    def call(params=None, w=w, h=h, **over):
        a = {"src": src.ctypes.data, "guide": guide.ctypes.data, "out": out.ctypes.data}
        a.update(over)
        p = None if params is None else ctypes.byref(ptamd.UpsampleParams(*params))
        return L.pt_upsample_host(a["src"], w, h, a["guide"], p, a["out"])

    assert call() == PT_OK and call(params=(2, 0.35, 0.25)) == PT_OK
    for k in ("src", "guide", "out"):
        assert call(**{k: None}) == PT_ERR_INVALID, k
    for bad_w, bad_h in [(0, 2), (3, 0), (-1, 2)]:
        assert call(w=bad_w, h=bad_h) == PT_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    for bad in [(1, 0.35, 0.25), (0, 0.35, 0.25), (-2, 0.35, 0.25), (9, 0.35, 0.25),
                (2, 0.0, 0.25), (2, -1.0, 0.25), (2, inf, 0.25), (2, nan, 0.25), (2, 1e-30, 0.25), (2, 1e30, 0.25),
                (2, 0.35, 0.0), (2, 0.35, -1.0), (2, 0.35, inf), (2, 0.35, nan), (2, 0.35, 1e-30), (2, 0.35, 1e30)]:
        assert call(params=bad) == PT_ERR_INVALID, bad
    assert call(params=(2, 1e-18, 1e18)) == PT_OK
    # W * H beyond 2^31 pixels: refused before an image is read
    assert call(w=32768, h=32768) == PT_ERR_INVALID                       # 2^32 at scale 2
    assert call(params=(8, 0.35, 0.25), w=8192, h=8192) == PT_ERR_INVALID    # 2^32 at scale 8
    with pytest.raises(ptamd.PTError):
        ptamd.upsample_host(src[:-4], w, h, guide)
    # a 1x1 source is valid at every scale
    # a 1x1 source is valid at every scale: its one pixel everywhere, (wt * c) / wt being c to a rounding
    pixel = np.array([1.0, 2.0, 3.0, 0.5], F)
    for s1 in range(2, 9):
        flat = np.tile(U.MISS, (s1, s1, 1))
        one = ptamd.upsample_host(pixel, 1, 1, flat, s1)
        assert one.shape == (s1, s1, 4) and np.allclose(one, pixel, rtol=2.0 ** -22, atol=0)
        same(one, U.upsample(pixel, flat, 1, 1, (s1, 0.35, 0.25)), f"1x1 at scale {s1}")
