"""The kernels downstream of the render on extreme and non-finite images,
without a GPU: every host function (the header code the kernels compile,
csrc/pt_denoise.h) against its numpy restatement on the image sets of
tests/hostile_images.py -- NaN where NaN, every other float bitwise
(support.same_nan) -- and known answers that pin the statement's behaviour at
NaN and infinity independently of both: the clamp of var_of_mean, what counts
as a miss for reprojection, and the footprint of one infinite colour.

fmin_/fmax_ are minNum/maxNum and every range test is written so that a NaN
fails it; the restatements say the same with np.fmin/np.fmax and comparisons.
A header whose variance clamp lets a NaN through fails
test_nan_moment_has_variance_zero and the host-against-restatement tests of the
variance filter, the reprojection and the spatial estimate; restatements that
clamp with np.maximum fail those and the adaptive rule's."""
import numpy as np
import pytest

import adaptive_ref as A
import denoise_ref as D
import denoise_var_ref as V
import hostile_images as X
import ptamd
import spatial_var_ref as S
import temporal_ref as T
from support import bits, same, same_nan
from test_temporal import CAMERAS, CUR

F = np.float32
KINDS = ("extremes", "nonfinite")
SIZES = X.TINY + X.BIG
REPROJECT_PARAMS = (None, (8, 0.25, 0.9, 0.02))
SPATIAL_PARAMS = [(4, 1, 0.5, 0.25), (65536, 2, 1.0, 1.0), (3, 3, 0.25, 1.0)]     # radii 1-3; 65536: every finite length
ADAPTIVE_PARAMS = (2, 9, 3, 0.25, 0.0625)
# the (plane, passes) of nonfinite() a one- or two-tile frame cannot run: three passes reach 14 pixels
SPREAD = {"atrous": ("color", "normal", "t", "all"), "var": ("color", "normal", "t", "all"),
          "plane": ("color", "variance", "normal", "t", "all")}


# ---- the generators -----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_generators_hold_every_case(W, H):
    have = set()
    for seed in X.seeds("extremes", W, H):
        d = X.images("extremes", W, H, seed)
        assert all(np.all(np.isfinite(a)) for a in d.values() if isinstance(a, np.ndarray))
        have |= X.holds(d)
    want = set(X.EXTREME_CASES) | (set(X.BESIDE_CASES) if W * H > 1 else set()) | (set(X.STRIP_CASES) if (W, H) in X.BIG else set())
    assert want <= have, sorted(want - have)
    for plane in X.PLANES:
        have = set()
        for seed in X.seeds("nonfinite", W, H):
            have |= X.holds(X.images("nonfinite", W, H, seed, plane))
            both = X.holds(X.images("nonfinite", W, H, seed, "all"))
            assert {h for h in have if ":" in h and not h.startswith(plane)} == set(), "one plane at a time"
            assert all(any(h.startswith(p + ":") for h in both) for p in X.PLANES), "all together"
        assert {f"{plane}: {s}" for s in X.SPECIAL_NAMES} <= have, (plane, sorted(have))


def test_the_cases_that_are_not_run():
    """A case of a 16x16-or-larger frame runs only if at least half of every
    output plane is not NaN in the restatement's result.  All of extremes()
    does; of nonfinite() three passes of a plane whose seeds spread do not fit
    a frame of one tile (the footprint of k passes reaches 2 (2^k - 1) = 14
    pixels) and are left to the 37x23 frame."""
    for op in ("atrous", "var", "plane"):
        for kind in KINDS:
            for W, H in X.BIG:
                every = {(s, p, k) for s in X.seeds(kind, W, H) for p in X.planes(kind) for k in X.PASSES[kind]}
                left = {(p, k) for _, p, k in every - set(X.filter_cases(op, kind, W, H))}
                want = {(p, 3) for p in SPREAD[op]} if kind == "nonfinite" and W < 32 else set()
                assert left == want, (op, kind, W, H, sorted(left))


# ---- host against restatement -------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_filters_match_their_restatements(kind, W, H):
    n_run = 0
    for op in ("atrous", "var", "plane"):
        for seed, plane, k in X.filter_cases(op, kind, W, H):
            d = X.images(kind, W, H, seed, plane)
            ref = X.reference(op, kind, W, H, seed, plane, k)
            if op == "atrous":
                got = ptamd.denoise_host(d["color"], d["guide"], W, H, X.denoise_params(k))
            elif op == "var":
                got = ptamd.denoise_var_host(d["color"], d["moments"], X.N_SAMPLES, d["guide"], W, H, X.var_params(k))
            else:
                got = ptamd.denoise_var_plane_host(d["color"], d["variance"], d["guide"], W, H, X.var_params(k))
            same_nan(got, ref, f"{op} {kind} {W}x{H} seed {seed} {plane}, {k} passes")
            same(got[..., 3], d["color"][..., 3], "alpha passes through")
            assert (W, H) in X.TINY or X.enough(ref)
            if kind == "extremes":
                assert np.isfinite(got[..., :3]).any() or W * H == 1
            n_run += 1
    assert n_run >= 3 * len(X.PASSES[kind])


@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_reprojection_matches_its_restatement(kind, W, H, cam):
    prev = CAMERAS[cam][0]
    blended = 0
    for seed in X.seeds(kind, W, H):
        for plane in (X.planes(kind) if cam == "orbit2" else ("all",)):
            d = X.images(kind, W, H, seed, plane, X.cam_key(CUR, prev))
            for hist in (X.history(d), None):
                for params in REPROJECT_PARAMS:
                    got = ptamd.reproject_host(CUR, prev, W, H, 2, d["color"], d["moments"], d["guide"], hist, params)
                    *ref, info = T.reproject(CUR, prev, W, H, 2, d["color"], d["moments"], d["guide"], hist,
                                             T.DEFAULTS if params is None else params)
                    for g, r, what in zip(got, ref, ("colour", "moments", "length", "variance")):
                        same_nan(g, r, f"{kind} {cam} {W}x{H} seed {seed} {plane} {params}: {what}")
                    assert (W, H) in X.TINY or X.enough(*ref)
                    blended += info["blended"]
    assert blended > 0 or cam == "away" or (W, H) in X.TINY


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_spatial_variance_matches_its_restatement(kind, W, H):
    for seed in X.seeds(kind, W, H):
        for plane in X.planes(kind):
            d = X.images(kind, W, H, seed, plane)
            ins = [d[k] for k in ("moments", "length", "variance", "guide")]
            for params in SPATIAL_PARAMS:
                ref = S.spatial_variance(*ins, W, H, params)
                same_nan(ptamd.spatial_variance_host(*ins, W, H, params), ref, f"{kind} {W}x{H} seed {seed} {plane} {params}")
                assert (W, H) in X.TINY or X.enough(ref)


def adaptive_counts(W, H, seed):
    bx, by = A.tiles(W, H)
    return np.random.default_rng(seed).integers(2, 10, bx * by).astype(np.uint32)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_rule_matches_its_restatement(kind, W, H):
    for seed in X.seeds(kind, W, H):
        d = X.images(kind, W, H, seed, "moments" if kind == "nonfinite" else "all")
        counts = adaptive_counts(W, H, seed)
        nxt, err = ptamd.adaptive_select_host(d["moments"], counts, W, H, ADAPTIVE_PARAMS)
        want_n, want_e = A.select(d["moments"], counts, W, H, ADAPTIVE_PARAMS)
        assert np.array_equal(nxt, want_n), (kind, W, H, seed)
        same(err, want_e, f"{kind} {W}x{H} seed {seed}: errors")       # never NaN: a NaN moment gives +inf
        assert not np.isnan(err).any()


def test_exp_edges_through_the_spatial_estimate():
    """exp_ of the header against the oracle's where the filters can take it:
    arguments -(dz * dz) across the subnormal results (-87.3 .. -103.97), below
    them (+0), -inf and NaN.  A 2x1 frame, sigma 1: pixel 0 taps pixel 1 with
    w = exp(-dz^2) * 2^100 beside a centre weight of 2^-40, so a subnormal exp decides the sums' bits."""
    args = np.concatenate([np.linspace(87.0, 104.5, 400), [103.97208, 103.9720840454, 103.972092, 110.0, 1e30]])
    for a in args:
        t1 = F(np.sqrt(a))
        m = np.array([[[0.5, 0.5], [3.0, 16.0]]], F)
        l = np.array([[2.0 ** -40, 2.0 ** 100]], F)                    # the centre weighs 2^-40, the tap 2^-50 .. 2^-27
        g = np.array([[[0, 0, 1, 0.0], [0, 0, 1, t1]]], F)
        v = np.zeros((1, 2), F)
        p = (65536, 1, 1.0, 1.0)
        same_nan(ptamd.spatial_variance_host(m, l, v, g, 2, 1, p), S.spatial_variance(m, l, v, g, 2, 1, p), f"dz^2 = {a}")
    for t1 in (np.inf, -np.inf, np.nan):
        g[0, 1, 3] = t1
        same_nan(ptamd.spatial_variance_host(m, l, v, g, 2, 1, p), S.spatial_variance(m, l, v, g, 2, 1, p), f"t = {t1}")


# ---- known answers ------------------------------------------------------------------------------
def _flat(W, H, colour=(0.25, 0.5, 0.75, 1.0)):
    rgba = np.empty((H, W, 4), F)
    rgba[...] = np.array(colour, F)
    guide = np.empty((H, W, 4), F)
    guide[...] = np.array([0.0, 0.0, 1.0, 3.0], F)
    return rgba, guide


@pytest.mark.parametrize("special", [float("nan"), -float("nan")])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_nan_moment_has_variance_zero(which, special):
    """var_of_mean's fmax_(0, NaN) is 0.  The statement's out_var shows it
    directly; the variance filter gives the image of a pixel whose moments have
    no variance at all."""
    W, H = 9, 7
    d = X.ordinary(W, H, 3)
    m = d["moments"].copy()
    m[3, 4, [0, 1] if which == 2 else which] = F(special)
    var = ptamd.reproject_host(CUR, CUR, W, H, 2, d["color"], m, d["guide"], None)[3]
    assert bits(var)[3, 4] == 0 and np.all(np.isfinite(var))
    zero = d["moments"].copy()
    zero[3, 4] = (1.0, 1.0)                                            # m2 == m1 * m1: variance +0
    for k in (1, 3):
        got = ptamd.denoise_var_host(d["color"], m, 2, d["guide"], W, H, X.var_params(k))
        assert np.all(np.isfinite(got))
        same(got, ptamd.denoise_var_host(d["color"], zero, 2, d["guide"], W, H, X.var_params(k)), f"{k} passes")
    sv = ptamd.spatial_variance_host(m, np.ones((H, W), F), np.zeros((H, W), F), d["guide"], W, H, (2, 1, 1.0, 1.0))
    assert bits(sv)[3, 4] == 0                                         # fmax_(0, NaN) / 1


def test_nan_moment_never_converges():
    """The clamp would make a NaN pixel's error 0: finite_p keeps it, and an
    infinite moment, from counting as converged at any count."""
    W, H = 16, 16
    for special, where in ((np.nan, 0), (np.nan, 1), (np.inf, 0), (np.inf, 1), (-np.inf, 0), (-np.inf, 1)):
        m = np.zeros((H, W, 2), F)
        nxt, err = ptamd.adaptive_select_host(m, np.array([2], np.uint32), W, H, ADAPTIVE_PARAMS)
        assert nxt[0] == 2 and bits(err)[0] == 0                       # all zero: converged at once
        m[5, 7, where] = special
        for n, want in ((2, 5), (8, 9), (9, 9)):
            nxt, err = ptamd.adaptive_select_host(m, np.array([n], np.uint32), W, H, ADAPTIVE_PARAMS)
            assert nxt[0] == want and err[0] == np.inf, (special, where, n)


@pytest.mark.parametrize("t", [float("nan"), 1e30, 3.0e38, float("inf"), -float("nan")])
def test_a_guide_depth_that_is_nan_or_a_miss_takes_the_new_frame(t):
    W, H, n = 9, 7, 2
    d = X.ordinary(W, H, 5, (CUR, CUR))
    g = d["guide"].copy()
    g[2, 3, 3] = g[4, 8, 3] = F(t)
    c, m, l, v = ptamd.reproject_host(CUR, CUR, W, H, n, d["color"], d["moments"], g, X.history(d))
    assert np.count_nonzero(l > n) >= W * H // 2                       # the others found their history
    for y, x in ((2, 3), (4, 8)):
        same(c[y, x], d["color"][y, x], "colour")
        same(m[y, x], d["moments"][y, x], "moments")
        assert l[y, x] == F(n)
    # the same depth in the history: that tap is not valid, nothing of it reaches the output
    hg = d["hguide"].copy()
    hg[2, 3, 3] = F(t)
    out = ptamd.reproject_host(CUR, CUR, W, H, n, d["color"], d["moments"], d["guide"], (d["hcolor"], d["hmoments"], d["length"], hg))
    assert all(np.all(np.isfinite(o)) for o in out)


@pytest.mark.parametrize("entry", [0, 1, 2, 4, 5, 6, 8, 9, 10, 12])
def test_nan_camera_entries_give_no_history(entry):
    W, H, n = 9, 7, 3
    d = X.ordinary(W, H, 7, (CUR, CUR))
    for which in (0, 1):
        cams = [np.array(CUR, F), np.array(CUR, F)]
        cams[which][entry] = np.nan
        c, m, l, v = ptamd.reproject_host(cams[0], cams[1], W, H, n, d["color"], d["moments"], d["guide"], X.history(d))
        same(c, d["color"], f"camera {which} entry {entry}: colour")
        same(m, d["moments"], "moments")
        assert np.all(l == F(n))
        same(v, ptamd.reproject_host(CUR, CUR, W, H, n, d["color"], d["moments"], d["guide"], None)[3], "variance")


@pytest.mark.parametrize("filt", ["atrous", "var"])
@pytest.mark.parametrize("special", [float("inf"), -float("inf")])
def test_the_footprint_of_one_infinite_colour(filt, special):
    """One pixel of infinite colour in a constant image: a tap on it weighs 0 and
    adds 0 * inf = NaN, so one pass turns exactly the 25 pixels that tap it into
    NaN (the pixel itself through inf - inf), k passes the block of 2 (2^k - 1)
    pixels to every side: 25, 169, 841.  Alpha is never touched.  This pins the
    behaviour; DESIGN.md section 9 lists skipping zero-weight taps as open."""
    W = H = 33
    rgba, guide = _flat(W, H)
    rgba[16, 16, :3] = F(special)
    moments = np.empty((H, W, 2), F)
    moments[...] = np.array([0.5, 0.3], F)
    flat = _flat(W, H)[0]
    clean = lambda k: (ptamd.denoise_host(flat, guide, W, H, X.denoise_params(k)) if filt == "atrous" else
                       ptamd.denoise_var_host(flat, moments, 2, guide, W, H, X.var_params(k)))
    for k in (1, 2, 3):
        if filt == "atrous":
            got = ptamd.denoise_host(rgba, guide, W, H, X.denoise_params(k))
            ref = D.atrous(rgba, guide, W, H, X.denoise_params(k))
        else:
            got = ptamd.denoise_var_host(rgba, moments, 2, guide, W, H, X.var_params(k))
            ref = V.atrous_var(rgba, moments, 2, guide, W, H, X.var_params(k))
        reach = 2 * (2 ** k - 1)
        want = np.zeros((H, W), bool)
        want[16 - reach:16 + reach + 1, 16 - reach:16 + reach + 1] = True
        assert np.count_nonzero(want) == (25, 169, 841)[k - 1]
        for c in range(3):
            assert np.array_equal(np.isnan(got[..., c]), want), (k, c)
        assert np.array_equal(np.isnan(ref), np.isnan(got))            # the dilation the restatement gives
        same_nan(got, ref, f"{filt}, {k} passes")
        same(got[..., 3], rgba[..., 3], "alpha")
        same(got[~want], clean(k)[~want], "outside the footprint: the image without the infinity")
    # at the frame's corner the footprint is clipped, not wrapped
    rgba, guide = _flat(W, H)
    rgba[0, 0, :3] = F(special)
    got = ptamd.denoise_host(rgba, guide, W, H, X.denoise_params(1))
    assert np.count_nonzero(np.isnan(got[..., 0])) == 9
