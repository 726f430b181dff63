"""Seeded image sets with extreme and non-finite values for every kernel
downstream of the render (not a test module): one source of values for
tests/test_post_hostile.py and tests/test_gpu_post_hostile.py.

An image set is a dict of float32 arrays of one W x H frame:
  color (H, W, 4), moments (H, W, 2), variance (H, W), length (H, W),
  guide (H, W, 4) = {n.xyz, t}, and the history (hcolor, hmoments, length,
  hguide) of a previous camera.
The guides are the analytic ones of temporal_ref.plane_guide for the two
cameras, so that reprojection finds history for most pixels; a second normal
region and a depth step give the edge-stops something to stop at.

extremes(): every value finite, but a share of the pixels of every plane takes
+-0, subnormals (0x00000001 and 0x007fffff among them), +-FLT_MIN, negative
colours, 1e-30, 1e19, 1e30 and FLT_MAX; moments with m2 far below m1 * m1,
m2 = -0, m2 < 0 and m1 * m1 overflowing; variances 0, subnormal and FLT_MAX;
lengths 0, 1, 65536 and non-integers; guide depths 0, negative, subnormal,
9.9e29, 1e30, FLT_MAX and normals of length 0 and 1e19.  They sit among
ordinary values, so single waves mix lanes inside and outside
rcp_in_range / sqrt_in_range; in a frame of at least 16 x 8 the first 16x4
strip (one wave) is extreme in every plane and out of sqrt_'s range in its
variances, the strip below it ordinary throughout.

nonfinite(): ordinary values plus up to five isolated pixels, two apart in
one corner, of quiet NaN of both signs, a quiet NaN with a payload, +inf and
-inf -- in one plane ("color", "moments", "variance", "length", "normal",
"t") or in all of them.  The seed rotates which pixel takes which value, so a
frame too small for five pixels sees all five over five seeds.

Signalling NaNs are left out on purpose: the renderer's arithmetic cannot
produce one, and numpy and libm treat them differently from version to
version.

holds() names the cases a set contains, in the style of display_ref.holds."""
import functools

import numpy as np

import denoise_ref as D
import denoise_var_ref as V
import scenes
import temporal_ref as T

F = np.float32


def _f(u):
    return np.array([u], np.uint32).view(F)[0]


FLT_MAX, FLT_MIN = np.finfo(F).max, np.finfo(F).tiny
SUB_LO, SUB_HI = _f(0x00000001), _f(0x007fffff)
NAN_POS, NAN_NEG, NAN_PAYLOAD = 0x7fc00000, 0xffc00000, 0x7fc12345
SPECIALS = np.array([NAN_POS, NAN_NEG, NAN_PAYLOAD, 0x7f800000, 0xff800000], np.uint32).view(F)
SPECIAL_NAMES = ("nan+", "nan-", "nan payload", "+inf", "-inf")
PLANES = ("color", "moments", "variance", "length", "normal", "t")

COLOUR_POOL = np.array([0.0, -0.0, SUB_LO, -SUB_LO, SUB_HI, -SUB_HI, FLT_MIN, -FLT_MIN, -0.75, -3.0, 1e-30, 1e19,
                        -1e19, 1e30, FLT_MAX], F)
# {m1, m2}: far below m1 * m1, m2 = -0, m2 < 0, m1 * m1 overflowing (three ways), zeros, subnormals, tiny
MOMENT_POOL = np.array([[1.5, 0.25], [2.0, -0.0], [1.0, -3.0], [1e30, 1e30], [FLT_MAX, FLT_MAX], [1e19, 1e30],
                        [0.0, 0.0], [-0.0, -0.0], [SUB_LO, SUB_LO], [SUB_HI, FLT_MAX], [-1.0, 2.0], [1e-30, 1e-30],
                        [FLT_MIN, FLT_MIN]], F)
VARIANCE_POOL = np.array([0.0, -0.0, SUB_LO, SUB_HI, FLT_MIN, 1e-30, 1e30, FLT_MAX], F)
VARIANCE_OUT = VARIANCE_POOL[:6]                       # below sqrt_in_range's 2^-96
LENGTH_POOL = np.array([0.0, 1.0, 65536.0, 0.5, 2.5, 100.75], F)
DEPTH_POOL = np.array([0.0, -0.0, -2.0, SUB_LO, SUB_HI, 9.9e29, 1e30, FLT_MAX], F)
NORMAL_POOL = np.array([[0.0, 0.0, 0.0], [1e19, 0.0, 0.0], [0.0, -1e19, 1e19]], F)


def _cameras(cams):
    if cams is None:
        return scenes.DEFAULT_CAMERA, T.rotate_y(scenes.DEFAULT_CAMERA, -2.0)
    return cams


def _colours(rng, W, H):
    rgba = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    rgba[..., 3] = rng.uniform(0.5, 1.0, (H, W)).astype(F)
    m1 = V.lum(rgba)
    spread = rng.uniform(0.05, 1.5, (H, W)).astype(F)
    return rgba, np.stack([m1, m1 * m1 + spread * spread], axis=-1).astype(F)


def ordinary(W, H, seed, cams=None):
    """The benign set both generators start from: every value finite, normal,
    non-negative and small."""
    cur, prev = _cameras(cams)
    rng = np.random.default_rng(seed)
    color, moments = _colours(rng, W, H)
    hcolor, hmoments = _colours(rng, W, H)
    guide, hguide = T.plane_guide(cur, W, H), T.plane_guide(prev, W, H)
    assert np.all(guide[..., 3] < 1e30)                                 # the previous camera may see none of it
    for g in (guide, hguide):
        g[:, (3 * W) // 4:, :3] = np.array([0.6, 0.0, 0.8], F)          # second normal region
    guide[(3 * H) // 4:, :, 3] += F(0.75)                               # depth step
    return {"color": color, "moments": moments, "variance": rng.uniform(0.01, 2.0, (H, W)).astype(F),
            "length": rng.integers(1, 201, (H, W)).astype(F), "guide": guide,
            "hcolor": hcolor, "hmoments": hmoments, "hguide": hguide, "W": W, "H": H}


def history(d):
    return d["hcolor"], d["hmoments"], d["length"], d["hguide"]


def _strips(W, H):
    """(all-extreme, all-ordinary) strip slices, or None in a frame without room for them."""
    if W < 16 or H < 8:
        return None
    return (slice(0, 4), slice(0, 16)), (slice(4, 8), slice(0, 16))


TINY_PIXELS = 64                                        # below this many pixels extremes() cycles instead of drawing
TINY_SEEDS = range(len(COLOUR_POOL) + len(COLOUR_POOL) // 2 + 1)   # seeds after which a pixel has seen every pool


def extremes(W, H, seed, cams=None, share=0.3):
    """See the module docstring.  share: the fraction of extreme pixels per
    plane.  Squares and differences of these values overflow inside the filters
    (to weights of 0), their weighted means cannot.  A frame of fewer than
    TINY_PIXELS pixels has no room for every value: there pixel i of a plane
    takes entry (7 i + seed + plane) mod (L + L/2 + 1) of its pool of L values
    and stays ordinary past the pool's end, so TINY_SEEDS hold every case."""
    d = ordinary(W, H, seed, cams)
    rng = np.random.default_rng([seed, 1])
    strips = _strips(W, H)
    salt = iter(range(100))

    def fill(pool):
        """(mask of the extreme pixels, index into the pool for each of them)"""
        L = len(pool)
        if W * H < TINY_PIXELS:
            idx = ((np.arange(W * H) * 7 + seed + next(salt)) % (L + L // 2 + 1)).reshape(H, W)
            m = idx < L
            return m, idx[m]
        m = rng.uniform(size=(H, W)) < share
        if strips:
            m[strips[0]] = True
            m[strips[1]] = False
        return m, rng.integers(0, L, int(m.sum()))

    for key in ("color", "hcolor"):
        m, idx = fill(COLOUR_POOL)
        step = np.arange(3) * 5 if W * H < TINY_PIXELS else rng.integers(0, len(COLOUR_POOL), (idx.size, 3))
        vals = COLOUR_POOL[(idx[:, None] + step) % len(COLOUR_POOL)]
        d[key][m, :3] = vals
    for key in ("moments", "hmoments"):
        m, idx = fill(MOMENT_POOL)
        d[key][m] = MOMENT_POOL[idx]
    m, idx = fill(VARIANCE_POOL)
    d["variance"][m] = VARIANCE_POOL[idx]
    if strips:
        d["variance"][strips[0]] = VARIANCE_OUT[rng.integers(0, len(VARIANCE_OUT), (4, 16))]
    m, idx = fill(LENGTH_POOL)
    d["length"][m] = LENGTH_POOL[idx]
    for key in ("guide", "hguide"):
        m, idx = fill(DEPTH_POOL)
        d[key][m, 3] = DEPTH_POOL[idx]
        m, idx = fill(NORMAL_POOL)
        d[key][m, :3] = NORMAL_POOL[idx]
    for k, a in d.items():
        if isinstance(a, np.ndarray):
            assert np.all(np.isfinite(a)), k
    return d


def seed_pixels(W, H, corner=0):
    """Up to five pixels two apart in a corner (0: top left, 1: bottom right)."""
    at = [(0, 0), (2, 0), (0, 2), (2, 2), (4, 0), (0, 4), (6, 0), (0, 6), (8, 0), (0, 8)]
    at = [(x, y) for x, y in at if x < W and y < H][:5]
    return [(W - 1 - x, H - 1 - y) for x, y in at] if corner else at


def nonfinite(W, H, seed, plane="all", cams=None, corner=0):
    """See the module docstring.  plane: one of PLANES, or "all"."""
    assert plane == "all" or plane in PLANES
    d = ordinary(W, H, seed, cams)
    for j, (x, y) in enumerate(seed_pixels(W, H, corner)):
        s = SPECIALS[(seed + j) % 5]
        if plane in ("color", "all"):
            d["color"][y, x, j % 3] = s
            d["hcolor"][y, x, (j + 1) % 3] = s
        if plane in ("moments", "all"):
            d["moments"][y, x, j % 2] = s
            d["hmoments"][y, x, (j + 1) % 2] = s
        if plane in ("variance", "all"):
            d["variance"][y, x] = s
        if plane in ("length", "all"):
            d["length"][y, x] = s
        if plane in ("normal", "all"):
            d["guide"][y, x, j % 3] = s
            d["hguide"][y, x, (j + 2) % 3] = s
        if plane in ("t", "all"):
            d["guide"][y, x, 3] = s
            d["hguide"][y, x, 3] = s
    return d


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _names(what, pool):
    return tuple(f"{what} {' '.join(f'{u:#010x}' for u in _bits(p).reshape(-1))}" for p in pool)


EXTREME_CASES = (_names("colour", COLOUR_POOL) + _names("moments", MOMENT_POOL) + _names("variance", VARIANCE_POOL)
                 + _names("length", LENGTH_POOL) + _names("t", DEPTH_POOL) + _names("normal", NORMAL_POOL)
                 + ("negative colour", "m2 far below m1*m1", "m2 = -0", "m2 < 0", "m1*m1 overflows",
                    "non-integer length"))
BESIDE_CASES = ("ordinary beside extreme",)                 # frames of more than one pixel
STRIP_CASES = ("strip out of range", "strip in range")      # frames of at least 16 x 8


def holds(d):
    """The names of the cases the set d contains: EXTREME_CASES (one name per
    pool value), BESIDE_CASES and STRIP_CASES for extremes(), "<plane>:
    <special>" for nonfinite()."""
    have = set()
    W, H = d["W"], d["H"]
    c, m, v, l, g = d["color"][..., :3], d["moments"], d["variance"], d["length"], d["guide"]
    for what, a, pool in (("colour", c.reshape(-1, 1), COLOUR_POOL), ("moments", m.reshape(-1, 2), MOMENT_POOL),
                          ("variance", v.reshape(-1, 1), VARIANCE_POOL), ("length", l.reshape(-1, 1), LENGTH_POOL),
                          ("t", g[..., 3].reshape(-1, 1), DEPTH_POOL), ("normal", g[..., :3].reshape(-1, 3), NORMAL_POOL)):
        for p, name in zip(pool, _names(what, pool)):
            if np.any(np.all(_bits(a) == _bits(p).reshape(1, -1), axis=1)):
                have.add(name)
    with np.errstate(all="ignore"):
        if np.any((c < 0) & np.isfinite(c)):
            have.add("negative colour")
        m1, m2 = m[..., 0], m[..., 1]
        if np.any(m2 < F(0.5) * (m1 * m1)):
            have.add("m2 far below m1*m1")
        if np.any(_bits(m2) == 0x80000000):
            have.add("m2 = -0")
        if np.any(m2 < 0):
            have.add("m2 < 0")
        if np.any(np.isinf(m1 * m1) & np.isfinite(m1)):
            have.add("m1*m1 overflows")
        if np.any(np.isfinite(l) & (l != np.floor(l))):
            have.add("non-integer length")
        big = np.any(np.abs(c) >= F(1e19), axis=-1)
        if np.any(big) and np.any(~big):
            have.add("ordinary beside extreme")
        strips = _strips(W, H)
        if strips:
            sv = v[strips[0]]
            if np.all(~((sv >= F(2.0 ** -96)) & (sv <= FLT_MAX))):
                have.add("strip out of range")
            ov, oc = v[strips[1]], d["color"][strips[1]]
            if np.all((ov >= F(0.01)) & (ov <= F(2.0))) and np.all((oc >= 0) & (oc <= 2)):
                have.add("strip in range")
    planes = {"color": c, "moments": m, "variance": v, "length": l, "normal": g[..., :3], "t": g[..., 3]}
    for name, a in planes.items():
        for s, what in zip(_bits(SPECIALS), SPECIAL_NAMES):
            if np.any(_bits(a) == s):
                have.add(f"{name}: {what}")
    return have


# ---- the cases both test modules run, and their restatement results (computed once) -------------
TINY = [(1, 1), (1, 19), (19, 1), (3, 3)]      # 3x3: narrower than the staged halo, passes 2+ tap nothing but the centre
BIG = [(16, 16), (17, 17), (37, 23)]           # one tile; one-pixel edge tiles; three tile columns, two rows
PASSES = {"extremes": (1, 5, 6), "nonfinite": (1, 2, 3)}   # three passes: both staged kernels and the plain one
N_SAMPLES = 2                                  # the moments' sample count (a device render of two batches)


def denoise_params(k):
    return (k, 0.6, 0.35, 0.25)


def var_params(k):
    return (k, 1.5, 0.35, 0.25)


def seeds(kind, W, H):
    """The seeds a size is run with: one, or those a tiny frame needs to see every value."""
    if (W, H) in BIG:
        return (100 * W + H,)
    return tuple(TINY_SEEDS) if kind == "extremes" else tuple(range(5))


def planes(kind):
    return ("all",) if kind == "extremes" else PLANES + ("all",)


@functools.lru_cache(maxsize=None)
def images(kind, W, H, seed, plane="all", cams=None):
    """The read-only image set of a case.  nonfinite seeds lie top left, in the 37x23 frame bottom right
    (its 5x7 corner tile)."""
    cams = None if cams is None else tuple(np.frombuffer(c, F) for c in cams)
    d = extremes(W, H, seed, cams) if kind == "extremes" else nonfinite(W, H, seed, plane, cams, corner=int(W > 32))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def cam_key(cur, prev):
    """Cameras as a hashable argument for images()."""
    return (np.ascontiguousarray(cur, F).tobytes(), np.ascontiguousarray(prev, F).tobytes())


@functools.lru_cache(maxsize=None)
def reference(op, kind, W, H, seed, plane, k):
    """The restatement's result of a filter case, read-only: op "atrous" (pt_denoise),
    "var" (pt_denoise_var from the moments) or "plane" (from the variance plane), k passes."""
    d = images(kind, W, H, seed, plane)
    if op == "atrous":
        out = D.atrous(d["color"], d["guide"], W, H, denoise_params(k))
    elif op == "var":
        out = V.atrous_var(d["color"], d["moments"], N_SAMPLES, d["guide"], W, H, var_params(k))
    else:
        out = T.atrous_var_plane(d["color"], d["variance"], d["guide"], W, H, var_params(k))
    out.setflags(write=False)
    return out


def enough(*outputs):
    """At least half of the floats of every output plane are not NaN: a NaN equals any NaN, so a
    result of mostly NaN would say little."""
    return all(2 * np.count_nonzero(~np.isnan(o)) >= o.size for o in outputs)


def filter_cases(op, kind, W, H):
    """(seed, plane, passes) of every case of a size that is run: all of a tiny size, and of the
    others those whose restatement result meets enough()."""
    for seed in seeds(kind, W, H):
        for plane in planes(kind):
            for k in PASSES[kind]:
                if (W, H) in TINY or enough(reference(op, kind, W, H, seed, plane, k)):
                    yield seed, plane, k
