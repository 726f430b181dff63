"""numpy-float32 restatement of the display transform (include/pathtracer.h,
"display transform"), independent of csrc/pt_display.h: vectorised over pixels,
every operation a float32 numpy operation in the stated association, exp and
log taken from the oracle's pinned math (oracle_lib.math), the sRGB code from
the double-precision statement itself (math.pow, no table).  Also the hostile
images tests/test_display.py and tests/test_gpu_display.py share, and what they
must contain (holds)."""
import functools
import math

import numpy as np

import oracle_lib

F = np.float32
BOUND = F(2.0 ** 40)
CLAMP, REINHARD, ACES = 0, 1, 2
DEFAULTS = (CLAMP, 1.0, 0, 0.18, 4.0, 1.0)   # pt_display_default_params
SEAM = F(0.0031308)
FLT_MAX = F(3.4028234663852886e38)


def srgb8_one(x):
    """The double-precision statement for one float32."""
    x = float(x)
    if not x > 0.0:
        return 0
    if x >= 1.0:
        return 255
    e = 12.92 * x if x <= float(SEAM) else 1.055 * math.pow(x, 1.0 / 2.4) - 0.055
    return int(e * 255.0 + 0.5)


def srgb8(v):
    """uint8 codes of a float32 array, each distinct value encoded once."""
    v = np.ascontiguousarray(v, F)
    uniq, inverse = np.unique(v.view(np.uint32).reshape(-1), return_inverse=True)
    codes = np.array([srgb8_one(x) for x in uniq.view(F)], np.uint8)
    return codes[inverse].reshape(v.shape)


@functools.lru_cache(maxsize=None)
def _thresholds():
    """T[1..255] as float32 bit patterns (index 0 unused, 0): the least float of each code, by bisection
    over the bit patterns of (0, 1]."""
    t = np.zeros(256, np.uint32)
    for k in range(1, 256):
        lo, hi = 0, 0x3f800000
        while hi - lo > 1:
            m = (lo + hi) // 2
            if srgb8_one(np.uint32(m).view(F)) >= k:
                hi = m
            else:
                lo = m
        t[k] = hi
    t.setflags(write=False)
    return t


def thresholds():
    return _thresholds().copy()


def lum(r, g, b):
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def _tree256(v):
    """v: (..., 256) float32; the halving tree on the last axis."""
    v = v.copy()
    s = 128
    while s > 0:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s >>= 1
    return v[..., 0]


def meter(rgba, W, H):
    """(sum of log L over the metered pixels by the stated tree, their number)."""
    c = np.ascontiguousarray(rgba, F).reshape(H, W, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.fmax(c[..., :3], F(0))
        L = lum(p[..., 0], p[..., 1], p[..., 2])
        metered = np.isfinite(L) & (L > 0)
    term = np.zeros((H, W), F)
    term[metered] = oracle_lib.math(0, L[metered])
    by, bx = (H + 15) // 16, (W + 15) // 16
    pad = np.zeros((by * 16, bx * 16), F)
    pad[:H, :W] = term
    tiles = pad.reshape(by, 16, bx, 16).transpose(0, 2, 1, 3).reshape(by * bx, 256)   # lane = ly * 16 + lx
    partial = _tree256(tiles)
    rows = (partial.size + 255) // 256
    grid = np.zeros(rows * 256, F)
    grid[:partial.size] = partial
    lanes = np.zeros(256, F)
    for r in grid.reshape(rows, 256):   # lane j: partials j, j + 256, ... in that order
        lanes = lanes + r
    return _tree256(lanes), int(np.count_nonzero(metered))


def auto_scale(total, n, key, adapt, prev):
    """prev: the previous scale, or None / 0 for none."""
    if n == 0:
        return F(prev) if prev else F(1)
    mean = F(total) / F(n)
    target = F(key) / oracle_lib.math(1, np.array([mean], F))[0]
    if not prev or F(adapt) == F(1):
        return F(target)
    return F(F(prev) + (F(target) - F(prev)) * F(adapt))


def tone(rgba, W, H, tonemap, scale, white):
    """rgb before the encode, (H, W, 3) float32."""
    c = np.ascontiguousarray(rgba, F).reshape(H, W, 4)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = np.fmin(np.fmax(c[..., :3] * F(scale), F(0)), BOUND)
        if tonemap == REINHARD:
            w2 = F(white) * F(white)
            L = lum(v[..., 0], v[..., 1], v[..., 2])
            Lp = (L * (F(1) + L / w2)) / (F(1) + L)
            q = Lp / L
            v = np.where((L > 0)[..., None], v * q[..., None], v)
        elif tonemap == ACES:
            v = (v * (F(2.51) * v + F(0.03))) / (v * (F(2.43) * v + F(0.59)) + F(0.14))
    return v.astype(F)


def display(rgba, W, H, params=DEFAULTS, prev=None):
    """((H, W, 4) uint8, the auto scale used or None without metering, the metered pixels or None)."""
    tonemap, exposure, auto, key, white, adapt = params
    scale, used, n = F(exposure), None, None
    if auto:
        total, n = meter(rgba, W, H)
        used = auto_scale(total, n, key, adapt, prev)
        scale = F(exposure) * used
    out = np.empty((H, W, 4), np.uint8)
    out[..., :3] = srgb8(tone(rgba, W, H, tonemap, scale, white))
    out[..., 3] = 255
    return out, used, n


# ---- the one comparison of bytes and of a float's bits -------------------------------------
def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and want.dtype == np.uint8 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, " \
                          f"want {want[tuple(bad[0])]}"


def same_float(got, want, what):
    assert F(got).view(np.uint32) == F(want).view(np.uint32), f"{what}: got {float(got)!r}, want {float(want)!r}"


# ---- the hostile images --------------------------------------------------------------------
def _u2f(bits):
    return np.array(bits, np.uint32).view(F)


SPECIALS = np.concatenate([
    _u2f([0x7fc00000, 0xffc00001]),                     # NaNs
    np.array([np.inf, -np.inf, -1.0, -3.0e38, -0.0], F),
    _u2f([0x00000001, 0x007fffff, 0x80000001]),         # subnormals
    np.array([3.4e38, FLT_MAX, 1.0, 0.5, float(SEAM), 2.0 ** 40, 2.0 ** 41, 1e-30], F)])


def image(kind, W, H, seed=0):
    """A W x H rgba image: "specials" (lit pixels of every magnitude with exact zeros beside them, the
    special values in the last rows, and, in a frame of more than one tile, tile 0 without a metered
    pixel), "thresholds" (pixel k - 1 holds the float below T[k], T[k] and the one above; random
    colours behind them) or "dark" (nothing metered: zeros, negatives, NaN)."""
    rng = np.random.default_rng(seed + 131 * W + H)
    img = np.exp(rng.uniform(-9.0, 3.0, (H, W, 4))).astype(F)
    img[..., 3] = 1
    if kind == "dark":
        img[..., :3] = rng.choice(np.array([0.0, -0.0, -1.0, np.nan, -np.inf], F), (H, W, 3))
        return img
    img[rng.random((H, W)) < 0.3, :3] = 0          # the culled background, beside lit pixels
    if kind == "thresholds":
        t = thresholds()[1:]
        flat = img.reshape(-1, 4)
        flat[:255, 0] = (t - 1).view(F)
        flat[:255, 1] = t.view(F)
        flat[:255, 2] = (t + 1).view(F)
        return img
    assert kind == "specials"
    flat = img.reshape(-1, 4)
    n = SPECIALS.size
    for k in range(3 * n):                          # every special in every channel, other channels lit or zero
        flat[flat.shape[0] - 1 - k, k % 3] = SPECIALS[k // 3]
    if W > 16 or H > 16:
        img[:16, :16, :3] = rng.choice(np.array([0.0, -2.0, np.nan], F), (min(H, 16), min(W, 16), 3))
    return img


def holds(img, W, H):
    """What an image contains, as a set of names."""
    c = np.ascontiguousarray(img, F).reshape(H, W, 4)[..., :3]
    u = c.view(np.uint32)
    have = set()
    if np.isnan(c).any():
        have.add("nan")
    if (c == np.inf).any():
        have.add("+inf")
    if (c == -np.inf).any():
        have.add("-inf")
    with np.errstate(invalid="ignore"):
        if ((c < 0) & np.isfinite(c)).any():
            have.add("negative")
        if (c >= F(3.4e38)).any() and np.isfinite(c[c >= F(3.4e38)]).any():
            have.add("huge")
    if (u == 0x80000000).any():
        have.add("-0")
    if (((u & 0x7f800000) == 0) & ((u & 0x007fffff) != 0)).any():
        have.add("subnormal")
    t = thresholds()[1:]
    if all(np.isin(t.astype(np.int64) + d, u).all() for d in (-1, 0, 1)):
        have.add("thresholds")
    zero = np.all(c == 0, axis=2)
    lit = np.all(c > 0, axis=2)
    if (zero[:, :-1] & lit[:, 1:]).any() or (zero[:, 1:] & lit[:, :-1]).any():
        have.add("zero beside lit")
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.fmax(c, F(0))
        L = lum(p[..., 0], p[..., 1], p[..., 2])
        metered = np.isfinite(L) & (L > 0)
    tiles = [metered[y:y + 16, x:x + 16].any() for y in range(0, H, 16) for x in range(0, W, 16)]
    if len(tiles) > 1 and not all(tiles) and any(tiles):
        have.add("empty tile")
    if not any(tiles):
        have.add("nothing metered")
    return have
