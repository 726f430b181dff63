"""The adaptive stopping rule restated in numpy float32, independent of the
library's header code, and what the adaptive tests share: the crafted 40x24
frame with every hard case, the composition of uniform renders by tile and the
simulation of the whole loop.

The rule, per 16x16 tile (raster order) with count n and each of its pixels p
inside the frame:
  finite_p = |m1_p| <= FLT_MAX and |m2_p| <= FLT_MAX
  e_p  = sqrt(fmax(0, m2_p - m1_p * m1_p) / float(n - 1)) / fmax(m1_p, lum_floor)  if finite_p else +inf
  tile converged iff every e_p <= threshold;  E_T = fmax over e_p, from +0
  next = n if converged or n >= max else min(n + step, max)
Every operation is one float32 numpy operation (IEEE, rounded once)."""
import numpy as np

from denoise_var_ref import clamp0

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def tiles(W, H):
    return (W + 15) // 16, (H + 15) // 16


def pixel_error(m1, m2, n, lum_floor):
    """e_p of arrays of moments at the per-pixel counts n (uint32, >= 2)."""
    m1, m2 = np.asarray(m1, F), np.asarray(m2, F)
    with np.errstate(all="ignore"):
        var = clamp0(m2 - m1 * m1) / (n.astype(np.uint32) - np.uint32(1)).astype(F)
        e = np.sqrt(var) / np.fmax(m1, F(lum_floor))
        finite = (np.abs(m1) <= FLT_MAX) & (np.abs(m2) <= FLT_MAX)
    return np.where(finite, e, F(np.inf)).astype(F)


def select(moments, counts, W, H, params):
    """(next counts uint32, errors float32), one per tile in raster order."""
    lo, hi, step, thr, floor = params
    bx, by = tiles(W, H)
    m = np.asarray(moments, F).reshape(H, W, 2)
    counts = np.asarray(counts, np.uint32).reshape(-1)
    nxt, err = np.empty(bx * by, np.uint32), np.empty(bx * by, F)
    for b in range(bx * by):
        ty, tx = divmod(b, bx)
        t = m[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        n = counts[b]
        e = pixel_error(t[..., 0], t[..., 1], np.full(t.shape[:2], n, np.uint32), floor)
        conv = bool(np.all(e <= F(thr)))
        err[b] = np.fmax.reduce(e.reshape(-1), initial=F(0))
        nxt[b] = n if conv or n >= hi else min(int(n) + int(step), int(hi))
    return nxt, err


# ---- the crafted frame ---------------------------------------------------------------------------
W0, H0 = 40, 24                      # 3 x 2 tiles: 16, 16 and 8 wide; 16 and 8 high
PARAMS0 = (2, 9, 3, 0.25, 0.0625)    # threshold and floor exact in float32


def crafted():
    """Moments of the 40x24 frame, tile by tile:
      0  all zero: e = 0, stops at once
      1  converged: small variances, pixels with m2 < m1 * m1 (the clamp) and with m1 < lum_floor
      2  (8 wide) noisy: not converged; one pixel an ulp above the threshold
      3  (8 high) one pixel exactly at the threshold at n = 2 (m1 = 1, m2 = 1 + 1/16: e = 0.25), else zero
      4  one NaN pixel (m1), else zero: never converged
      5  (8 x 8) one pixel with m2 = +inf, else zero: never converged
    Returns (moments (H, W, 2) float32, a dict of where the cases lie)."""
    rng = np.random.default_rng(7)
    m = np.zeros((H0, W0, 2), F)
    # tile 1: m1 in [0.5, 2), variance of one sample at most (0.2 * m1)^2 -> e <= 0.2 at n = 2
    m1 = rng.uniform(0.5, 2.0, (16, 16)).astype(F)
    rel = rng.uniform(0.0, 0.2, (16, 16)).astype(F)
    m[0:16, 16:32, 0] = m1
    m[0:16, 16:32, 1] = m1 * m1 + (rel * m1) * (rel * m1)
    m[3, 20] = (1.5, 2.0)            # m2 < m1 * m1 = 2.25: the clamp, e = 0
    m[4, 21] = (0.01, 0.0002)        # m1 < lum_floor: var 1e-4, sqrt 0.01, / 0.0625 = 0.16
    m[5, 22] = (-0.5, 0.2501)        # a negative mean: the floor again
    # tile 2: m1 = 1, variance in [0.25, 4) -> e >= 0.5 at n = 2
    v = rng.uniform(0.25, 4.0, (16, 8)).astype(F)
    m[0:16, 32:40, 0] = 1.0
    m[0:16, 32:40, 1] = F(1.0) + v
    # tile 3: exactly at the threshold
    m[16, 0] = (1.0, 1.0625)
    # tile 4: NaN; tile 5: inf
    m[20, 18, 0] = np.nan
    m[23, 39] = (1.0, np.inf)
    where = {"zero": 0, "converged": 1, "noisy": 2, "at threshold": 3, "nan": 4, "inf": 5}
    return m, where


def just_above_threshold():
    """The crafted frame with tile 3's pixel one ulp of m2 above the threshold."""
    m, where = crafted()
    m[16, 0, 1] = np.nextafter(F(1.0625), F(2.0))
    return m, where


# ---- composition and simulation --------------------------------------------------------------------
def compose(by_count, counts, W, H):
    """The image whose tile b is by_count[counts[b]]'s: by_count maps a count to an (H, W, k) image."""
    bx, _ = tiles(W, H)
    first = next(iter(by_count.values()))
    out = np.empty_like(first)
    for b, n in enumerate(np.asarray(counts).reshape(-1)):
        ty, tx = divmod(b, bx)
        sl = (slice(ty * 16, ty * 16 + 16), slice(tx * 16, tx * 16 + 16))
        out[sl] = by_count[int(n)][sl]
    return out


def schedule(params):
    """The counts a tile can hold: min, min + step, ..., max."""
    lo, hi, step = params[:3]
    return sorted(set(list(range(lo, hi, step)) + [hi]))


def simulate(moments_by_count, W, H, params, rounds=None):
    """The loop in numpy: every round a tile's moments are the uniform render's at its count.  Returns
    (counts after the rounds, per round the ascending list of live tiles [(b, first_batch, n_batches)])."""
    lo, hi, step = params[:3]
    bx, by = tiles(W, H)
    counts = np.full(bx * by, lo, np.uint32)
    total = -(-(hi - lo) // step)
    lives = []
    for _ in range(total if rounds is None else min(rounds, total)):
        m = compose(moments_by_count, counts, W, H)
        nxt, _ = select(m, counts, W, H, params)
        lives.append([(b, int(counts[b]), int(nxt[b] - counts[b])) for b in range(bx * by) if nxt[b] != counts[b]])
        counts = nxt
    return counts, lives
