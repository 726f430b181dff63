"""numpy-float32 restatement of the spatial variance estimate of pixels with a
short history (include/pathtracer.h, "spatial variance of pixels with too few
samples"), independent of csrc/pt_denoise.h: vectorised over pixels, every
operation a float32 numpy operation in the stated association, exp taken from
the oracle's pinned math (oracle_lib.math), division numpy's correctly rounded
one.  Also the hostile inputs the tests share.  Used by tests/test_spatial_var.py
and tests/test_gpu_spatial_var.py."""
import numpy as np

import oracle_lib
from denoise_var_ref import clamp0

F = np.float32
DEFAULTS = (2, 1, 1.0, 0.5)              # pt_spatial_var_default_params: below, radius, sigma_normal, sigma_depth
MISS = np.array([0.0, 0.0, 0.0, 1e30], F)
TILE = 16


def spatial_variance(moments, length, variance, guide, W, H, params=DEFAULTS):
    """The statement: (H, W) float32."""
    below, r, sigma_normal, sigma_depth = params
    m = np.ascontiguousarray(moments, F).reshape(H, W, 2)
    l = np.ascontiguousarray(length, F).reshape(H, W)
    v = np.ascontiguousarray(variance, F).reshape(H, W)
    g = np.ascontiguousarray(guide, F).reshape(H, W, 4)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sz2 = F(sigma_depth) * F(sigma_depth)
    ys, xs = np.mgrid[0:H, 0:W]
    sw, s1, s2 = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                qx, qy = xs + dx, ys + dy
                ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                mq, lq, gq = m[cy, cx], l[cy, cx], g[cy, cx]
                dn = g[..., :3] - gq[..., :3]
                d2n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                dz = g[..., 3] - gq[..., 3]
                arg = -(d2n / sn2 + (dz * dz) / sz2)
                w = oracle_lib.math(1, arg.astype(F).reshape(-1)).reshape(H, W) * lq
                # a tap whose guide compares equal to the centre's weighs len_q itself: exp(-0) * len_q for
                # finite guides, and the defined weight where an infinite component would make dz inf - inf
                w = np.where(np.all(g == gq, axis=-1), lq, w)
                sw = np.where(ok, sw + w, sw)
                s1 = np.where(ok, s1 + w * mq[..., 0], s1)
                s2 = np.where(ok, s2 + w * mq[..., 1], s2)
        M1, M2 = s1 / sw, s2 / sw
        est = (clamp0(M2 - M1 * M1) / l).astype(F)                # fmax_(0, x): a NaN difference gives 0
        short = l < F(below)                                       # false for a NaN length: the variance passes
    return np.where(short, est, v).astype(F)


def variance_of(moments, length):
    """The reprojection statement's out_var of the moments and lengths."""
    m1, m2 = moments[..., 0], moments[..., 1]
    with np.errstate(all="ignore"):
        return (clamp0(m2 - m1 * m1) / np.fmax(length - F(1), F(1))).astype(F)


def make_inputs(W, H, seed, only=None):
    """Hostile images for the estimate.  Returns a dict: moments (H, W, 2),
    length (H, W), variance (H, W), guide (H, W, 4), and the tile origins
    `tile_none` and `tile_corner` (None in a frame of a single tile column).

    The guide: normal +z and a depth rising gently across the frame; in the
    first W/8 columns the normal flipped to -z (a flip between neighbours); from
    row 3H/4 the depth times 1.2 (a depth step); a block of misses of a third
    of the frame at (W/4 + 2, H/4), whose moments are zero -- misses next to hits
    and next to misses.  Lengths: about a third 1 (m2 == m1 * m1, variance 0),
    the rest 2..64, also 2 and 3 (short under below = 4); fireflies.  With more
    than two tile columns, tile (1, 0) has no short pixel and tile (1, 1) only
    its first pixel, whose neighbourhood lies in three other tiles (the halo);
    pixels of length 1 are forced onto all four frame edges outside those
    tiles.  only = "none": every length long; only = "corner": every length
    long but pixel (0, 0)'s."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    g = np.zeros((H, W, 4), F)
    g[..., 2] = F(1.0)
    g[..., 3] = (F(3.0) + F(0.01) * xs.astype(F) + F(0.02) * ys.astype(F)).astype(F)
    g[:, :max(W // 8, 2), 2] = F(-1.0)                                      # the normal flip
    g[(3 * H) // 4:, :, 3] *= F(1.2)                                        # the depth step
    y0, x0 = H // 4, W // 4 + 2                                             # clear of pixel (16, 16)
    miss = np.zeros((H, W), bool)
    miss[y0:y0 + max(H // 3, 2), x0:x0 + max(W // 3, 2)] = True
    g[miss] = MISS
    length = rng.integers(2, 65, (H, W)).astype(F)
    length[rng.uniform(size=(H, W)) < 0.15] = F(2)
    length[rng.uniform(size=(H, W)) < 0.10] = F(3)
    length[rng.uniform(size=(H, W)) < 0.35] = F(1)
    tile_none = tile_corner = None
    if only == "none":
        length = np.maximum(length, F(8))
    elif only == "corner":
        length = np.maximum(length, F(8))
        length[0, 0] = F(1)
    elif W > 2 * TILE and H > TILE:
        tile_none, tile_corner = (TILE, 0), (TILE, TILE)
        for (tx, ty) in (tile_none, tile_corner):
            length[ty:ty + TILE, tx:tx + TILE] = np.maximum(length[ty:ty + TILE, tx:tx + TILE], F(8))
        length[TILE, TILE] = F(1)                                           # tile (1, 1)'s corner
    if only is None:
        length[0, 2] = length[H - 1, 3] = length[5, 0] = length[7, W - 1] = F(1)   # the four frame edges
    m1 = rng.uniform(0.0, 2.0, (H, W)).astype(F)
    spread = rng.uniform(0.05, 1.5, (H, W)).astype(F)
    fire = rng.uniform(size=(H, W)) < 0.05
    m1[fire] *= F(40.0)
    spread[fire] *= F(40.0)
    m2 = (m1 * m1 + spread * spread).astype(F)
    one = length == F(1)
    m2[one] = (m1 * m1)[one]                                                # one sample: m2 == m1 * m1
    m1[miss] = F(0)
    m2[miss] = F(0)
    moments = np.stack([m1, m2], axis=-1).astype(F)
    return {"moments": moments, "length": length, "variance": variance_of(moments, length), "guide": g,
            "miss": miss, "tile_none": tile_none, "tile_corner": tile_corner}
