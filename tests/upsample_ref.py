"""numpy-float32 restatement of guide-driven upsampling (include/pathtracer.h,
"guide-driven upsampling"), independent of csrc/pt_upsample.h: vectorised over
the output pixels, every operation a float32 numpy operation in the stated
association, exp taken from the oracle's pinned math (oracle_lib.math).  Not a
test module: shared by tests/test_upsample.py and tests/test_gpu_upsample.py."""
import functools

import numpy as np

import hostile_images as HI
import oracle_lib

F = np.float32
DEFAULTS = (2, 0.35, 0.25)          # pt_upsample_default_params
MISS = np.array([0.0, 0.0, 0.0, 1e30], F)
# (w, h, scale) of the seeded cases: a 1x1 source; one cell whose fx is no dyadic fraction; an odd size;
# 68x48 = four tiles and a ragged fifth, the last lattice column without a right neighbour; the largest scale
SHAPES = [(1, 1, 2), (3, 2, 3), (9, 5, 2), (17, 12, 4), (5, 3, 8)]


def upsample(src, guide, w, h, params=DEFAULTS, fallbacks=False):
    """The statement: (s*h, s*w, 4) float32 from the (h, w, 4) colours and the
    (s*h, s*w, 4) guide {n.xyz, t}.  fallbacks: also the mask of the pixels that
    took the fallback."""
    s, sigma_normal, sigma_depth = params
    W, H = s * w, s * h
    c = np.ascontiguousarray(src, F).reshape(h, w, 4)
    g = np.ascontiguousarray(guide, F).reshape(H, W, 4)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sz2 = F(sigma_depth) * F(sigma_depth)
    Y, X = np.mgrid[0:H, 0:W]
    i0, j0 = X // s, Y // s
    fx = (X - i0 * s).astype(F) / F(s)
    fy = (Y - j0 * s).astype(F) / F(s)
    bx, by = (F(1) - fx, fx), (F(1) - fy, fy)
    sum_c = np.zeros((H, W, 3), F)
    sum_w = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dj in (0, 1):
            for di in (0, 1):
                i, j = i0 + di, j0 + dj
                ok = (i < w) & (j < h) & (bx[di] != 0) & (by[dj] != 0)
                ic, jc = np.minimum(i, w - 1), np.minimum(j, h - 1)
                gq = g[jc * s, ic * s]
                cq = c[jc, ic]
                dn = g[..., :3] - gq[..., :3]
                d2n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                dz = g[..., 3] - gq[..., 3]
                arg = -(d2n / sn2 + (dz * dz) / sz2)
                wt = (bx[di] * by[dj]) * oracle_lib.math(1, arg.astype(F).reshape(-1)).reshape(H, W)
                sum_c = np.where(ok[..., None], sum_c + wt[..., None] * cq[..., :3], sum_c)
                sum_w = np.where(ok, sum_w + wt, sum_w)
        c0 = c[j0, i0]
        good = sum_w > 0                      # false for NaN too
        out = np.empty((H, W, 4), F)
        out[..., :3] = np.where(good[..., None], sum_c / sum_w[..., None], c0[..., :3])
        out[..., 3] = c0[..., 3]
    return (out, ~good) if fallbacks else out


def make_images(w, h, s, seed):
    """Seeded finite colours of the low frame and a full-size guide with two normal
    regions, a depth step and a block of misses."""
    W, H = s * w, s * h
    rng = np.random.default_rng(seed)
    rgba = rng.uniform(0.0, 2.0, (h, w, 4)).astype(F)
    rgba[rng.uniform(size=(h, w)) < 0.05, :3] *= F(40.0)       # fireflies
    guide = np.zeros((H, W, 4), F)
    guide[..., :3] = np.array([0.0, 0.0, 1.0], F)
    guide[:, W // 2:, :3] = np.array([0.6, 0.0, 0.8], F)       # second normal region
    guide[..., 3] = (3.0 + 0.01 * rng.uniform(size=(H, W))).astype(F)
    guide[H // 2:, :, 3] += F(0.25)                             # depth step
    y0, x0 = H // 4, W // 4
    guide[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 3, 1)] = MISS
    return rgba, guide


def edge_images(w, h, s):
    """A flat wall with a block of misses whose border lies off the lattice, at
    least s pixels wide and high and clear of the last lattice row and column:
    every pixel then has a lattice tap of its own kind (hit or miss) with a
    non-zero bilinear weight.  Colour 0.25 at the hit lattice points and 4.0 at
    the miss ones: powers of two, so every product and quotient is exact."""
    W, H = s * w, s * h
    guide = np.zeros((H, W, 4), F)
    guide[..., 2] = F(1.0)
    guide[..., 3] = (F(3.0) + F(2.0 ** -10) * (np.arange(W, dtype=F)[None, :] + np.arange(H, dtype=F)[:, None])).astype(F)
    x0, x1 = s * (w // 4) + 1, s * (w - w // 4 - 1) - 1
    y0, y1 = s * (h // 4) + 1, s * (h - h // 4 - 1) - 1
    assert x0 % s and x1 % s and y0 % s and y1 % s and x1 - x0 + 1 >= s and y1 - y0 + 1 >= s
    assert x1 < s * (w - 1) and y1 < s * (h - 1)
    guide[y0:y1 + 1, x0:x1 + 1] = MISS
    miss = guide[..., 3] >= F(1e30)
    src = np.zeros((h, w, 4), F)
    src[..., :3] = np.where(miss[::s, ::s, None], F(4.0), F(0.25))
    src[..., 3] = F(1.0)
    return src, guide, miss


# ---- the hostile pools (tests/hostile_images.py): colour of the low frame, normal and distance planes of the
# full one, scale 2 ------------------------------------------------------------------------------------------
HOSTILE_SCALE = 2


def hostile_cases(kind):
    """(w, h, seed, plane) of every hostile case of a kind: "extremes", or "nonfinite" with the values in
    the colour, the normal, the distance or all planes; the sizes are the source's."""
    for w, h in HI.TINY + HI.BIG:
        for seed in HI.seeds(kind, w, h):
            for plane in (("all",) if kind == "extremes" else ("color", "normal", "t", "all")):
                yield w, h, seed, plane


def hostile_images(kind, w, h, seed, plane):
    """(colours (h, w, 4), full guide (2h, 2w, 4)) of a case, read-only: the colour of the w x h set, the
    guide of the 2w x 2h set (a plane that a case leaves alone is ordinary)."""
    s = HOSTILE_SCALE
    return HI.images(kind, w, h, seed, plane)["color"], HI.images(kind, s * w, s * h, seed, plane)["guide"]


@functools.lru_cache(maxsize=None)
def hostile_reference(kind, w, h, seed, plane):
    color, guide = hostile_images(kind, w, h, seed, plane)
    out = upsample(color, guide, w, h, (HOSTILE_SCALE, 0.35, 0.25))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def seeded(w, h, s):
    """(colours, guide, the restatement's result at the default sigmas) of a seeded shape, read-only."""
    rgba, guide = make_images(w, h, s, 1000 * w + 10 * h + s)
    out = upsample(rgba, guide, w, h, (s, 0.35, 0.25))
    for a in (rgba, guide, out):
        a.setflags(write=False)
    return rgba, guide, out
