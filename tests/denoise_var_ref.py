"""numpy-float32 restatements of the luminance moments (PT_OPT_MOMENTS) and of
the variance-guided a-trous filter (include/pathtracer.h, "per-pixel luminance
moments and the variance-guided filter"), independent of csrc/pt_denoise.h:
vectorised over pixels, every operation a float32 numpy operation in the stated
association, exp taken from the oracle's pinned math (oracle_lib.math; numpy's
float32 sqrt is correctly rounded, like the library's).  Shared by
tests/test_denoise_var.py, tests/test_gpu_moments.py and
tests/test_gpu_denoise_var.py."""
import numpy as np

import oracle_lib

F = np.float32
TAP_K = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))   # the 5x5 taps, as pt_denoise
VAR_K = (F(0.5), F(0.25))                              # the 3x3 prefilter of the variance
DEFAULTS = (4, 1.5, 1.0, 1.0)                          # pt_denoise_var_default_params


def lum(rgb):
    """(0.2126 r + 0.7152 g) + 0.0722 b on the last axis."""
    rgb = np.asarray(rgb, F)
    return ((F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]).astype(F)


def fold_moments(moments, colours, batch):
    """One step of the fold: (H, W, 2) moments of batches 0..batch-1 and the
    (H, W, >= 3) sample colours of `batch` -> the moments of 0..batch."""
    L = lum(colours)
    fb, fb1 = F(batch), F(batch + 1)
    out = np.empty_like(moments, dtype=F)
    out[..., 0] = (moments[..., 0] * fb + L) / fb1
    out[..., 1] = (moments[..., 1] * fb + L * L) / fb1
    return out


def clamp0(x):
    """The statement's fmax_(0, x): x where x > 0, else +0 -- for a NaN too
    (fmax_ is maxNum) and for -0 (+0 is the first operand and the larger zero).
    Spelt out because numpy's fmax returns either zero, by array length."""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(x, F) > 0, x, F(0)).astype(F)


def var_of_mean(moments, n):
    """clamp0(m2 - m1 * m1) / float(n - 1)."""
    m1, m2 = moments[..., 0], moments[..., 1]
    with np.errstate(all="ignore"):
        return (clamp0(m2 - m1 * m1) / F(n - 1)).astype(F)


def atrous_var(rgba, moments, n_samples, guide, W, H, params=DEFAULTS):
    """The filter: (H, W, 4) float32."""
    iterations, sigma_lum, sigma_normal, sigma_depth = params
    c = np.ascontiguousarray(rgba, F).reshape(H, W, 4).copy()
    g = np.ascontiguousarray(guide, F).reshape(H, W, 4)
    v = var_of_mean(np.ascontiguousarray(moments, F).reshape(H, W, 2), n_samples)
    ys, xs = np.mgrid[0:H, 0:W]
    sl = F(sigma_lum)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sz2 = F(sigma_depth) * F(sigma_depth)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            gsum = np.zeros((H, W), F)
            gw = np.zeros((H, W), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qx, qy = xs + dx, ys + dy
                    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    k = VAR_K[abs(dx)] * VAR_K[abs(dy)]
                    vq = v[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    gsum = np.where(ok, gsum + k * vq, gsum)
                    gw = np.where(ok, gw + k, gw)
            den = (sl * np.sqrt(gsum / gw) + F(1e-6)).astype(F)
            lp = lum(c)
            sum_c = np.zeros((H, W, 3), F)
            sum_v = np.zeros((H, W), F)
            sum_w = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = xs + s * dx, ys + s * dy
                    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq, gq, vq = c[cy, cx], g[cy, cx], v[cy, cx]
                    h = TAP_K[abs(dx)] * TAP_K[abs(dy)]
                    dl = np.abs(lp - lum(cq))
                    dn = g[..., :3] - gq[..., :3]
                    d2n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                    dz = g[..., 3] - gq[..., 3]
                    arg = -((dl / den + d2n / sn2) + (dz * dz) / sz2)
                    w = h * oracle_lib.math(1, arg.astype(F).reshape(-1)).reshape(H, W)
                    sum_c = np.where(ok[..., None], sum_c + w[..., None] * cq[..., :3], sum_c)
                    sum_v = np.where(ok, sum_v + (w * w) * vq, sum_v)
                    sum_w = np.where(ok, sum_w + w, sum_w)
            out = np.empty_like(c)
            out[..., :3] = sum_c / sum_w[..., None]
            out[..., 3] = c[..., 3]
            c = out
            v = (sum_v / (sum_w * sum_w)).astype(F)
    return c


def make_images(W, H, seed, n_samples=8):
    """Seeded colours, moments and guide: fireflies, a block of zero variance
    beside the noisy rest, a block of misses in the guide, and pixels whose
    m2 is below m1 * m1 by rounding."""
    rng = np.random.default_rng(seed)
    rgba = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    fire = rng.uniform(size=(H, W)) < 0.05
    rgba[fire, :3] *= F(40.0)                                  # fireflies
    rgba[..., 3] = rng.uniform(0.5, 1.0, (H, W)).astype(F)
    m1 = lum(rgba)
    spread = rng.uniform(0.05, 1.5, (H, W)).astype(F)
    spread[fire] *= F(40.0)
    m2 = (m1 * m1 + spread * spread).astype(F)
    y0, x0 = H // 2, W // 8
    zy, zx = slice(y0, y0 + max(H // 3, 1)), slice(x0, x0 + max(W // 3, 1))
    rgba[zy, zx, :3] = np.array([0.25, 0.5, 0.75], F)          # a converged block: every sample the same
    m1[zy, zx] = lum(rgba[zy, zx])
    m2[zy, zx] = m1[zy, zx] * m1[zy, zx]
    below = rng.uniform(size=(H, W)) < 0.03                    # m2 < m1 * m1 by an ulp: the variance clamps at 0
    m2[below] = np.nextafter((m1 * m1).astype(F), F(0))[below]
    moments = np.stack([m1, m2], axis=-1).astype(F)
    guide = np.zeros((H, W, 4), F)
    guide[..., :3] = np.array([0.0, 0.0, 1.0], F)
    guide[:, W // 2:, :3] = np.array([0.6, 0.0, 0.8], F)       # second normal region
    guide[..., 3] = (3.0 + 0.01 * rng.uniform(size=(H, W))).astype(F)
    guide[H // 2:, :, 3] += F(0.75)                            # depth step
    gy, gx = H // 4, W // 4
    guide[gy:gy + max(H // 3, 1), gx:gx + max(W // 3, 1)] = np.array([0.0, 0.0, 0.0, 1e30], F)   # misses
    return rgba, moments, guide
