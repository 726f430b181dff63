"""numpy-float32 restatements of the guide ray and the a-trous filter
(include/pathtracer.h, "first-hit guide image and edge-avoiding a-trous
denoiser"), independent of csrc/pt_denoise.h: vectorised over pixels, every
operation a float32 numpy operation in the stated association, tan and exp
taken from the oracle's pinned math (oracle_lib.math).  Shared by
tests/test_denoise.py and tests/test_gpu_denoise.py."""
import numpy as np

import oracle_lib

F = np.float32
RAD = F(float.fromhex("0x1.1df46ap-6"))   # GLSL radians(): deg * float(pi / 180)
TAP_K = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
DEFAULTS = (5, 16.0, 0.35, 0.25)          # pt_denoise_default_params


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def _normalize(a):
    """a * (1 / sqrt((x*x + y*y) + z*z)) on the last axis."""
    d = a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]
    inv = F(1) / np.sqrt(d)
    return (a * inv[..., None]).astype(F)


def guide_rays(camera_ubo, W, H):
    """(origin (3,), directions (H, W, 3)) of every pixel's guide ray."""
    cam = np.asarray(camera_ubo, F)
    pos, cdir, cup, fov = cam[0:3], cam[4:7], cam[8:11], cam[12]
    right = _normalize(_cross(cdir, -cup))
    up = _normalize(_cross(right, cdir))
    tan_fov = oracle_lib.math(4, np.array([(fov * F(0.5)) * RAD], F))[0]
    ndc_x = (F(2) * np.arange(W, dtype=F)) / F(W) - F(1)
    ndc_y = (F(2) * np.arange(H, dtype=F)) / F(H) - F(1)
    aspect = F(W) / F(H)
    kx = ((ndc_x * tan_fov) * aspect)[None, :, None]   # (1, W, 1)
    ky = (ndc_y * tan_fov)[:, None, None]              # (H, 1, 1)
    d = (cdir[None, None, :] + (-right)[None, None, :] * kx) - up[None, None, :] * ky
    return pos.copy(), _normalize(d.astype(F))


def atrous(rgba, guide, W, H, params=DEFAULTS):
    """The filter: (H, W, 4) float32 from colours and guide {n.xyz, t}."""
    iterations, sigma_color, sigma_normal, sigma_depth = params
    c = np.ascontiguousarray(rgba, F).reshape(H, W, 4).copy()
    g = np.ascontiguousarray(guide, F).reshape(H, W, 4)
    ys, xs = np.mgrid[0:H, 0:W]
    sn2 = F(sigma_normal) * F(sigma_normal)
    sz2 = F(sigma_depth) * F(sigma_depth)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            sc = F(sigma_color) * F(2.0 ** -i)
            sc2 = sc * sc
            sum_c = np.zeros((H, W, 3), F)
            sum_w = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = xs + s * dx, ys + s * dy
                    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cq = c[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    gq = g[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    h = TAP_K[abs(dx)] * TAP_K[abs(dy)]
                    dc = c[..., :3] - cq[..., :3]
                    d2c = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                    dn = g[..., :3] - gq[..., :3]
                    d2n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                    dz = g[..., 3] - gq[..., 3]
                    arg = -((d2c / sc2 + d2n / sn2) + (dz * dz) / sz2)
                    w = h * oracle_lib.math(1, arg.astype(F).reshape(-1)).reshape(H, W)
                    sum_c = np.where(ok[..., None], sum_c + w[..., None] * cq[..., :3], sum_c)
                    sum_w = np.where(ok, sum_w + w, sum_w)
            out = np.empty_like(c)
            out[..., :3] = sum_c / sum_w[..., None]
            out[..., 3] = c[..., 3]
            c = out
    return c


def make_images(W, H, seed):
    """Seeded finite colours and a guide with two normal regions, a depth
    step and a block of misses."""
    rng = np.random.default_rng(seed)
    rgba = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    rgba[rng.uniform(size=(H, W)) < 0.05, :3] *= F(40.0)      # fireflies
    rgba[..., 3] = rng.uniform(0.5, 1.0, (H, W)).astype(F)
    guide = np.zeros((H, W, 4), F)
    guide[..., :3] = np.array([0.0, 0.0, 1.0], F)
    guide[:, W // 2:, :3] = np.array([0.6, 0.0, 0.8], F)      # second normal region
    guide[..., 3] = (3.0 + 0.01 * rng.uniform(size=(H, W))).astype(F)
    guide[H // 2:, :, 3] += F(0.75)                            # depth step
    y0, x0 = H // 4, W // 4
    guide[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 3, 1)] = np.array([0.0, 0.0, 0.0, 1e30], F)   # misses
    return rgba, guide
