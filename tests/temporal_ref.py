"""numpy-float32 restatements of the temporal reprojection statement
(include/pathtracer.h, "temporal reprojection") and of the variance-guided
a-trous filter from an explicit variance plane (pt_denoise_var_plane_host,
pt_temporal_denoise), independent of csrc/pt_denoise.h: vectorised over pixels,
every operation a float32 numpy operation in the stated association, tan and
exp taken from the oracle's pinned math (oracle_lib.math), division and square
root numpy's correctly rounded ones.  Shared by tests/test_temporal.py and
tests/test_gpu_temporal.py."""
import numpy as np

import denoise_ref as D
import denoise_var_ref as V
import oracle_lib

F = np.float32
DEFAULTS = (64, 0.0, 0.5, 0.05)          # pt_temporal_default_params
MISS = np.array([0.0, 0.0, 0.0, 1e30], F)


def cam_basis(cam):
    """(pos, dir, right, up', tan_fov) of a camera UBO, as the guide ray's frame."""
    cam = np.asarray(cam, F)
    pos, cdir, cup, fov = cam[0:3].copy(), cam[4:7].copy(), cam[8:11], cam[12]
    right = D._normalize(D._cross(cdir, -cup))
    up = D._normalize(D._cross(right, cdir))
    tan_fov = oracle_lib.math(4, np.array([(fov * F(0.5)) * D.RAD], F))[0]
    return pos, cdir, right, up, tan_fov


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rotate_y(cam, degrees):
    """The camera UBO with position and direction rotated about +y (float64, rounded once)."""
    a = np.deg2rad(float(degrees))
    c, s = np.cos(a), np.sin(a)
    out = np.array(cam, F)
    for o in (0, 4):
        x, z = float(cam[o]), float(cam[o + 2])
        out[o], out[o + 2] = x * c + z * s, z * c - x * s
    return out


def reproject(cam_cur, cam_prev, W, H, n, color, moments, guide, history=None, params=DEFAULTS):
    """The statement.  Returns (colour (H, W, 4), moments (H, W, 2), length
    (H, W), variance (H, W), info); info counts the pixels of each branch:
    'miss', 'behind' (z <= 0), 'outside' (fx or fy off the frame), 'no_valid'
    (sw == 0), 'blended', and 'taps'[k] = blended pixels with k valid taps."""
    max_history, alpha_min, normal_min, depth_rel = params
    c = np.ascontiguousarray(color, F).reshape(H, W, 4)
    m = np.ascontiguousarray(moments, F).reshape(H, W, 2)
    g = np.ascontiguousarray(guide, F).reshape(H, W, 4)
    fn = F(n)
    out_c, out_m = c.copy(), m.copy()
    out_len = np.full((H, W), fn, F)
    info = {"miss": 0, "behind": 0, "outside": 0, "no_valid": 0, "blended": 0, "taps": [0] * 5}
    if history is not None:
        hc = np.ascontiguousarray(history[0], F).reshape(H, W, 4)
        hm = np.ascontiguousarray(history[1], F).reshape(H, W, 2)
        hl = np.ascontiguousarray(history[2], F).reshape(H, W)
        hg = np.ascontiguousarray(history[3], F).reshape(H, W, 4)
        pos = cam_basis(cam_cur)[0]
        _, dirs = D.guide_rays(cam_cur, W, H)
        ppos, pdir, pright, pup, ptan = cam_basis(cam_prev)
        t = g[..., 3]
        hit = t < F(1e30)
        with np.errstate(all="ignore"):
            P = (pos[None, None, :] + dirs * t[..., None]).astype(F)
            v = (P - ppos[None, None, :]).astype(F)
            z = _dot(v, pdir[None, None, :])
            front = hit & (z > F(0))
            aspect = F(W) / F(H)
            sx = _dot(v, (-pright)[None, None, :]) / (z * (ptan * aspect))
            sy = _dot(v, (-pup)[None, None, :]) / (z * ptan)
            fx = ((sx + F(1)) * F(W)) * F(0.5)
            fy = ((sy + F(1)) * F(H)) * F(0.5)
            inside = front & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
            x0f, y0f = np.floor(fx), np.floor(fy)
            ax, ay = (fx - x0f).astype(F), (fy - y0f).astype(F)
            x0 = np.where(inside, x0f, F(0)).astype(np.int64)
            y0 = np.where(inside, y0f, F(0)).astype(np.int64)
            dexp = np.sqrt(_dot(v, v))
            dtol = F(depth_rel) * dexp
            sw = np.zeros((H, W), F)
            sc = np.zeros((H, W, 3), F)
            sm = np.zeros((H, W, 2), F)
            lmin = np.full((H, W), np.inf, F)
            nvalid = np.zeros((H, W), np.int64)
            for ty in (0, 1):
                for tx in (0, 1):
                    qx, qy = x0 + tx, y0 + ty
                    ok = inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    b = ((ax if tx else F(1) - ax) * (ay if ty else F(1) - ay)).astype(F)
                    hlq, hgq, hcq, hmq = hl[cy, cx], hg[cy, cx], hc[cy, cx], hm[cy, cx]
                    valid = (ok & (hlq > F(0)) & (hgq[..., 3] < F(1e30)) & (np.abs(hgq[..., 3] - dexp) <= dtol)
                             & (_dot(g[..., :3], hgq[..., :3]) >= F(normal_min)))
                    sw = np.where(valid, sw + b, sw)
                    sc = np.where(valid[..., None], sc + b[..., None] * hcq[..., :3], sc)
                    sm = np.where(valid[..., None], sm + b[..., None] * hmq, sm)
                    lmin = np.where(valid, np.fmin(lmin, hlq), lmin)
                    nvalid += valid
            found = inside & (sw > F(0))
            h = (sc / sw[..., None]).astype(F)
            h_m = (sm / sw[..., None]).astype(F)
            N = np.fmin(lmin, F(max_history))
            a = np.fmax(F(alpha_min), fn / (N + fn)).astype(F)
            bc = (h + (c[..., :3] - h) * a[..., None]).astype(F)
            bm = (h_m + (m - h_m) * a[..., None]).astype(F)
        out_c[..., :3] = np.where(found[..., None], bc, c[..., :3])
        out_m = np.where(found[..., None], bm, m).astype(F)
        out_len = np.where(found, N + fn, fn).astype(F)
        info["miss"] = int(np.count_nonzero(~hit))
        info["behind"] = int(np.count_nonzero(hit & ~front))
        info["outside"] = int(np.count_nonzero(front & ~inside))
        info["no_valid"] = int(np.count_nonzero(inside & ~found))
        info["blended"] = int(np.count_nonzero(found))
        info["taps"] = [int(np.count_nonzero(found & (nvalid == k))) for k in range(5)]
    with np.errstate(all="ignore"):
        var = (V.clamp0(out_m[..., 1] - out_m[..., 0] * out_m[..., 0]) / np.fmax(out_len - F(1), F(1))).astype(F)
    return out_c, out_m, out_len, var, info


def atrous_var_plane(rgba, variance, guide, W, H, params=V.DEFAULTS):
    """The variance-guided filter from pass 0's variance plane: (H, W, 4) float32."""
    iterations, sigma_lum, sigma_normal, sigma_depth = params
    c = np.ascontiguousarray(rgba, F).reshape(H, W, 4).copy()
    g = np.ascontiguousarray(guide, F).reshape(H, W, 4)
    v = np.ascontiguousarray(variance, F).reshape(H, W).copy()
    ys, xs = np.mgrid[0:H, 0:W]
    sl = F(sigma_lum)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sz2 = F(sigma_depth) * F(sigma_depth)
    g5 = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
    g3 = (F(0.5), F(0.25))
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            gsum, gw = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qx, qy = xs + dx, ys + dy
                    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    k = g3[abs(dx)] * g3[abs(dy)]
                    vq = v[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                    gsum = np.where(ok, gsum + k * vq, gsum)
                    gw = np.where(ok, gw + k, gw)
            den = (sl * np.sqrt(gsum / gw) + F(1e-6)).astype(F)
            lp = V.lum(c)
            sum_c, sum_v, sum_w = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = xs + s * dx, ys + s * dy
                    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq, gq, vq = c[cy, cx], g[cy, cx], v[cy, cx]
                    h = g5[abs(dx)] * g5[abs(dy)]
                    dl = np.abs(lp - V.lum(cq))
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


def plane_guide(cam, W, H):
    """The analytic guide {n.xyz, t} of `cam`'s guide rays on the plane z = 0
    (normal +z); a ray that does not reach it in front of the camera is a miss."""
    pos, dirs = D.guide_rays(cam, W, H)
    with np.errstate(all="ignore"):
        t = (-pos[2] / dirs[..., 2]).astype(F)
    hit = np.isfinite(t) & (t > F(0)) & (t < F(1e6))
    g = np.empty((H, W, 4), F)
    g[...] = MISS
    g[hit, :3] = np.array([0.0, 0.0, 1.0], F)
    g[hit, 3] = t[hit]
    return g


def _colours(rng, W, H):
    rgba = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    fire = rng.uniform(size=(H, W)) < 0.05
    rgba[fire, :3] *= F(40.0)                                              # fireflies
    rgba[..., 3] = rng.uniform(0.5, 1.0, (H, W)).astype(F)
    m1 = V.lum(rgba)
    spread = rng.uniform(0.05, 1.5, (H, W)).astype(F)
    spread[fire] *= F(40.0)
    m2 = (m1 * m1 + spread * spread).astype(F)
    below = rng.uniform(size=(H, W)) < 0.03                                # m2 < m1 * m1 by an ulp
    m2[below] = np.nextafter((m1 * m1).astype(F), F(0))[below]
    return rgba, np.stack([m1, m2], axis=-1).astype(F), fire


def make_inputs(W, H, seed, cam_cur, cam_prev):
    """Hostile images around the analytic guides of the two cameras on the
    plane z = 0: a block of misses in the new guide; in the history guide a
    depth step (rows from 3H/4: t * 1.2) and a second normal region (columns
    from 3W/4: a normal perpendicular to +z), so that pixels at their borders
    have one to three valid taps; a block of zero history length; history
    lengths up to 200, above max_history 64; fireflies; m2 < m1 * m1 by an ulp.
    Returns a dict: color, moments, guide, history = (colour, moments, length,
    guide), fire (the new frame's firefly mask)."""
    rng = np.random.default_rng(seed)
    color, moments, fire = _colours(rng, W, H)
    hcolor, hmoments, _ = _colours(rng, W, H)
    guide = plane_guide(cam_cur, W, H)
    y0, x0 = H // 4, W // 4
    guide[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 3, 1)] = MISS           # a block of misses
    hguide = plane_guide(cam_prev, W, H)
    hguide[(3 * H) // 4:, :, 3] *= F(1.2)                                  # depth step (a miss stays >= 1e30)
    sec = hguide[:, (3 * W) // 4:, :]
    sec[sec[..., 3] < F(1e30), :3] = np.array([0.6, 0.8, 0.0], F)          # second normal region
    hlength = rng.integers(1, 201, (H, W)).astype(F)
    zy, zx = H // 8, W // 2
    hlength[zy:zy + max(H // 4, 1), zx:zx + max(W // 4, 1)] = F(0)         # no history here
    return {"color": color, "moments": moments, "guide": guide, "fire": fire,
            "history": (hcolor, hmoments, hlength, hguide)}
