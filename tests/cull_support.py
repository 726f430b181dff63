"""What the primary-cull tests share, on the CPU and on the GPU: the cameras and
lights of the cases, float64 restatements of the primary rays and of what
they can reach, the pixel mask of a rectangle set, and the count of samples
the tight rectangles let the kernel skip."""
import numpy as np

import ptamd
import scenes


def frame(cam):
    cpos, cdir, cup, fov = cam[0:3].astype(np.float64), cam[4:7].astype(np.float64), cam[8:11].astype(np.float64), float(cam[12])
    right = np.cross(cdir, -cup)
    right /= np.linalg.norm(right)
    up = np.cross(right, cdir)
    up /= np.linalg.norm(up)
    return cpos, cdir, right, up, np.tan(np.radians(fov * 0.5))


def rays(cam, W, H, px, py, ox, oy, jx, jy):
    """Primary rays of raytrace_comp.comp:430-460 for given aperture/jitter draws (float64)."""
    cpos, cdir, right, up, T = frame(cam)
    A = W / H
    ndcx = (2.0 * px / W - 1.0) + jx * 0.5 / W
    ndcy = (2.0 * py / H - 1.0) + jy * 0.5 / H
    o = cpos + right * ox + up * oy
    b = cdir - right * (ndcx * T * A) - up * (ndcy * T)
    b /= np.linalg.norm(b)
    d = cpos + 3.0 * b - o
    return o, d / np.linalg.norm(d)


def slab_hit(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0 = (lo - o) * inv
        t1 = (hi - o) * inv
    tmin = np.nanmax(np.fmin(t0, t1))
    tmax = np.nanmin(np.fmax(t0, t1))
    return tmin <= tmax and tmax >= 0


def light_hit(o, d, L):
    pos, n = L[0:3].astype(np.float64), L[4:7].astype(np.float64)
    nn = n / np.linalg.norm(n)
    basis = np.array([0.0, 1.0, 0.0]) if abs(nn[1]) < 0.999 else np.array([1.0, 0.0, 0.0])
    r = np.cross(nn, basis)
    r /= np.linalg.norm(r)
    u = np.cross(r, nn)
    den = np.dot(n, d)
    if abs(den) < 1e-4:
        return False
    t = np.dot(n, pos - o) / den
    if t <= 0:
        return False
    th = o + d * t - pos
    return abs(np.dot(th, r)) <= L[12] * 0.5 and abs(np.dot(th, u)) <= L[13] * 0.5


def culled_mask(rects, W, H):
    px = np.arange(W, dtype=np.float32)
    py = np.arange(H, dtype=np.float32)
    nx = (np.float32(2.0) * px / np.float32(W)) - np.float32(1.0)
    ny = (np.float32(2.0) * py / np.float32(H)) - np.float32(1.0)
    live = np.zeros((H, W), bool)
    for x0, x1, y0, y1 in rects:
        live |= ((ny >= y0) & (ny <= y1))[:, None] & ((nx >= x0) & (nx <= x1))[None, :]
    return ~live


def margin_mask(loose, tight, W, H):
    """Pixels inside a loose rectangle but outside every tight one."""
    return ~culled_mask(loose, W, H) & culled_mask(tight, W, H)


TWO_LIGHTS = np.concatenate([scenes.REFERENCE_LIGHT,
                             np.array([1.5, 0.5, 2.0, 0, -1, 0, 0, 0, 3, 2, 1, 0, 0.5, 1.0, 0, 0], np.float32)])

# (name, camera, W, H, lights)
CASES = [
    ("default", scenes.DEFAULT_CAMERA, 96, 54, scenes.REFERENCE_LIGHT),
    ("orbit", scenes.camera((3.0, 2.0, 4.0)), 80, 60, scenes.REFERENCE_LIGHT),
    ("far_wide", scenes.camera((0.0, 0.5, 12.0), fov=100.0), 64, 64, TWO_LIGHTS),
    ("narrow", scenes.camera((1.0, -1.0, 7.0), fov=20.0), 70, 40, TWO_LIGHTS),
    ("tiny", scenes.DEFAULT_CAMERA, 17, 13, scenes.REFERENCE_LIGHT),
    ("tilted_up", np.array([0, 0, 14, 0, 0, 0, -2, 0, 0.3, 1, 0.2, 0, 45, 0, 0, 0], np.float32), 64, 48,
     scenes.REFERENCE_LIGHT),
]
CASE_IDS = [c[0] for c in CASES]


def ring_lights(n):
    """n small lights on a ring above the box, facing down."""
    return np.concatenate([ptamd.pack_light([1.5 * np.cos(k * 0.785), 2, 1.5 * np.sin(k * 0.785)], [0, -1, 0], [3, 2, 1],
                                            [0.6, 0.6]) for k in range(n)])


def rng_draws(seeds, n):
    """The shader's RNG (raytrace_comp.comp:207-216) in numpy: the first n
    draws of every seed, (len(seeds), n) float32."""
    s = np.asarray(seeds, np.uint64) & np.uint64(0xFFFFFFFF)
    m32 = np.uint64(0xFFFFFFFF)
    out = np.empty((s.size, n), np.float32)
    for k in range(n):
        s = (s * np.uint64(747796405) + np.uint64(2891336453)) & m32
        r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & m32
        r = (r >> np.uint64(22)) ^ r
        out[:, k] = r.astype(np.uint32).astype(np.float32) / np.float32(4294967296.0)
    return out


def skip_counts(cam, W, H, lights, first_batch, n_batches, lo=(-1, -1, -1), hi=(1, 1, 1)):
    """What include/pathtracer.h defines for PT_OPT_CULL_TIGHT, counted on the
    host: (live pixels, margin samples the kernel must skip, margin samples it
    must trace) over the batches.  A margin pixel lies inside a loose
    rectangle and outside every tight one; its sample of a batch is skipped
    when draws 0 and 2 of seed (batch * H + y) * W + x, after fmax(1e-38, .),
    are both at least u0."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    loose = ptamd.primary_cull_rects(cam, W, H, lo, hi, lights)
    tight, u0 = ptamd.primary_cull_rects_r(cam, W, H, lo, hi, lights)
    assert loose is not None and tight is not None and len(loose) == len(tight)
    u0 = np.float32(u0)
    live = ~culled_mask(loose, W, H)
    ys, xs = np.nonzero(margin_mask(loose, tight, W, H))
    skipped = traced = 0
    for batch in range(first_batch, first_batch + n_batches):
        seeds = (np.uint64(batch) * np.uint64(H) + ys.astype(np.uint64)) * np.uint64(W) + xs.astype(np.uint64)
        u = np.maximum(np.float32(1e-38), rng_draws(seeds, 3))
        skip = (u[:, 0] >= u0) & (u[:, 2] >= u0)
        skipped += int(skip.sum())
        traced += int((~skip).sum())
    return int(live.sum()), skipped, traced
