"""What the ray-query tests share, on the CPU and on the GPU: the scenes, the
rays of each with the oracle's answers (computed once per process, read-only),
the occlusion limits drawn around those answers, hostile rays, and an
independent numpy float32 Moller-Trumbore."""
import functools

import numpy as np

import oracle_lib
import ptamd
import support
from sweep_support import make_rays, plane_rays

SCENES = ["box", "sphere", "grid:8", "tri:2000"]   # box.obj, displaced_sphere(3), grid_mesh(8), random_triangles(2000)
N_MAKE, N_PLANE = 3000, 600
# make_rays seeds under which every family of every scene has hits and misses (test_rays.py asserts it)
SEEDS = {"box": 1, "sphere": 2, "grid:8": 3, "tri:2000": 4}
F32 = np.float32


def families(n=N_MAKE):
    """The slices of make_rays' six families in its n rays."""
    k = n // 6
    return [slice(j * k, (j + 1) * k if j < 5 else n) for j in range(6)]


def oracle_answers(scene, rays):
    """(hit, t, n) of oracle_lib.trace per ray; t = 1e30 and n = 0 on a miss."""
    v, i, n = scene
    hit = np.zeros(len(rays), bool)
    t = np.full(len(rays), 1e30, F32)
    nr = np.zeros((len(rays), 3), F32)
    for k, r in enumerate(rays):
        h, tt, _, nn, _ = oracle_lib.trace(v, i, n, r[0:3], r[3:6])
        if h:
            hit[k], t[k], nr[k] = True, F32(tt), nn
    return hit, t, nr


def limits_around(t, base):
    """One limit per ray, cycling: the ray's own t, its two float neighbours, 0, -1, inf, NaN, the drawn one."""
    t = np.asarray(t, F32)
    k = np.arange(len(t)) % 8
    below, above = np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf))
    choices = [t, below, above, np.zeros_like(t), np.full_like(t, -1), np.full_like(t, np.inf), np.full_like(t, np.nan),
               np.asarray(base, F32)]
    return np.choose(k, choices).astype(F32)


def grid_edge_rays(n=8):
    """Rays at the shared edges and vertices of grid_mesh(n)'s quads, where two to six coplanar triangles are
    hit at one t: straight down at every grid vertex and at the edge midpoints (zero direction components: the
    exact walk), and slanted ones, no component zero (the wide walk where there is one), through a point of every
    x edge at the three heights the quads lie at.  make_rays' in-plane family never hits this mesh."""
    rows = []
    for a in range(n + 1):
        for b in range(n + 1):
            x, y, s = -1 + 2 * a / n, -1 + 2 * b / n, 2 / n
            rows.append([x, y, 1, 0, 0, -1])
            rows.append([x + s / 2 if a < n else x, y, 1, 0, 0, -1])
            for d in ([0.5, 0.5, -0.70710678], [0.25, 0.5, -0.82915619]):
                for z in (-0.25, 0.0, 0.25):
                    rows.append([x - d[0], y + s / 4 - d[1], z - d[2]] + d)
    rays = np.zeros((len(rows), 8), F32)
    rays[:, 0:6] = np.array(rows, np.float64).astype(F32)
    rays[:, 6] = F32(1e30)
    return rays


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(scene, rays, hit, t, n, any_rays, occluded) of a scene: 3000 make_rays and 600 plane_rays rays
    (then, for the grid, grid_edge_rays), the oracle's closest hits, the same rays with limits around those
    hits and the occlusion they imply."""
    scene = support.scene(name)
    v, i, _ = scene
    V = v.reshape(-1, 3)
    rays = np.concatenate([make_rays(v, i, N_MAKE, SEEDS[name]), plane_rays(V.min(0), V.max(0), N_PLANE, SEEDS[name] + 10)]
                          + ([grid_edge_rays(8)] if name == "grid:8" else []))
    hit, t, n = oracle_answers(scene, rays)
    any_rays = rays.copy()
    any_rays[:, 6] = limits_around(t, rays[:, 6])
    with np.errstate(invalid="ignore"):
        occluded = (hit & ~(t >= any_rays[:, 6])).astype(np.uint32)   # the least accepted t decides
    out = dict(scene=scene, rays=rays, hit=hit, t=t, n=n, any_rays=any_rays, occluded=occluded)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_answers(name):
    """(closest records, occlusion words) of pt_trace_rays_host on case(name)'s rays."""
    c = case(name)
    hits = ptamd.trace_rays_host(*c["scene"], c["rays"], ptamd.RAYS_CLOSEST)
    occ = ptamd.trace_rays_host(*c["scene"], c["any_rays"], ptamd.RAYS_ANY)
    hits.setflags(write=False)
    occ.setflags(write=False)
    return hits, occ


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F32)


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F32)


def moller_trumbore(scene, rays, tri):
    """(accepted, t, u, v) of intersectTriangle for ray k against triangle indices[3*tri[k] ..] of the uploaded
    arrays, in numpy float32, one rounding per operation, the shader's order (raytrace_comp.comp:114-157)."""
    v, idx, _ = scene
    V = np.asarray(v, F32).reshape(-1, 3)
    T = np.asarray(idx).reshape(-1, 3)[np.asarray(tri)]
    v0, v1, v2 = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    o, d = np.asarray(rays[:, 0:3], F32), np.asarray(rays[:, 3:6], F32)
    with np.errstate(all="ignore"):
        e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
        p = _cross(d, e2)
        det = _dot(e1, p)
        inv = (F32(1.0) / det).astype(F32)
        s = (o - v0).astype(F32)
        u = (inv * _dot(s, p)).astype(F32)
        q = _cross(s, e1)
        w = (inv * _dot(d, q)).astype(F32)
        t = (inv * _dot(e2, q)).astype(F32)
        ok = ~(np.abs(det) < F32(0.000001)) & ~((u < 0) | (u > 1)) & ~((w < 0) | ((u + w).astype(F32) > 1)) & ~(t <= F32(0.000001))
    return ok, t, u, w


def ties(scene, rays, t_best):
    """Rays at least two of whose triangles are accepted at exactly the winning t."""
    v, idx, _ = scene
    nt = np.asarray(idx).size // 3
    count = np.zeros(len(rays), int)
    for tri in range(nt):
        ok, t, _, _ = moller_trumbore(scene, rays, np.full(len(rays), tri))
        count += ok & (support.bits(t) == support.bits(t_best))
    return count >= 2


def hostile_rays(scene):
    """Rays no renderer would cast, device against host on every one: NaN and infinite origins and directions,
    the zero direction, -0 and subnormal components, |d| = 1e-3 and 1e3, origins at 1e15 and 1e20, limits NaN,
    negative and infinite.  Returns (rays, rows of the non-unit rays, rows of the zero-component rays)."""
    v, idx, _ = scene
    V = np.asarray(v, F32).reshape(-1, 3)
    P = V[np.asarray(idx).reshape(-1, 3)].mean(1).astype(F32)   # triangle centroids
    lo, hi = V.min(0), V.max(0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    rng = np.random.default_rng(5)
    rows = []

    def add(o, d, limit=1e30):
        rows.append(np.concatenate([np.asarray(o, F32), np.asarray(d, F32), F32([limit, 0])]))
        return len(rows) - 1

    nan, inf = np.nan, np.inf
    for bad in (nan, inf, -inf):
        for a in range(3):
            o, d = c + [0.1, 0.2, 2 * ext], np.array([0.0, 0.0, -1.0])
            o2 = o.copy()
            o2[a] = bad
            add(o2, d)
            d2 = np.array([0.3, -0.2, -1.0])
            d2[a] = bad
            add(o, d2)
    add(c, [0, 0, 0])
    add(c + [0, 0, 2 * ext], [0, 0, 0])
    scaled, zero = [], []
    targets = P[rng.integers(0, len(P), 48)]
    for k, p in enumerate(targets):
        o = (c + rng.normal(size=3) * 0.3 + [0, 0, 2 * ext]).astype(F32)
        d = (p - o).astype(np.float64)
        d /= np.linalg.norm(d)
        # |d| = 1e-3 and 1e3: the exact walk, t scales
        scaled.append(add(o, d * (1e-3 if k % 2 else 1e3), limit=[1e30, 0.5, nan, -1.0][k % 4]))
    for k, p in enumerate(targets[:24]):
        # towards a centroid along an axis: two zero components, written 0, -0 or subnormal
        a = k % 3
        o = p.copy()
        o[a] = hi[a] + ext
        d = np.array([[0.0, -0.0, 1e-45, -1e-41][(k + j) % 4] for j in range(3)], F32)
        d[a] = -1.0
        zero.append(add(o, d, limit=[inf, -inf, nan, 0.0, -1.0, ext][k % 6]))
    for big in (1e15, 1e20, -1e20):
        for a in range(3):
            o = c.astype(np.float64).copy()
            o[a] = big
            d = np.zeros(3)
            d[a] = -np.sign(big)
            add(o, d)
            add(o, (c + [0.01, 0.02, 0.03] - o) / np.linalg.norm(c - o))
    for limit in (nan, -1.0, inf, -inf, 0.0):   # ordinary rays under every odd limit
        for p in targets[:6]:
            o = (c + [0.2, 0.1, 2 * ext]).astype(F32)
            d = (p - o).astype(np.float64)
            add(o, d / np.linalg.norm(d), limit=limit)
    return np.ascontiguousarray(np.stack(rows), F32), np.array(scaled), np.array(zero)
