"""Deterministic test/bench scenes and the reference's fixed inputs."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX_OBJ = os.path.join(ROOT, "tests", "golden", "box.obj")

# Camera.cpp:4-10 / Camera.h:34-36 default orbit camera as the std140 UBO.
DEFAULT_CAMERA = np.array([0, 0, 5, 0, 0, 0, -1, 0, 0, 1, 0, 0, 60, 0, 0, 0], np.float32)
# VulkanRayTracer.cpp:149-162 light, packed as Light.cpp:16-33 (normal already unit).
REFERENCE_LIGHT = np.array([0, 2, 0, 0, 0, -1, 0, 0, 10, 10, 10, 0, 2.5, 2.5, 0, 0], np.float32)


def camera(pos, up=(0, 1, 0), fov=60.0):
    """UBO for a camera at `pos` looking at the origin (Camera::getDirection)."""
    p = np.array(pos, np.float64)
    d = (0.0 - p) / np.linalg.norm(p)
    ubo = np.zeros(16, np.float32)
    ubo[0:3] = p
    ubo[4:7] = d
    ubo[8:11] = up
    ubo[12] = fov
    return ubo


def transformed(v, scale, offset):
    """Vertices `v * scale + offset`, computed in float64 and rounded to float32."""
    p = np.asarray(v, np.float64).reshape(-1, 3) * float(scale) + np.asarray(offset, np.float64)
    return p.astype(np.float32).reshape(-1)


def transformed_camera(ubo, scale, offset):
    """The camera UBO that sees `transformed(v, scale, offset)` from where `ubo`
    sees `v`: the position moves, direction, up and fov stay (the shader's
    aperture 0.02 and focal distance 3 do not scale, so only the blur differs)."""
    out = np.array(ubo, np.float32)
    out[0:3] = (np.asarray(ubo[0:3], np.float64) * float(scale) + np.asarray(offset, np.float64)).astype(np.float32)
    return out


def transformed_light(light16, scale, offset):
    """The packed light moved with the scene: position moved, size times scale,
    intensity times scale^2 (the irradiance at the moved surface stays)."""
    out = np.array(light16, np.float32)
    out[0:3] = (np.asarray(light16[0:3], np.float64) * float(scale) + np.asarray(offset, np.float64)).astype(np.float32)
    out[8:11] = (np.asarray(light16[8:11], np.float64) * float(scale) ** 2).astype(np.float32)
    out[12:14] = (np.asarray(light16[12:14], np.float64) * float(scale)).astype(np.float32)
    return out


def coincident_copies(v, i, copies):
    """The index list `copies` times over the same vertices, odd copies with
    flipped winding: every ray that hits ties in t across `copies` triangles,
    and the winner's normal depends on the visit order."""
    t = np.asarray(i, np.uint32).reshape(-1, 3)
    parts = [t if c % 2 == 0 else t[:, [0, 2, 1]] for c in range(copies)]
    return np.asarray(v, np.float32).reshape(-1).copy(), np.concatenate(parts).astype(np.uint32).reshape(-1)


def floor_and_cloud():
    """5,000 small triangles over a two-triangle floor 40 units across (y = -0.6,
    geometric normal +y): triangle sizes three orders of magnitude apart in one
    tree.  The floor's coefficients exceed the cull bound, so every wide node
    above it gives up culling while its siblings still cull."""
    v, i = random_triangles(5000, seed=3, spread=0.5, size=0.01)
    quad = np.array([(-20, -0.6, -20), (-20, -0.6, 20), (20, -0.6, 20), (20, -0.6, -20)], np.float32)
    base = v.size // 3
    qi = np.array([0, 1, 2, 0, 2, 3], np.uint32) + np.uint32(base)
    return np.concatenate([v, quad.reshape(-1)]).astype(np.float32), np.concatenate([i, qi]).astype(np.uint32)


def with_degenerates(v, i):
    """Every 5th triangle with two equal vertices (a segment), every 7th
    collapsed to a point: zero-extent leaf boxes and det = 0."""
    t = np.array(i, np.uint32).reshape(-1, 3)
    k = np.arange(len(t))
    t[k % 5 == 0, 1] = t[k % 5 == 0, 0]
    t[k % 7 == 0, 1] = t[k % 7 == 0, 0]
    t[k % 7 == 0, 2] = t[k % 7 == 0, 0]
    return np.asarray(v, np.float32).reshape(-1).copy(), t.reshape(-1)


def flat_quad():
    """Two triangles in z = 0 (geometric normal +z): the root box has zero thickness."""
    v = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], np.float32)
    return v.reshape(-1), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def random_triangles(n, seed=42, spread=1.0, size=0.01):
    """SURVEY.md §8d config 5 generator: centroids ~U[-1,1]^3, vertex offsets
    ~U[-size,size]^3, unshared vertices."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3)).astype(np.float32)
    off = rng.uniform(-size, size, (n, 3, 3)).astype(np.float32)
    v = (c + off).astype(np.float32).reshape(-1)
    idx = np.arange(3 * n, dtype=np.uint32)
    return v, idx


def grid_mesh(n=8, seed=0):
    """Axis-aligned quads on a grid: many equal centroid keys, exercising the
    unstable sort's tie order."""
    rng = np.random.default_rng(seed)
    verts, idx = [], []
    for i in range(n):
        for j in range(n):
            z = float(rng.integers(0, 3)) * 0.25 - 0.25
            base = len(verts)
            x0, y0 = -1 + 2 * i / n, -1 + 2 * j / n
            x1, y1 = x0 + 2 / n, y0 + 2 / n
            verts += [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(verts, np.float32).reshape(-1), np.array(idx, np.uint32)


def displaced_sphere(subdiv=5, seed=3):
    """Stand-in for the missing Sylveon.obj: an
    icosphere with radial noise — deep BVH, divergent secondary rays."""
    t = (1.0 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
         (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
         (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]

        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = nf
    V = np.array(V)
    rng = np.random.default_rng(seed)
    r = 1.0 + 0.08 * rng.standard_normal(len(V))
    V = (V * r[:, None]).astype(np.float32)
    return V.reshape(-1), np.array(F, np.uint32).reshape(-1)
