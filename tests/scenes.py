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


# three different extents, translated off the origin: no two of its six plane values coincide
CUBOID_LO = np.float32([0.375, -1.25, 2.0])
CUBOID_HI = np.float32([1.125, -0.75, 3.5])


def cuboid(lo=CUBOID_LO, hi=CUBOID_HI, outward=True):
    """(vertices, indices) of the cuboid [lo, hi]: 8 vertices, 12 triangles, their geometric normals
    pointing out of it (or, for a view from inside, into it)."""
    v = np.float32([[hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]] for i in range(8)])
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    idx = np.uint32([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    if outward:
        idx = idx[:, [0, 2, 1]]
    return v.reshape(-1), idx.reshape(-1)


def cuboid_inward():
    return cuboid(outward=False)


def open_cuboid(outward=True):
    """The cuboid without its y hi face (triangles 6 and 7): 10 triangles, the root box still [CUBOID_LO, CUBOID_HI]."""
    v, i = cuboid(outward=outward)
    return v, np.delete(i.reshape(-1, 3), [6, 7], axis=0).reshape(-1)


def cuboid_with_inner_triangle():
    """The cuboid and one tilted triangle inside it: the triangle's box is a general one."""
    v, i = cuboid()
    c, e = (CUBOID_LO + CUBOID_HI) * np.float32(0.5), CUBOID_HI - CUBOID_LO
    tri = np.float32([c + e * [-0.25, -0.125, 0.125], c + e * [0.25, -0.25, -0.125], c + e * [0.0, 0.25, 0.25]])
    return np.concatenate([v, tri.reshape(-1)]), np.concatenate([i, np.uint32([8, 9, 10])])


def stacked_cuboids():
    """Two cuboids, the second on top of the first (y): no face of either spans the root box of both."""
    v, i = cuboid()
    up = v.reshape(-1, 3) + np.float32([0.0, CUBOID_HI[1] - CUBOID_LO[1], 0.0])
    return np.concatenate([v, up.reshape(-1)]).astype(np.float32), np.concatenate([i, i + np.uint32(8)])


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


# Scenes away from the [-1, 1]^3 most cases live in, for the wide walk.  The
# cull bound's terms grow with |o - v0|, with the edge lengths and with the
# largest coefficients below a node (wide_bvh.cpp: wide_tri_coeffs,
# node_cull_consts), and the 64-byte nodes' 8-bit grid is rounded outward from
# each node's own origin and scale.
WIDE_HOSTILE = {
    "cloud_far": lambda: (transformed(random_triangles(20000, seed=7)[0], 1.0, (1000, -500, 2000)),
                          random_triangles(20000, seed=7)[1]),
    "sphere_at_300": lambda: (transformed(displaced_sphere(3)[0], 1.0, (300, 300, -300)), displaced_sphere(3)[1]),
    "sphere_x50": lambda: (transformed(displaced_sphere(3)[0], 50.0, (0, 0, 0)), displaced_sphere(3)[1]),
    "sphere_x0.05": lambda: (transformed(displaced_sphere(3)[0], 0.05, (0, 0, 0)), displaced_sphere(3)[1]),
    "floor_and_cloud": floor_and_cloud,
    "coincident_x6": lambda: coincident_copies(*displaced_sphere(2), 6),
    "degenerates": lambda: with_degenerates(*random_triangles(3000, seed=8, spread=0.5, size=0.02)),
}
