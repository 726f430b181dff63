"""What the sweep-walk tests share, on the CPU and on the GPU: the tiny scenes
(oracle-built), the ray families, and the four host check libraries
(tests/sweep*_check.cpp) with their calls."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import native
import ptamd
import scenes
from oracle_lib import F32P, I32P, U32P, U64P
from support import TWO_LIGHTS, box_mesh, oracle_built

SOURCES = [os.path.join(native.CSRC, "scene", "small_sweep.cpp"), os.path.join(native.CSRC, "scene", "threaded_bvh.cpp")]
FLAGS = native.COMMON + ["-I", native.CSRC]
# sweep_hull, sweep_fold and sweep_cube include tests/sweep_check.cpp
FLAGS_TESTS = FLAGS + ["-I", native.TESTS]
SZ = ctypes.c_size_t
SCENE_ARGS = [F32P, SZ, U32P, SZ, F32P, SZ, ctypes.c_int]   # vertices, indices, nodes, 0


@functools.lru_cache(maxsize=None)
def lib(name):
    """tests/<name>.cpp as a shared library, with the argument types of its entry points."""
    first = name == "sweep_check"
    so = native.build(f"lib{name}.so", [os.path.join(native.TESTS, name + ".cpp")] + SOURCES,
                      ["-O2"] + (FLAGS if first else FLAGS_TESTS), shared=True)
    L = ctypes.CDLL(so)
    tail = [ctypes.c_char_p, SZ]
    if first:
        L.sweep_info.argtypes = SCENE_ARGS + [I32P] + tail
        L.sweep_check.argtypes = SCENE_ARGS + [F32P, SZ, U64P] + tail
    else:
        extra = [I32P] if name == "sweep_fold_check" else []
        getattr(L, name).argtypes = SCENE_ARGS + [F32P, SZ, U64P, I32P] + extra + tail
    return L


def run_main(name, define):
    """The check's stand-alone main (the program meant for host sanitizer runs), built with -D<define>
    and run: it must succeed; what it printed is returned."""
    exe = native.build(name, [os.path.join(native.TESTS, name + ".cpp")] + SOURCES, ["-O1", "-g", "-D" + define] + FLAGS_TESTS)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def info(v, idx, nodes):
    out = np.zeros(4, np.int32)
    err = ctypes.create_string_buffer(256)
    rc = lib("sweep_check").sweep_info(v, v.size, idx, idx.size // 3, nodes, nodes.size // 8, 0, out, err, 256)
    assert rc in (0, 2), err.value.decode()
    return rc == 0, out


def check(v, idx, nodes, rays):
    """(the scene has a sweep table, stats[8]) of tests/sweep_check.cpp."""
    st, _, rc = native.sweep_call(lib("sweep_check").sweep_check, v, idx, nodes, rays, 8, 0, accept=(0, 2))
    return rc == 0, st


def hull_check(v, idx, nodes, rays):
    """(stats[12], info[5] = boxes, leaves, flat, coded by the table, n_hull) of tests/sweep_hull_check.cpp."""
    st, inf, _ = native.sweep_call(lib("sweep_hull_check").sweep_hull_check, v, idx, nodes, rays, 12, 5)
    return st, [int(x) for x in inf]


def fold_check(v, idx, nodes, rays):
    """(stats[16], boxes, leaves, slot per leaf in visit order, flat boxes) of tests/sweep_fold_check.cpp."""
    slots = np.full(32, -1, np.int32)
    st, inf, _ = native.sweep_call(lib("sweep_fold_check").sweep_fold_check, v, idx, nodes, rays, 16, 3, extra=(slots,))
    return st, int(inf[0]), int(inf[1]), slots[:int(inf[1])].copy(), int(inf[2])


def visit_order(v, idx, nodes):
    """The triangle slot of each leaf of the scene's sweep table, in visit order."""
    return fold_check(v, idx, nodes, np.zeros((1, 8), np.float32) + np.float32(1.0))[3]


def cube_check(v, idx, nodes, rays):
    """(stats[12], info[5] = boxes, leaves, n_hull, cube, faces) of tests/sweep_cube_check.cpp."""
    st, inf, _ = native.sweep_call(lib("sweep_cube_check").sweep_cube_check, v, idx, nodes, rays, 12, 5)
    return st, [int(x) for x in inf]


# Tiny scenes away from the origin-centred, unit-sized, non-degenerate ones:
# name -> (vertices, indices) before the BVH build.
HOSTILE = {
    "box@300": lambda: (scenes.transformed(box_mesh()[0], 1.0, (300, 300, -300)), box_mesh()[1]),
    "box*50": lambda: (scenes.transformed(box_mesh()[0], 50.0, (0, 0, 0)), box_mesh()[1]),
    "box*0.01": lambda: (scenes.transformed(box_mesh()[0], 0.01, (0, 0, 0)), box_mesh()[1]),
    "box:copies2": lambda: scenes.coincident_copies(*box_mesh(), 2),
    "tri4:copies8": lambda: scenes.coincident_copies(*scenes.random_triangles(4), 8),
    "flat_quad": scenes.flat_quad,
    "tri8:degenerate": lambda: scenes.with_degenerates(*scenes.random_triangles(8)),
}
# (distinct boxes, leaves) of the tables where the scene fixes them
HOSTILE_TABLES = {"box:copies2": (7, 24), "tri4:copies8": (7, 32), "flat_quad": (1, 2), "tri8:degenerate": (15, 8)}
# the box moved and scaled keeps its six hull faces (the codes compare bits, not values near the origin)
MOVED_BOXES = ["box@300", "box*50", "box*0.01", "box:copies2"]
CUBOIDS = {
    "cuboid": scenes.cuboid,
    "cuboid-open": scenes.open_cuboid,
    "cuboid+tri": scenes.cuboid_with_inner_triangle,
    "cuboids-stacked": scenes.stacked_cuboids,
}
MESHES = dict(HOSTILE, box=box_mesh, **CUBOIDS)
# the makers support.scene needs for the GPU sweep tests' scenes
GPU_MAKERS = dict(CUBOIDS, **{"cuboid-inward": scenes.cuboid_inward})


@functools.lru_cache(maxsize=None)
def scene(name):
    """(vertices, indices, nodes) from the oracle's build: a name of MESHES, "grid:N" or "tri:N"."""
    if name in MESHES:
        return oracle_built(*MESHES[name]())
    kind, n = name.split(":")
    return oracle_built(*(scenes.grid_mesh(int(n)) if kind == "grid" else scenes.random_triangles(int(n))))


def unit(a):
    a = np.asarray(a, np.float32)
    return (a / np.sqrt((a * a).sum(-1, keepdims=True))).astype(np.float32)


def make_rays(v, idx, n, seed):
    """n x 8 float32 {o, d, shadow limit, 0}: a mix of ray families."""
    rng = np.random.default_rng(seed)
    V = v.reshape(-1, 3)
    lo, hi = V.min(0), V.max(0)
    ext = np.maximum(hi - lo, np.float32(0.05))
    k = n // 6
    fam = []
    # 1. origins around the scene, random directions
    fam.append((rng.uniform(lo - ext, hi + ext, (k, 3)), unit(rng.normal(size=(k, 3)))))
    # 2. origins inside the root box, random directions
    fam.append((rng.uniform(lo, hi, (k, 3)), unit(rng.normal(size=(k, 3)))))
    # 3. from outside towards points on the triangles
    P = V[idx.reshape(-1, 3)]
    t = rng.integers(0, len(P), k)
    b = rng.dirichlet([1, 1, 1], k).astype(np.float32)
    # (placed by the scene's bounds: (0.3, 0.2, 3.0) for the box's [-1, 1]^3)
    o = np.tile(((lo + hi) / 2 + ext.max() * np.float32([0.15, 0.1, 1.5])).astype(np.float32), (k, 1))
    fam.append((o, unit((P[t] * b[:, :, None]).sum(1) - o)))
    # 4. one or two zero direction components, origins anywhere (half of them inside)
    o = rng.uniform(lo - ext * 0.5, hi + ext * 0.5, (k, 3))
    d = unit(rng.normal(size=(k, 3)))
    d[np.arange(k), rng.integers(0, 3, k)] = 0.0
    two = rng.random(k) < 0.3
    d[two, (rng.integers(0, 3, k))[two]] = 0.0
    d[(d == 0).all(1)] = np.float32([0, 0, -1])
    fam.append((o, unit(d)))
    # 5. origin on a face plane of the root box or on a vertex coordinate, direction free
    o = rng.uniform(lo, hi, (k, 3))
    ax = rng.integers(0, 3, k)
    pick = V[rng.integers(0, len(V), k), ax]
    side = rng.random(k)
    o[np.arange(k), ax] = np.where(side < 0.33, lo[ax], np.where(side < 0.66, hi[ax], pick))
    fam.append((o, unit(rng.normal(size=(k, 3)))))
    # 6. rays lying in such a plane: the origin's coordinate on it, that direction component zero
    k6 = n - 5 * k
    o = rng.uniform(lo - ext * 0.5, hi + ext * 0.5, (k6, 3))
    ax = rng.integers(0, 3, k6)
    pick = V[rng.integers(0, len(V), k6), ax]
    side = rng.random(k6)
    o[np.arange(k6), ax] = np.where(side < 0.33, lo[ax], np.where(side < 0.66, hi[ax], pick))
    d = unit(rng.normal(size=(k6, 3)))
    d[np.arange(k6), ax] = 0.0
    fam.append((o, unit(d)))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = np.concatenate([f[0] for f in fam]).astype(np.float32)
    rays[:, 3:6] = np.concatenate([f[1] for f in fam]).astype(np.float32)
    rays[:, 6] = rng.uniform(0.0, 4.0, n).astype(np.float32)
    return rays


def _ulps(x, k):
    """x moved by k units in the last place (k of either sign)."""
    x = np.asarray(x, np.float32).copy()
    for _ in range(int(np.max(np.abs(k)))):
        step = np.where(k > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        x = np.where(k != 0, np.nextafter(x, step), x).astype(np.float32)
        k = k - np.sign(k)
    return x


def plane_rays(lo, hi, n, seed):
    """n x 8 rays about the root box's six planes: (a) the origin on a plane, the direction component on that axis
    0, -0 or a subnormal of either sign; (b) the origin 1-3 ulp to either side of a plane; (c) axis-parallel rays,
    their other components +-0, from inside, from a plane and from outside."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ext = hi - lo
    tiny = np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-41, -1e-41, 1.1e-38, -1.1e-38])   # 0, -0 and subnormals
    rays = np.zeros((n, 8), np.float32)
    o = rng.uniform(lo - ext * 0.25, hi + ext * 0.25, (n, 3)).astype(np.float32)
    inside = rng.random(n) < 0.5
    o[inside] = rng.uniform(lo, hi, (int(inside.sum()), 3)).astype(np.float32)
    d = unit(rng.normal(size=(n, 3)))
    ax = rng.integers(0, 3, n)
    plane = np.where(rng.random(n) < 0.5, lo[ax], hi[ax]).astype(np.float32)
    fam = np.arange(n) % 3
    row = np.arange(n)
    a, b, c = fam == 0, fam == 1, fam == 2
    o[row[a], ax[a]] = plane[a]
    d[row[a], ax[a]] = tiny[rng.integers(0, len(tiny), int(a.sum()))]
    k = rng.integers(1, 4, n) * np.where(rng.random(n) < 0.5, 1, -1)
    o[row[b], ax[b]] = _ulps(plane[b], k[b])
    zero_too = b & (rng.random(n) < 0.25)
    d[row[zero_too], ax[zero_too]] = tiny[rng.integers(0, 2, int(zero_too.sum()))]
    d[c] = tiny[rng.integers(0, 2, (int(c.sum()), 3))]
    d[row[c], ax[c]] = np.where(rng.random(int(c.sum())) < 0.5, 1.0, -1.0)
    on_plane = c & (rng.random(n) < 0.4)
    other = (ax + 1 + rng.integers(0, 2, n)) % 3
    o[row[on_plane], other[on_plane]] = np.where(rng.random(int(on_plane.sum())) < 0.5, lo[other[on_plane]],
                                                 hi[other[on_plane]])
    rays[:, 0:3], rays[:, 3:6] = o, d
    rays[:, 6] = rng.uniform(0.0, 4.0, n).astype(np.float32)
    return rays


CENTRE = (scenes.CUBOID_LO.astype(np.float64) + scenes.CUBOID_HI) * 0.5


def _ubo(pos, at, fov=60.0, up=(0, 1, 0)):
    d = np.asarray(at, np.float64) - np.asarray(pos, np.float64)
    ubo = np.zeros(16, np.float32)
    ubo[0:3] = pos
    ubo[4:7] = d / np.linalg.norm(d)
    ubo[8:11] = up
    ubo[12] = fov
    return ubo


def _light(pos, at, size):
    d = np.asarray(at, np.float64) - np.asarray(pos, np.float64)
    return ptamd.pack_light(pos, d / np.linalg.norm(d), [10, 10, 10], size)


# the GPU hull test's cases (the cube test runs them too): name -> (scene, camera, lights, hull faces expected)
HULL_CASES = {
    "box": ("box", scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT, True),
    "cuboid": ("cuboid", _ubo(CENTRE + [1.5, 1.25, 3.5], CENTRE, 40.0),
               np.concatenate([_light(CENTRE + [0.5, 2.0, 1.0], CENTRE, [2.0, 2.0]),
                               _light(CENTRE + [2.5, 0.25, 2.0], CENTRE, [1.0, 1.0])]), True),
    "cuboid-inside": ("cuboid-inward", _ubo(CENTRE + [0.0, 0.0, 0.5], CENTRE + [0.25, 0.125, -1.0], 90.0),
                      _light(CENTRE + [0.0, 0.2, 0.0], CENTRE + [0.0, -1.0, 0.0], [0.2, 0.2]), True),
    "grid:2": ("grid:2", scenes.camera((0.0, 0.0, 3.0)), TWO_LIGHTS, False),
    "tri:4": ("tri:4", scenes.camera((0.0, 0.0, 3.0), fov=50.0), TWO_LIGHTS, False),
}
