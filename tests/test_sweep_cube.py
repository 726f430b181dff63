"""The cube table of the sweep walk (scene/small_sweep.h SmallSweep::cube,
csrc/sweep_walk.h sweep_cands_cube) on the CPU.

A table in which every box other than the root is a hull face of it -- no
general box, every flat box coded, one box per (axis, code): the box, a cuboid,
a cuboid without one face -- is walked straight-line: the root's six products,
its test, then the six faces with their axis and code fixed at compile time and
their under words handed in.  tests/sweep_cube_check.cpp compiles the header
for the host and compares, per ray, sweep_cands_cube's leaf mask and `none`
with sweep_cands<true> (the walk it replaces) and with
sweep_leaves(sweep_mask(...)), which goes through slab for every box; the
predicate with its definition; cube_under[] and cube_all with under[] by value.
At least 10^6 rays per scene: test_sweep.make_rays' families (origins inside
the root and on face planes, zero direction components, rays lying in face
planes) and, on the root's planes, direction components of 0, -0 and
subnormals, origins a few ulp to either side, and axis-parallel rays.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import scenes
import test_sweep
import test_sweep_hull

ROOT = test_sweep.ROOT
CSRC = test_sweep.CSRC
SRC = os.path.join(ROOT, "tests", "sweep_cube_check.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libsweep_cube_check.so")
FLAGS = test_sweep_hull.FLAGS
N_RAYS = 1 << 20
_LIB = None


def _sources():
    srcs = [SRC, os.path.join(CSRC, "scene", "small_sweep.cpp"), os.path.join(CSRC, "scene", "threaded_bvh.cpp")]
    deps = srcs + [os.path.join(ROOT, "tests", "sweep_check.cpp")] + [
        os.path.join(CSRC, f) for f in ("sweep_walk.h", "pt_isect.h", "pt_math.h", os.path.join("scene", "small_sweep.h"),
                                        os.path.join("scene", "threaded_bvh.h"))]
    return srcs, deps


_stale = test_sweep_hull._stale


def lib():
    global _LIB
    if _LIB is None:
        srcs, deps = _sources()
        if _stale(SO, deps):
            os.makedirs(BUILD, exist_ok=True)
            subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", SO] + srcs)
        L = ctypes.CDLL(SO)
        F32P = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
        U32P = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
        U64P = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
        I32P = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
        sz = ctypes.c_size_t
        L.sweep_cube_check.argtypes = [F32P, sz, U32P, sz, F32P, sz, ctypes.c_int, F32P, sz, U64P, I32P,
                                       ctypes.c_char_p, sz]
        _LIB = L
    return _LIB


def cube_check(v, idx, nodes, rays):
    """(stats[12], info[5] = boxes, leaves, n_hull, cube, faces) of tests/sweep_cube_check.cpp."""
    st = np.zeros(12, np.uint64)
    info = np.zeros(5, np.int32)
    err = ctypes.create_string_buffer(256)
    rays = np.ascontiguousarray(rays, np.float32)
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1)
    rc = lib().sweep_cube_check(v, v.size, idx, idx.size // 3, nodes, nodes.size // 8, 0, rays, rays.shape[0], st, info,
                                err, 256)
    assert rc == 0, (rc, err.value.decode())
    return st, [int(x) for x in info]


LO, HI = test_sweep_hull.CUBOID_LO, test_sweep_hull.CUBOID_HI


def open_cuboid(outward=True):
    """The cuboid without its y hi face (triangles 6 and 7): 10 triangles, the root box still [LO, HI]."""
    v, i = test_sweep_hull.cuboid(outward=outward)
    return v, np.delete(i.reshape(-1, 3), [6, 7], axis=0).reshape(-1)


def cuboid_with_inner_triangle():
    """The cuboid and one tilted triangle inside it: the triangle's box is a general one."""
    v, i = test_sweep_hull.cuboid()
    c, e = (LO + HI) * np.float32(0.5), HI - LO
    tri = np.float32([c + e * [-0.25, -0.125, 0.125], c + e * [0.25, -0.25, -0.125], c + e * [0.0, 0.25, 0.25]])
    return np.concatenate([v, tri.reshape(-1)]), np.concatenate([i, np.uint32([8, 9, 10])])


def stacked_cuboids():
    """Two cuboids, the second on top of the first (y): no face of either spans the root box of both."""
    v, i = test_sweep_hull.cuboid()
    up = v.reshape(-1, 3) + np.float32([0.0, HI[1] - LO[1], 0.0])
    return np.concatenate([v, up.reshape(-1)]).astype(np.float32), np.concatenate([i, i + np.uint32(8)])


MESHES = {
    "cuboid": test_sweep_hull.cuboid,
    "cuboid-open": open_cuboid,
    "cuboid+tri": cuboid_with_inner_triangle,
    "cuboids-stacked": stacked_cuboids,
}
CUBE_SCENES = {"box": 6, "cuboid": 6, "cuboid-open": 5}          # name -> faces
OTHER_SCENES = ["grid:2", "tri:4", "cuboid+tri", "cuboids-stacked"]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in MESHES:
        v, i = MESHES[name]()
        idx, nodes = oracle_lib.bvh_build(np.ascontiguousarray(v, np.float32), i)
        return np.ascontiguousarray(v, np.float32), idx, nodes
    return test_sweep._scene(name)


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
    d = test_sweep._unit(rng.normal(size=(n, 3)))
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


@functools.lru_cache(maxsize=None)
def rays_of(name):
    v, idx, _ = scene(name)
    V = v.reshape(-1, 3)
    half = N_RAYS // 2
    return np.concatenate([test_sweep.make_rays(v, idx, half, seed=len(name) * 263 + idx.size),
                           plane_rays(V.min(0), V.max(0), N_RAYS - half, seed=len(name) * 911 + 7)])


@pytest.mark.parametrize("name", list(CUBE_SCENES))
def test_cube_walk_equals_hull_walk_and_two_passes(name):
    v, idx, nodes = scene(name)
    rays = rays_of(name)
    assert len(rays) >= 10 ** 6
    st, (boxes, leaves, n_hull, cube, faces) = cube_check(v, idx, nodes, rays)
    first = int(st[3])
    where = f"{name}: first bad ray {first}: {rays[first % len(rays)]}"
    print(f"{name}: boxes {boxes} leaves {leaves} faces {faces}; differing masks {int(st[0])}, none {int(st[1])}, "
          f"two-pass {int(st[2])}; root pass {int(st[6])} fail {int(st[7])}, NaN products {int(st[10])}")
    assert leaves == idx.size // 3
    assert int(st[4]) == 0, f"{name}: SmallSweep::cube differs from its definition"
    assert cube == 1 and faces == CUBE_SCENES[name] and boxes == 1 + faces and n_hull == faces
    assert int(st[5]) == 0, f"{name}: cube_under[] / cube_all differ from under[]"
    assert int(st[11]) == len(rays)
    assert (int(st[0]), int(st[1])) == (0, 0), f"leaf mask / none differ from sweep_cands<true>: {st[:2]}; {where}"
    assert int(st[2]) == 0, f"leaf mask / none differ from sweep_leaves(sweep_mask): {st[2]}; {where}"
    # coverage, so that the pass means something
    assert int(st[8]) == (1 << leaves) - 1, f"{name}: leaf bits never set in a mask: {(1 << leaves) - 1 - int(st[8]):#x}"
    assert st[6] > 0 and st[7] > 0 and st[9] > 0, "rays passing the root box, rays failing it, candidates"
    assert st[10] > 0, "rays with a NaN among the root's products (0 * inf)"


@pytest.mark.parametrize("name", OTHER_SCENES)
def test_other_tables_are_not_cube_tables(name):
    v, idx, nodes = scene(name)
    st, (boxes, leaves, n_hull, cube, faces) = cube_check(v, idx, nodes, np.ones((1, 8), np.float32))
    assert leaves == idx.size // 3
    assert int(st[4]) == 0, f"{name}: SmallSweep::cube differs from its definition"
    assert cube == 0 and faces == 0, f"{name}: {boxes} boxes, {n_hull} coded"
    assert int(st[5]) == 0, f"{name}: cube_under[] / cube_all are not zero without a cube table"
    assert int(st[11]) == 0
    if name == "cuboid+tri":
        assert n_hull == 6 and boxes > 7, "the six faces keep their codes beside the general box"


def _program(exe, extra):
    srcs, deps = _sources()
    if _stale(exe, deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-g", "-DSWEEP_CUBE_MAIN"] + extra + FLAGS + ["-o", exe] + srcs)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 3, out.stdout + out.stderr
    assert "boxes=7 leaves=12 hull_boxes=6 cube=1 faces=6 mask=0 none=0 two_pass=0 predicate=0 under=0" in lines[0], out.stdout
    assert "boxes=6 leaves=10 hull_boxes=5 cube=1 faces=5 mask=0 none=0 two_pass=0 predicate=0 under=0" in lines[1], out.stdout
    assert "boxes=8 leaves=13 hull_boxes=6 cube=0 faces=0 mask=0 none=0 two_pass=0 predicate=0 under=0" in lines[2], out.stdout


def test_standalone_program():
    """The harness's own main builds and passes: a cuboid (six faces), the same without one face (five), and the
    whole one beside a triangle inside it (no cube table)."""
    _program(os.path.join(BUILD, "sweep_cube_check"), [])
