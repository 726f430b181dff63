"""The hull faces of the sweep table (scene/small_sweep.h, csrc/sweep_walk.h
sweep_slab_hull) on the CPU.

A flat box of the table that is a face of the root box -- its flat coordinate
bitwise the root's lo or hi on that axis, its other four extents bitwise the
root's -- carries a code, and sweep_cands tests it with the slab products the
root's test formed instead of its own.  tests/sweep_hull_check.cpp compiles
the header for the host and compares, per ray, sweep_cands' leaf mask and
`none` with sweep_leaves(sweep_mask(...)), which goes through slab for every
box; the same for the table packed without codes (PT_OPT_SWEEP_HULL 0) and for
a lane riding along past a failed root test; sweep_slab_hull with slab on every
(ray, coded box); and every code with its definition by memcmp.  The rays are
test_sweep.make_rays': zero direction components (NaNs in the slab test),
origins inside the root and on face planes, rays lying in face planes.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import test_sweep

ROOT = test_sweep.ROOT
CSRC = test_sweep.CSRC
SRC = os.path.join(ROOT, "tests", "sweep_hull_check.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libsweep_hull_check.so")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
         "-I", os.path.join(ROOT, "tests")]
_LIB = None


def _sources():
    srcs = [SRC, os.path.join(CSRC, "scene", "small_sweep.cpp"), os.path.join(CSRC, "scene", "threaded_bvh.cpp")]
    deps = srcs + [os.path.join(ROOT, "tests", "sweep_check.cpp")] + [
        os.path.join(CSRC, f) for f in ("sweep_walk.h", "pt_isect.h", "pt_math.h", os.path.join("scene", "small_sweep.h"),
                                        os.path.join("scene", "threaded_bvh.h"))]
    return srcs, deps


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


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
        L.sweep_hull_check.argtypes = [F32P, sz, U32P, sz, F32P, sz, ctypes.c_int, F32P, sz, U64P, I32P,
                                       ctypes.c_char_p, sz]
        _LIB = L
    return _LIB


def hull_check(v, idx, nodes, rays):
    """(stats[12], info[5] = boxes, leaves, flat, coded by the table, n_hull) of tests/sweep_hull_check.cpp."""
    st = np.zeros(12, np.uint64)
    info = np.zeros(5, np.int32)
    err = ctypes.create_string_buffer(256)
    rays = np.ascontiguousarray(rays, np.float32)
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1)
    rc = lib().sweep_hull_check(v, v.size, idx, idx.size // 3, nodes, nodes.size // 8, 0, rays, rays.shape[0], st, info,
                                err, 256)
    assert rc == 0, (rc, err.value.decode())
    return st, [int(x) for x in info]


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


def scene(name):
    if name == "cuboid":
        v, i = cuboid()
        idx, nodes = oracle_lib.bvh_build(v, i)
        return np.ascontiguousarray(v, np.float32), idx, nodes
    return test_sweep._scene(name)


# the test_sweep.HOSTILE names: the box moved and scaled keeps its six hull faces
# (the codes compare bits, not values near the origin); the flat quad's only box is the root
MOVED_BOXES = ["box@300", "box*50", "box*0.01", "box:copies2"]
SCENES = ["box", "cuboid", "grid:2", "tri:4"] + MOVED_BOXES + ["flat_quad", "tri4:copies8"]


@pytest.mark.parametrize("name", SCENES)
def test_hull_faces_equal_slab(name):
    v, idx, nodes = scene(name)
    rays = test_sweep.make_rays(v, idx, 6000, seed=len(name) * 257 + idx.size)
    st, (boxes, leaves, flat, coded, n_hull) = hull_check(v, idx, nodes, rays)
    first = int(st[5])
    where = f"{name}: first bad ray {first}: {rays[first % len(rays)]}"
    assert leaves == idx.size // 3
    assert int(st[6]) == 0, f"{name}: codes that differ from their definition, or a table without codes that has one"
    assert coded == n_hull <= flat
    assert (int(st[0]), int(st[1])) == (0, 0), f"leaf mask / none differ from sweep_leaves(sweep_mask): {st[:2]}; {where}"
    assert int(st[2]) == 0, f"the table without codes differs from sweep_leaves(sweep_mask): {st[2]}; {where}"
    assert int(st[3]) == 0, f"the sweep past the root differs from the two passes without the early exit: {st[3]}; {where}"
    assert int(st[4]) == 0, f"sweep_slab_hull differs from slab on {int(st[4])} (ray, box) pairs; {where}"
    if name == "box" or name in MOVED_BOXES:
        assert (boxes, flat, coded) == (7, 6, 6), "the box's six face boxes are hull faces"
    if name == "flat_quad":
        assert (boxes, leaves, coded) == (1, 2, 0), "the root alone: nothing to share its products with"
    if name == "cuboid":
        assert coded >= 2, "the cuboid has hull faces"
    if name.startswith("tri"):
        assert coded == 0, "random triangles have no hull face"
    if coded:
        assert st[7] > 0, "rays whose product on a hull face's flat axis is NaN (0 * inf)"
    # coverage, so that the pass means something
    assert int(st[10]) == (1 << leaves) - 1, f"{name}: leaf bits never set in a mask: {(1 << leaves) - 1 - int(st[10]):#x}"
    assert st[8] > 0 and st[9] > 0 and st[11] > 0, "rays passing the root box, rays failing it, candidates"


def test_standalone_program():
    """The harness's own main (the program meant for host sanitizer runs)
    builds and passes: a cuboid alone (six hull faces) and the same cuboid
    beside a tilted triangle under a larger root (none)."""
    srcs, deps = _sources()
    exe = os.path.join(BUILD, "sweep_hull_check")
    if _stale(exe, deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-g", "-DSWEEP_HULL_MAIN"] + FLAGS + ["-o", exe] + srcs)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2
    assert "leaves=12 flat_boxes=6 hull_boxes=6 mask=0 none=0 plain=0 riding=0 hull=0 codes=0" in lines[0], out.stdout
    assert "leaves=13 flat_boxes=6 hull_boxes=0 mask=0 none=0 plain=0 riding=0 hull=0 codes=0" in lines[1], out.stdout
