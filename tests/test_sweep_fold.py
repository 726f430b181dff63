"""The one-pass sweep (csrc/sweep_walk.h sweep_cands: each box's record carries
the leaves it guards) against its two-pass restatement and the threaded walk,
on the CPU.

tests/sweep_fold_check.cpp compiles the header for the host and, from one
packed table, compares per ray: the leaf mask and `none` of sweep_cands with
those of sweep_leaves(sweep_mask(...)); the sweep past the root's test with
the two passes run without the early exit (what a lane computes that fails
the root while another lane of its wave passes); the closest hit and the
shadow answer taken from the new mask with the threaded walk's, bit for bit.
It also checks every box's under word against its definition from need[],
the table's order (root, general, x-, y-, z-flat boxes) against the boxes, and
the flat loops' slab test against slab on every ray and flat box.
The rays are test_sweep.make_rays': zero direction components (NaNs in the
slab test), origins inside the root and on face planes, and a family aimed at
every triangle.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_sweep

ROOT = test_sweep.ROOT
CSRC = test_sweep.CSRC
SRC = os.path.join(ROOT, "tests", "sweep_fold_check.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libsweep_fold_check.so")
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
        L.sweep_fold_check.argtypes = [F32P, sz, U32P, sz, F32P, sz, ctypes.c_int, F32P, sz, U64P, I32P, I32P,
                                       ctypes.c_char_p, sz]
        _LIB = L
    return _LIB


def fold_check(v, idx, nodes, rays):
    """(stats[16], boxes, leaves, slot per leaf in visit order, flat boxes) of tests/sweep_fold_check.cpp."""
    st = np.zeros(16, np.uint64)
    info = np.zeros(3, np.int32)
    slots = np.full(32, -1, np.int32)
    err = ctypes.create_string_buffer(256)
    rays = np.ascontiguousarray(rays, np.float32)
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1)
    rc = lib().sweep_fold_check(v, v.size, idx, idx.size // 3, nodes, nodes.size // 8, 0, rays, rays.shape[0], st, info,
                                slots, err, 256)
    assert rc == 0, (rc, err.value.decode())
    return st, int(info[0]), int(info[1]), slots[:int(info[1])].copy(), int(info[2])


def visit_order(v, idx, nodes):
    """The triangle slot of each leaf of the scene's sweep table, in visit order."""
    return fold_check(v, idx, nodes, np.zeros((1, 8), np.float32) + np.float32(1.0))[3]


SCENES = ["box", "grid:2", "grid:3", "tri:1", "tri:3", "tri:8", "tri:32"]


@pytest.mark.parametrize("name", SCENES)
def test_fold_equals_two_passes_and_threaded_walk(name):
    v, idx, nodes = test_sweep._scene(name)
    rays = test_sweep.make_rays(v, idx, 6000, seed=len(name) * 131 + idx.size)
    st, boxes, leaves, slots, flat = fold_check(v, idx, nodes, rays)
    first = int(st[5])
    where = f"{name}: first bad ray {first}: {rays[first % len(rays)]}"
    assert leaves == idx.size // 3 and sorted(slots) == list(range(leaves))
    if name == "tri:32":
        assert boxes == 63, "the table past 32 boxes (64-bit need words) is in force"
    assert int(st[12]) == 0, f"{name}: {int(st[12])} boxes whose under word is not {{l : need[l] has the box's bit}}"
    assert (int(st[0]), int(st[1])) == (0, 0), f"leaf mask / none differ from sweep_leaves(sweep_mask): {st[:2]}; {where}"
    assert int(st[2]) == 0, f"the sweep past the root differs from the two passes without the early exit: {st[2]}; {where}"
    assert (int(st[3]), int(st[4])) == (0, 0), f"closest hit / shadow differ from the threaded walk: {st[3:5]}; {where}"
    assert int(st[15]) == 0, f"{name}: {int(st[15])} boxes out of the table's order root, general, x-, y-, z-flat"
    assert int(st[13]) == 0, f"{name}: sweep_slab_flat differs from slab on {int(st[13])} (ray, box) pairs"
    # every axis-aligned face is flat: the box's six, the quads of the grids; counted here from the
    # nodes' distinct boxes, the root's apart.  Rays lying in a vertex plane give them a NaN on the
    # flat axis (0 * inf)
    nd = np.ascontiguousarray(nodes, np.float32).reshape(-1, 8)
    distinct = {r[[0, 1, 2, 4, 5, 6]].tobytes(): bool((r[0:3].view(np.uint32) == r[4:7].view(np.uint32)).any())
                for r in nd[1:] if r[[0, 1, 2, 4, 5, 6]].tobytes() != nd[0][[0, 1, 2, 4, 5, 6]].tobytes()}
    assert len(distinct) == boxes - 1 and flat == sum(distinct.values())
    if name == "box":
        assert flat == 6
    if name.startswith(("box", "grid")):
        assert flat >= 4 and st[14] > 0, "flat boxes, and rays whose t on the flat axis is NaN"
    # coverage, so that the pass means something
    assert int(st[6]) == (1 << leaves) - 1, f"{name}: leaf bits never set in a mask: {(1 << leaves) - 1 - int(st[6]):#x}"
    assert st[7] > 0 and st[8] > 0, "rays failing the root box and rays passing it"
    assert st[9] > 0 and st[10] > 0 and st[11] > 0, "the rays reach the geometry"


def test_standalone_program():
    """The harness's own main (the program meant for host sanitizer runs)
    builds and passes on its built-in scene: a cube of flat face boxes plus a
    tilted triangle."""
    srcs, deps = _sources()
    exe = os.path.join(BUILD, "sweep_fold_check")
    if _stale(exe, deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-g", "-DSWEEP_FOLD_MAIN"] + FLAGS + ["-o", exe] + srcs)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "leaves=13 flat_boxes=6 mask=0 none=0 riding=0 hit=0 shadow=0 under=0 flat=0 order=0" in out.stdout, out.stdout
