"""Building and calling the host check programs (tests/*_check.cpp).

One builder for every one of them, a shared library or a program, in
tests/_build or a directory handed in.  An output is rebuilt when it is
missing, older than any file the compiler read for it, or was made by another
command line; what the compiler reads is the compiler's own account (a `-M`
run of the same flags over the same sources, kept beside the output as
<output>.d, with <output>.argv).  `-MD -MF` inside the build command names only
the last source's headers when a command compiles several sources."""
import ctypes
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "discovering-path-tracer_amd", "csrc")
BUILD = os.path.join(TESTS, "_build")
HIPCC = "/opt/rocm/bin/hipcc"
# the checks compare floats bit for bit: no contraction, no fast math
COMMON = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-ffp-contract=off", "-fno-fast-math"]


def _read_files(depfile):
    """The files a make-style dependency file names as prerequisites."""
    with open(depfile) as f:
        words = f.read().replace("\\\n", " ").split()
    return [w for w in words if not w.endswith(":")]


def _stale(out, argv):
    try:
        with open(out + ".argv") as f:
            if json.load(f) != argv:
                return True
        built = os.path.getmtime(out)
        return any(os.path.getmtime(d) > built for d in _read_files(out + ".d"))
    except (OSError, ValueError):   # no output, no record, or a file the last build read is gone
        return True


def build(name, sources, flags, shared=False, libs=(), out_dir=BUILD):
    """Compiles `sources` with `flags` into out_dir/name (a shared library or a program; `libs` go
    behind the sources) unless it is up to date, and returns its path."""
    out = os.path.join(str(out_dir), name)
    argv = [HIPCC] + list(flags) + (["-fPIC", "-shared"] if shared else []) + ["-o", out] + list(sources) + list(libs)
    if _stale(out, argv):
        os.makedirs(str(out_dir), exist_ok=True)
        deps = subprocess.check_output([HIPCC] + list(flags) + ["-M"] + list(sources), text=True)
        subprocess.check_call(argv)
        with open(out + ".d", "w") as f:
            f.write(deps)
        with open(out + ".argv", "w") as f:
            json.dump(argv, f)
    return out


def against_library(name, out_dir):
    """The stand-alone program tests/<name>.cpp built plainly against libptamd in out_dir."""
    from support import PKG as pkg
    return build(name, [os.path.join(TESTS, name + ".cpp")], ["-O2"] + COMMON + ["-I", INCLUDE, "-I", os.path.join(pkg, "csrc")],
                 libs=["-L", pkg, "-lptamd", "-Wl,-rpath," + pkg], out_dir=out_dir)


def sweep_call(fn, v, idx, nodes, rays, n_stats, n_info, extra=(), accept=(0,)):
    """One call of a sweep check's entry point: (vertices, n, indices, triangles, nodes, n, 0, rays, n,
    stats[n_stats], [info[n_info],] *extra, error text, 256).  Returns (stats, info, rc); info is None
    without n_info.  The call must return one of `accept`."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1)
    rays = np.ascontiguousarray(rays, np.float32)
    st = np.zeros(n_stats, np.uint64)
    info = np.zeros(n_info, np.int32) if n_info else None
    err = ctypes.create_string_buffer(256)
    out = (st,) + ((info,) if n_info else ()) + tuple(extra)
    rc = fn(v, v.size, idx, idx.size // 3, nodes, nodes.size // 8, 0, rays, rays.shape[0], *out, err, 256)
    assert rc in accept, (rc, err.value.decode())
    return st, info, rc
