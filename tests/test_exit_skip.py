"""The exit skip's predicate (csrc/pt_isect.h exit_skip, PT_OPT_EXIT_SKIP,
DESIGN.md section 4) on the CPU.

tests/exit_skip_check.cpp compiles the kernels' headers for the host and
checks the three things the skip rests on: (a) the cosine that
sample_hemisphere's sincos_ returns for acos_(sqrt_(1 - r1)) is positive for
every float r1 in [0, 1) -- all 1 065 353 216 of them -- and negative at
r1 == 1.0f, which rng_next can return; (b) over 10^7 generated hits on the six
faces of five root boxes (box.obj's cube, a cuboid, flat_quad's flat root,
floor_and_cloud's root, a cube far from the origin; normals +-1 and +-0.9995
with +0 and -0 tangent components; the hit a few ulp either side of the plane;
r1 == 1.0f mixed in) wherever the predicate holds slab() on the root box with
the full hemisphere direction is false; (c) the predicate is false for a root
face whose normal points inward, a tangent component of one ulp, |hn.a| of
0.998, r1 == 1.0f, and ro.a exactly on the plane.
"""
import os
import re
import subprocess

import pytest

import native

_OUT = None


def output():
    """The program's three lines as {name: {key: value}}, run once."""
    global _OUT
    if _OUT is None:
        exe = native.build("exit_skip_check", [os.path.join(native.TESTS, "exit_skip_check.cpp")],
                           ["-O2"] + native.COMMON + ["-pthread", "-I", native.CSRC])
        run = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        lines = {}
        for line in run.stdout.strip().splitlines():
            name, *kv = line.split()
            lines[name] = dict(item.split("=") for item in kv)
        _OUT = (run.returncode, run.stdout + run.stderr, lines)
    return _OUT


def test_cosine_positive_on_every_draw_below_one():
    rc, text, lines = output()
    a = lines["ct_sweep"]
    print(text)
    assert int(a["inputs"]) == 0x3f800000 == 1065353216, "every float of [0, 1)"
    assert int(a["nonpositive"]) == 0, text
    assert float(a["min_ct"]) > 0.0
    # the bound the theorem quotes (|bd.a| >= 2.4e-4 * 0.999: rcp_ stays normal)
    assert float(a["min_ct"]) >= 2.4e-4
    assert float(a["ct_at_one"]) < 0.0, "r1 == 1.0f is why the predicate asks for r1 < 1"


def test_predicate_implies_root_miss():
    rc, text, lines = output()
    b = lines["fire"]
    print(text)
    assert int(b["fired"]) >= 10 ** 7, text
    assert int(b["wrong"]) == 0, text
    assert int(b["fired"]) < int(b["cases"]), "r1 == 1.0f is mixed in: some cases must not fire"


@pytest.mark.parametrize("kind", ["inward", "tangent_ulp", "n0998", "r1_one", "on_plane"])
def test_predicate_false(kind):
    rc, text, lines = output()
    held, asked = (int(x) for x in lines["nofire"][kind].split("/"))
    print(text)
    assert asked > 10 ** 5, text
    assert held == 0, text


def test_program_status():
    rc, text, _ = output()
    assert rc == 0, text
    assert re.search(r"^fire ", text, re.M) and re.search(r"^nofire ", text, re.M)
