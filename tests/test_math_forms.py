"""The cheaper exact forms of csrc/pt_math.h, on the CPU.

* sincos_ selects and flips sign bits by the quadrant instead of switching; the
  header's sentence "bitwise the same as sin_(x) and cos_(x)" is the test:
  every float in [0, 2*pi] (the shader's domain, 1.09e9 inputs), the specials
  and a million random bit patterns outside that range.
* div1p5_fast_(x) -- x * RN(1/1.5f) with one remainder correction -- is x / 1.5f
  for every x inside div1p5_in_range, over all 2^32 inputs; exactly three
  inputs differ at all (-0, +inf, -inf), and the range excludes them.
* sqrt_in_range, rcp_in_range and div1p5_in_range hold and fail at the bit
  patterns on either side of their stated bounds.

tests/math_forms_check.cpp does the work with pt_math.h's host functions (the
fast forms of sqrt_ and rcp_ need the device's estimate instructions:
pt_selftest_exhaustive fn 4 and 5, tests/test_gpu_math_forms.py).
"""
import os
import re
import subprocess

import pytest

import native


def _fma_flag():
    """fmaf inline instead of through libm, where the CPU has it: the same bits, a third of the time."""
    try:
        with open("/proc/cpuinfo") as f:
            return ["-mfma"] if re.search(r"^flags\s*:.*\bfma\b", f.read(), re.M) else []
    except OSError:
        return []


@pytest.fixture(scope="module")
def report():
    exe = native.build("math_forms_check", [os.path.join(native.TESTS, "math_forms_check.cpp")],
                       ["-O2"] + _fma_flag() + native.COMMON + ["-I", native.CSRC], libs=["-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    fields = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    fields["returncode"] = out.returncode
    return fields


def test_sincos_is_sin_and_cos_bitwise(report):
    assert int(report["sincos_n"]) == 0x40C90FDB + 1, "every float of [0, 2*pi], 2*pi = RN(2 * RN(pi))"
    assert int(report["sincos_bad"]) == 0, report["sincos_first"]
    assert int(report["special_n"]) == 18 and int(report["special_bad"]) == 0
    assert int(report["random_n"]) == 1000000 and int(report["random_bad"]) == 0
    assert report["returncode"] == 0


def test_constant_quotient_is_the_ieee_quotient_in_range(report):
    assert int(report["div_n"]) == 1 << 32
    assert int(report["div_bad"]) == 0, report["div_first"]
    # the range is pinned: -0 and the infinities are all that differ, nothing finite and nonzero
    assert int(report["div_fails"]) == 3 and int(report["div_max_fail_abs"], 16) == 0
    assert int(report["div_lo"], 16) == 0x00000001


def test_range_predicates_at_their_bounds(report):
    # sqrt: 2^-96 in, the float below out, FLT_MAX in; inf, NaN, +0, -0, -2^-96, -1, the least subnormal out; 1 in
    assert report["sqrt_bounds"] == "10100000001"
    # rcp: 2^-126 in, the largest subnormal out, 2^126 in, the float above out, the same four negated;
    # +0, -0, +inf, -inf, NaN out; 1 in
    assert report["rcp_bounds"] == "10101010000001"
    # x / 1.5f: the least subnormal in, +0 out, FLT_MAX in, inf out, the same four negated; +0, -0, NaN out; 1 in
    assert report["div_bounds"] == "101010100001"
