"""The wave-uniform fast forms of csrc/pt_math.h on the GPU.

sqrt_, rcp_ and the SSS step's x / 1.5f run their fast form only when no active
lane of the wave is outside the form's range, and the IEEE form for the whole
wave otherwise.  Two things make that exact:

* the pieces: for every one of the 2^32 bit patterns, NAME_in_range(x) implies
  NAME_fast_(x) is bitwise the IEEE result (pt_selftest_exhaustive fn 4 sqrt,
  5 rcp, 7 x / 1.5f) -- checked on the pieces because consecutive inputs share
  a wave, so the guarded function would answer the 63 inputs next to a range
  boundary from the IEEE side;
* the guard: launches whose waves mix in-range and out-of-range lanes go through
  sqrt_ and rcp_ themselves (pt_selftest_math) and equal the IEEE results.

fn 6: the branch-free sincos_ against sin_ and cos_ over all 2^32 inputs.
"""
import numpy as np
import pytest

import oracle_lib
import ptamd

pytestmark = pytest.mark.gpu

FN_SQRT, FN_RCP = 6, 8   # pt_selftest_math


@pytest.mark.parametrize("fn,name", [(4, "sqrt_fast_ within sqrt_in_range against __builtin_sqrtf"),
                                     (5, "rcp_fast_ within rcp_in_range against 1.0f / x"),
                                     (6, "sincos_ against sin_ and cos_"),
                                     (7, "div1p5_fast_ within div1p5_in_range against x / 1.5f")],
                         ids=["sqrt", "rcp", "sincos", "div1p5"])
def test_fast_forms_exhaustive(fn, name):
    bad, first = ptamd.device_math_exhaustive(fn)
    assert bad == 0, f"{name}: {bad} of 2^32 inputs differ, first 0x{first:08x}"


def test_exhaustive_rejects_an_unknown_fn():
    with pytest.raises(ptamd.PTError):
        ptamd.device_math_exhaustive(8)


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


# 0, -0, subnormals, inf, NaN, 2^-127, 2^127 and the floats at and next to both forms' bounds
SPECIALS = _f([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
               0x7FC00000, 0xFFC00000, 0x00400000, 0x80400000, 0x7F000000, 0xFF000000,
               0x00800000, 0x7E800000, 0x7E800001, 0x0F800000, 0x0F7FFFFF, 0x7F7FFFFF, 0xBF800000])


def _mixed_waves(positive):
    """Waves of 64 consecutive inputs: one special among 63 in-range values, at every 7th lane in turn;
    two, sixteen and sixty-four specials; and waves with none (the fast side)."""
    rnd = np.random.default_rng(29)

    def plain(n):
        x = np.exp(rnd.uniform(-40.0, 40.0, n)).astype(np.float32)
        return x if positive else x * rnd.choice(np.float32([-1.0, 1.0]), n)

    waves = []
    for k, s in enumerate(SPECIALS):
        w = plain(64)
        w[(7 * k) % 64] = s
        waves.append(w)
    for count in (2, 16, 64):
        w = plain(64)
        w[rnd.choice(64, count, replace=False)] = rnd.choice(SPECIALS, count)
        waves.append(w)
    waves += [plain(64) for _ in range(4)]
    return np.concatenate(waves)


@pytest.mark.parametrize("fn,positive", [(FN_SQRT, True), (FN_RCP, False)], ids=["sqrt", "rcp"])
def test_mixed_waves_equal_the_ieee_results(fn, positive):
    x = _mixed_waves(positive)
    assert x.size % 64 == 0
    got = ptamd.device_math(fn, x)
    with np.errstate(all="ignore"):
        want = np.sqrt(x) if fn == FN_SQRT else np.float32(1.0) / x
    nan = np.isnan(want)
    assert nan.any() and np.isinf(want).any() and (want == 0).any(), "the specials reach every IEEE corner"
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    # the oracle's own IEEE forms say the same
    ref = oracle_lib.math(fn, x)
    assert np.array_equal(ref.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
