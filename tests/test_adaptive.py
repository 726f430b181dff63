"""Adaptive sampling without a GPU: pt_adaptive_select_host (the header code the
kernel compiles, csrc/pt_denoise.h adaptive_error / adaptive_next) against the
independent numpy-float32 restatement of tests/adaptive_ref.py, bit for bit, on
a crafted 40x24 frame with partial tiles on the right and bottom edges; the
parameter refusals; the plan function's table; the stand-alone program under
the address and undefined-behaviour sanitizers; and the exports."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as A
import native
import ptamd
from support import same

PT_OK, PT_ERR_INVALID = 0, -1
F = np.float32
W, H, P = A.W0, A.H0, A.PARAMS0


def test_symbols_and_defaults():
    L = ptamd.lib()
    for name in ("pt_adaptive_default_params", "pt_adaptive_select_host", "pt_adaptive_select", "pt_adaptive_begin",
                 "pt_adaptive_advance", "pt_adaptive_info", "pt_adaptive_read_counts", "pt_adaptive_read_live",
                 "pt_adaptive_device_ptr", "pt_adaptive_denoise"):
        assert hasattr(L, name), name
        assert name in ptamd.EXPORTS
    assert L.pt_abi_version() == 3
    p = ptamd.adaptive_default_params()
    assert 2 <= p.min_batches <= p.max_batches and p.step >= 1
    assert np.isfinite(p.threshold) and p.threshold > 0 and np.isfinite(p.lum_floor) and p.lum_floor > 0
    assert L.pt_adaptive_default_params(None) == PT_ERR_INVALID


def test_the_crafted_frame_holds_every_case():
    m, where = A.crafted()
    assert A.tiles(W, H) == (3, 2) and W % 16 and H % 16                  # partial tiles on both edges
    n2 = np.full((H, W), 2, np.uint32)
    e = A.pixel_error(m[..., 0], m[..., 1], n2, P[4])
    tile = lambda b: (slice((b // 3) * 16, (b // 3) * 16 + 16), slice((b % 3) * 16, (b % 3) * 16 + 16))
    assert not np.any(m[tile(where["zero"])])
    t1 = m[tile(where["converged"])]
    assert np.any(t1[..., 1] < t1[..., 0] * t1[..., 0]) and np.any(t1[..., 0] < F(P[4]))   # the clamp, the floor
    assert np.all(e[tile(where["converged"])] <= F(P[3])) and np.any(e[tile(where["converged"])] > 0)
    assert np.all(e[tile(where["noisy"])] > F(P[3]))
    assert np.max(e[tile(where["at threshold"])]) == F(P[3])              # exactly at it
    assert np.count_nonzero(np.isnan(m)) == 1 and np.count_nonzero(np.isinf(m)) == 1
    assert np.isnan(m[tile(where["nan"])]).any() and np.isinf(m[tile(where["inf"])]).any()


COUNTS = {
    "all at min": np.full(6, 2, np.uint32),
    "mixed": np.array([2, 5, 8, 5, 2, 8], np.uint32),
    "n + step overshoots max": np.full(6, 8, np.uint32),
    "already at max": np.full(6, 9, np.uint32),
}


@pytest.mark.parametrize("which", list(COUNTS))
@pytest.mark.parametrize("frame", ["crafted", "an ulp above"])
def test_host_matches_restatement(which, frame):
    m, where = A.crafted() if frame == "crafted" else A.just_above_threshold()
    n = COUNTS[which]
    got_n, got_e = ptamd.adaptive_select_host(m, n, W, H, P)
    want_n, want_e = A.select(m, n, W, H, P)
    assert np.array_equal(got_n, want_n), (got_n, want_n)
    same(got_e, want_e, f"{frame}, {which}: E_T")
    # the cases, by their meaning
    lo, hi, step = P[:3]
    grown = np.minimum(n + step, hi) if which != "already at max" else n
    for k in ("nan", "inf", "noisy"):                                      # never converged: stop only at max
        assert got_n[where[k]] == grown[where[k]], k
        assert which == "already at max" or got_n[where[k]] > n[where[k]], k
    assert np.isposinf(got_e[where["nan"]]) and np.isposinf(got_e[where["inf"]])
    assert got_n[where["zero"]] == n[where["zero"]] and got_e[where["zero"]] == 0 and not np.signbit(got_e[where["zero"]])
    assert got_n[where["converged"]] == n[where["converged"]]
    if which == "all at min":
        at = where["at threshold"]
        if frame == "crafted":
            assert got_e[at] == F(P[3]) and got_n[at] == 2                 # e == threshold converges
        else:
            assert got_e[at] > F(P[3]) and got_n[at] == 5
    if which == "already at max":
        assert np.all(got_n == 9)
    assert np.all(got_n <= hi) and np.all(got_n >= n)


def test_a_full_tile_frame_and_a_single_pixel():
    rng = np.random.default_rng(3)
    for w, h in [(32, 16), (1, 1), (17, 33)]:
        m1 = rng.uniform(0, 2, (h, w)).astype(F)
        m = np.stack([m1, m1 * m1 + rng.uniform(0, 0.2, (h, w)).astype(F)], -1)
        bx, by = A.tiles(w, h)
        n = rng.integers(2, 9, bx * by).astype(np.uint32)
        got_n, got_e = ptamd.adaptive_select_host(m, n, w, h, (2, 9, 2, 0.2, 0.01))
        want_n, want_e = A.select(m, n, w, h, (2, 9, 2, 0.2, 0.01))
        assert np.array_equal(got_n, want_n)
        same(got_e, want_e, f"{w}x{h}")


def test_parameter_refusals():
    L = ptamd.lib()
    m, _ = A.crafted()
    m = np.ascontiguousarray(m).reshape(-1)
    n = np.full(6, 2, np.uint32)
    nxt, err = np.zeros(6, np.uint32), np.zeros(6, F)

    def call(params=P, w=W, h=H, **over):
        a = {"m": m.ctypes.data, "n": n.ctypes.data, "nxt": nxt.ctypes.data, "err": err.ctypes.data}
        a.update(over)
        p = None if params is None else ctypes.byref(ptamd.AdaptiveParams(*params))
        return L.pt_adaptive_select_host(a["m"], a["n"], w, h, p, a["nxt"], a["err"])

    assert call() == PT_OK and call(params=None) == PT_OK and call(err=None) == PT_OK
    for k in ("m", "n", "nxt"):
        assert call(**{k: None}) == PT_ERR_INVALID, k
    for w, h in [(0, 24), (40, 0), (-1, 24)]:
        assert call(w=w, h=h) == PT_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    for bad in [(1, 9, 3, 0.25, 0.01), (0, 9, 3, 0.25, 0.01),            # min_batches < 2
                (4, 3, 3, 0.25, 0.01),                                     # max_batches < min_batches
                (2, 9, 0, 0.25, 0.01),                                     # step = 0
                (2, 9, 3, 0.0, 0.01), (2, 9, 3, -1.0, 0.01), (2, 9, 3, inf, 0.01), (2, 9, 3, nan, 0.01),
                (2, 9, 3, 0.25, 0.0), (2, 9, 3, 0.25, -1.0), (2, 9, 3, 0.25, inf), (2, 9, 3, 0.25, nan)]:
        assert call(params=bad) == PT_ERR_INVALID, bad
        assert b"pt_adaptive_params" in L.pt_last_error()
    for good in [(2, 2, 1, 0.25, 0.01), (2, 65536, 2**32 - 1, 1e-30, 1e30)]:
        assert call(params=good) == PT_OK, good
    with pytest.raises(ptamd.PTError):
        ptamd.adaptive_select_host(m, n[:-1], W, H, P)


def test_plan_table():
    """tests/adaptive_plan_check.cpp: plan_adaptive and launch_render_adaptive's selection, row by row."""
    exe = native.build("adaptive_plan_check", [os.path.join(native.TESTS, "adaptive_plan_check.cpp")],
                       ["-O1"] + native.COMMON[:2] + ["-I", native.CSRC])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert lines[-1].startswith("ok: ") and int(lines[-1].split()[1]) == len(lines) - 1 >= 25
    assert sum(1 for ln in lines if "refuse_code=" in ln) >= 10


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/adaptive_check.cpp with -fsanitize=address,undefined: the host
    statement over the crafted frame in exactly sized arrays, run once on the
    CPU as a program of its own (nothing is loaded into this process)."""
    exe = native.build("adaptive_check", [os.path.join(native.TESTS, "adaptive_check.cpp")],
                       ["-O1", "-g"] + native.COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                        "-fno-omit-frame-pointer", "-I", native.CSRC],
                       out_dir=tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.startswith("ok:")
