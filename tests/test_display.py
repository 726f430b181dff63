"""Host side of the display transform, without a GPU: the exhaustive check of
the 8-bit sRGB encode (tests/display_check.cpp: the threshold table of
csrc/pt_display.h against the double-precision statement for all 2^32 bit
patterns), pt_display_host against the independent numpy-float32 restatement of
tests/display_ref.py byte for byte on hostile images, answers derived by hand,
the PNG of the bytes against pt_write_image's, and the argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import display_ref as R
import native
import ptamd
from display_ref import same_bytes, same_float

PT_ERR_INVALID = -1
F = np.float32
SIZES = [(16, 16), (37, 23), (64, 48)]
OPERATORS = [R.CLAMP, R.REINHARD, R.ACES]
OP_IDS = ["clamp", "reinhard", "aces"]


# ---- the encode, exhaustively -------------------------------------------------------------------
@pytest.fixture(scope="module")
def report():
    exe = native.build("display_check", [os.path.join(native.TESTS, "display_check.cpp")],
                       ["-O2"] + native.COMMON + ["-I", native.CSRC], libs=["-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    fields = dict(re.findall(r"(\w+)=(\S+)", out.stdout))
    fields["returncode"] = out.returncode
    return fields


def test_encode_is_the_double_statement_for_every_float(report):
    assert int(report["encode_n"]) == 1 << 32
    assert int(report["encode_bad"]) == 0, report["encode_first"]
    assert report["returncode"] == 0


def test_thresholds_increase_and_are_the_least_floats(report):
    assert report["table_increasing"] == "1" and report["table_least"] == "1"
    assert report["seam_codes"] == "10,10"          # both branches at 0.0031308f
    assert report["ends"] == "0,0,0,255,255"        # NaN, -1, -0, +inf, 1


def test_restatement_finds_the_same_thresholds():
    """The restatement's thresholds (bisection over math.pow) are the header's: pt_display_host at the
    default parameters steps from code k - 1 to k exactly there."""
    t = R.thresholds()[1:]
    img = np.zeros((1, 255, 4), F)
    img[0, :, 0] = (t - 1).view(F)
    img[0, :, 1] = t.view(F)
    img[0, :, 2] = (t + 1).view(F)
    got, _ = ptamd.display_host(img, 255, 1)
    k = np.arange(1, 256)
    assert np.array_equal(got[0, :, 0], k - 1) and np.array_equal(got[0, :, 1], k) and np.array_equal(got[0, :, 2], k)
    assert np.all(got[0, :, 3] == 255)


# ---- against the restatement ----------------------------------------------------------------------
EXPECT = {
    "specials": {"nan", "+inf", "-inf", "negative", "-0", "subnormal", "huge", "zero beside lit"},
    "thresholds": {"thresholds"},
    "dark": {"nan", "-inf", "negative", "-0", "nothing metered"},
}


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", list(EXPECT))
def test_hostile_images_hold_their_cases(kind, W, H):
    have = R.holds(R.image(kind, W, H), W, H)
    assert EXPECT[kind] <= have, EXPECT[kind] - have
    if kind == "specials" and (W, H) != (16, 16):
        assert "empty tile" in have
    if kind == "thresholds" and (W, H) != (16, 16):   # 16x16: 255 of its 256 pixels hold the thresholds
        assert "zero beside lit" in have
    if kind != "dark":
        assert "nothing metered" not in have


@pytest.mark.parametrize("auto", [0, 1], ids=["fixed", "metered"])
@pytest.mark.parametrize("tonemap", OPERATORS, ids=OP_IDS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", list(EXPECT))
def test_host_matches_restatement(kind, W, H, tonemap, auto):
    img = R.image(kind, W, H)
    params = (tonemap, 1.5, auto, 0.18, 2.0, 1.0)
    got, used = ptamd.display_host(img, W, H, params)
    ref, ref_used, n = R.display(img, W, H, params)
    same_bytes(got, ref, "against the restatement")
    assert np.all(got[..., 3] == 255)
    if auto:
        same_float(used, ref_used, "the auto scale")
        if kind == "dark":
            assert n == 0 and used == 1.0
    else:
        assert used == 0.0   # untouched without metering


@pytest.mark.parametrize("W,H", SIZES)
def test_three_chained_calls_adapt(W, H):
    params = (R.REINHARD, 1.0, 1, 0.18, 4.0, 0.25)
    prev_host, prev_ref, scales = 0.0, None, []
    for k, kind in enumerate(["specials", "thresholds", "specials"]):
        with np.errstate(over="ignore"):
            img = R.image(kind, W, H, seed=k) * F(4.0 ** k)
        got, prev_host = ptamd.display_host(img, W, H, params, auto_scale=prev_host)
        ref, prev_ref, _ = R.display(img, W, H, params, prev=prev_ref)
        same_bytes(got, ref, f"call {k}")
        same_float(prev_host, prev_ref, f"the auto scale of call {k}")
        scales.append(prev_host)
    assert len(set(scales)) == 3   # the state moved every time
    # a frame with nothing metered keeps the previous scale
    dark = R.image("dark", W, H)
    _, kept = ptamd.display_host(dark, W, H, params, auto_scale=scales[-1])
    assert kept == scales[-1]


# ---- answers derived by hand --------------------------------------------------------------------
def test_reinhard_at_white_gives_luminance_one():
    """L == white: Lp = (L * (1 + L / L^2)) / (1 + L) = (L + 1) / (1 + L) = 1 in real numbers.  In the
    statement's float32 with white = 4 and a grey pixel v = 4 (exposure 1): the products 0.2126f * 4,
    0.7152f * 4 and 0.0722f * 4 are exact (a power of two scales them), and their two rounded sums give
    L = 0x1p+2 = 4 exactly.  Then L / 16 = 0.25, 1 + 0.25 = 1.25, L * 1.25 = 5, 1 + L = 5, all exact:
    Lp = 0x1p+0, q = Lp / L = 0x1p-2, v * q = 0x1p+0 in every channel, the mapped luminance
    lum(1, 1, 1) = 0x1p+0 (bits 0x3f800000), and the code of 1.0 is 255."""
    L = R.lum(F(4), F(4), F(4))
    assert float(L).hex() == "0x1.0000000000000p+2"
    img = np.full((1, 1, 4), 4.0, F)
    v = R.tone(img, 1, 1, R.REINHARD, 1.0, 4.0)
    assert all(F(x).view(np.uint32) == 0x3f800000 for x in v.reshape(-1))
    assert R.lum(*v.reshape(-1)).view(np.uint32) == 0x3f800000   # the mapped luminance: 1 exactly
    got, _ = ptamd.display_host(img, 1, 1, (R.REINHARD, 1.0, 0, 0.18, 4.0, 1.0))
    assert got.reshape(-1).tolist() == [255, 255, 255, 255]
    # half of white stays well below: Lp = (2 * 1.125) / 3 = 0.75
    half, _ = ptamd.display_host(np.full((1, 1, 4), 2.0, F), 1, 1, (R.REINHARD, 1.0, 0, 0.18, 4.0, 1.0))
    assert half[0, 0, 0] == R.srgb8_one(R.tone(np.full((1, 1, 4), 2.0, F), 1, 1, R.REINHARD, 1.0, 4.0)[0, 0, 0])
    assert 220 <= half[0, 0, 0] < 255


@pytest.mark.parametrize("W,H", SIZES)
def test_constant_grey_meters_key_over_its_luminance(W, H):
    """Every term is the same log_(L), every pairwise sum of the tree exact doublings where the counts are
    powers of two; in general the scale is key / exp_(sum / n) with the tree's sum.  For 16x16 the sum
    is 256 * log_(L) exactly, so the scale is key / exp_(log_(L))."""
    import oracle_lib
    grey = F(0.37)
    img = np.full((H, W, 4), grey, F)
    _, used = ptamd.display_host(img, W, H, (R.CLAMP, 1.0, 1, 0.18, 4.0, 1.0))
    L = R.lum(grey, grey, grey)
    logL = oracle_lib.math(0, np.array([L], F))[0]
    if (W, H) == (16, 16):
        want = F(0.18) / oracle_lib.math(1, np.array([logL], F))[0]
        same_float(used, want, "key / exp_(log_(L))")
    total, n = R.meter(img, W, H)
    assert n == W * H
    same_float(used, R.auto_scale(total, n, 0.18, 1.0, None), "the restatement's scale")
    assert abs(used * float(L) / 0.18 - 1.0) < 1e-5   # the mean luminance lands on the key


def test_aces_at_zero_is_zero_and_ends():
    img = np.zeros((1, 4, 4), F)
    img[0, 1, :3] = [np.nan, -1.0, -0.0]
    img[0, 2, :3] = np.inf
    img[0, 3, :3] = 3.4e38
    for tonemap in OPERATORS:
        got, _ = ptamd.display_host(img, 4, 1, (tonemap, 1.0, 0, 0.18, 4.0, 1.0))
        assert got[0, 0].tolist() == [0, 0, 0, 255] and got[0, 1].tolist() == [0, 0, 0, 255], tonemap
        assert got[0, 2].tolist() == [255, 255, 255, 255] and got[0, 3].tolist() == [255, 255, 255, 255], tonemap
    assert float(R.tone(img, 4, 1, R.ACES, 1.0, 4.0)[0, 0, 0]) == 0.0


@pytest.mark.parametrize("tonemap", OPERATORS, ids=OP_IDS)
def test_codes_are_monotone_on_a_grey_ramp(tonemap):
    n = 4096
    ramp = np.concatenate([np.linspace(0, 1, n // 2, dtype=F), np.exp(np.linspace(0, 30, n // 2)).astype(F)])
    assert np.all(np.diff(ramp) >= 0)
    img = np.repeat(ramp[None, :, None], 4, axis=2)
    got, _ = ptamd.display_host(img, n, 1, (tonemap, 1.0, 0, 0.18, 4.0, 1.0))
    for c in range(3):
        assert np.all(np.diff(got[0, :, c].astype(int)) >= 0), c
    assert got[0, 0, 0] == 0 and got[0, -1, 0] == 255


# ---- the default path is pt_write_image's encode -----------------------------------------------
def test_default_params_are_srgb8_and_the_same_png(tmp_path):
    W, H = 37, 23
    rng = np.random.default_rng(5)
    img = (rng.random((H, W, 4), dtype=F) * F(1.3) - F(0.1)).astype(F)
    got, _ = ptamd.display_host(img, W, H)
    assert np.array_equal(got[..., :3], R.srgb8(img[..., :3]))
    a, b = tmp_path / "bytes.png", tmp_path / "floats.png"
    ptamd.write_png8(a, got, W, H)
    ptamd.write_image(b, img, W, H, "png")
    assert a.read_bytes() == b.read_bytes()
    # the alpha a caller hands in is dropped
    got2 = got.copy()
    got2[..., 3] = 7
    ptamd.write_png8(a, got2, W, H)
    assert a.read_bytes() == b.read_bytes()


# ---- arguments, defaults, exports -------------------------------------------------------------
def test_defaults_exports_and_abi():
    p = ptamd.display_default_params()
    assert (p.tonemap, p.exposure, p.auto_exposure, p.key, p.white, p.adapt) == (
        R.DEFAULTS[0], 1.0, 0, float(F(0.18)), 4.0, 1.0)
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in ["pt_display_default_params", "pt_display", "pt_display_device_ptr", "pt_read_display",
                 "pt_display_exposure", "pt_display_reset", "pt_display_readback_begin", "pt_display_readback_end",
                 "pt_display_host", "pt_write_png8"]:
        assert name in ptamd.EXPORTS and hasattr(L, name), name
    img = R.image("specials", 16, 16)
    assert np.array_equal(ptamd.display_host(img, 16, 16)[0], ptamd.display_host(img, 16, 16, R.DEFAULTS)[0])


BAD_PARAMS = [(3, 1, 0, .18, 4, 1), (-1, 1, 0, .18, 4, 1), (0, 0, 0, .18, 4, 1), (0, -1, 0, .18, 4, 1),
              (0, np.inf, 0, .18, 4, 1), (0, np.nan, 0, .18, 4, 1), (0, 1, 2, .18, 4, 1), (0, 1, -1, .18, 4, 1),
              (0, 1, 1, 0, 4, 1), (0, 1, 1, np.nan, 4, 1), (0, 1, 1, np.inf, 4, 1), (1, 1, 0, .18, 0, 1),
              (1, 1, 0, .18, 1e-30, 1), (1, 1, 0, .18, 1e30, 1), (1, 1, 0, .18, np.nan, 1), (0, 1, 1, .18, 4, 0),
              (0, 1, 1, .18, 4, 1.5), (0, 1, 1, .18, 4, np.nan), (0, 1, 1, .18, 4, -0.5)]


def test_host_rejects_bad_arguments(tmp_path):
    L = ptamd.lib()
    img = np.zeros((4, 4, 4), F)
    out = np.zeros((4, 4, 4), np.uint8)
    s = ctypes.c_float(0)
    for bad in BAD_PARAMS:
        p = ptamd.DisplayParams(int(bad[0]), float(bad[1]), int(bad[2]), float(bad[3]), float(bad[4]), float(bad[5]))
        assert L.pt_display_host(img.ctypes.data, 4, 4, ctypes.byref(p), ctypes.byref(s), out.ctypes.data) == PT_ERR_INVALID, bad
    ok = ptamd.DisplayParams(0, 1.0, 1, 0.18, 4.0, 1.0)
    assert L.pt_display_host(None, 4, 4, None, None, out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_display_host(img.ctypes.data, 4, 4, None, None, None) == PT_ERR_INVALID
    assert L.pt_display_host(img.ctypes.data, 0, 4, None, None, out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_display_host(img.ctypes.data, 4, -1, None, None, out.ctypes.data) == PT_ERR_INVALID
    for prev in (-1.0, float("nan"), float("inf")):   # the previous scale: 0 or finite and > 0
        s = ctypes.c_float(prev)
        assert L.pt_display_host(img.ctypes.data, 4, 4, ctypes.byref(ok), ctypes.byref(s), out.ctypes.data) == PT_ERR_INVALID
    assert L.pt_display_host(img.ctypes.data, 4, 4, ctypes.byref(ok), None, out.ctypes.data) == 0   # no state kept
    assert L.pt_display_default_params(None) == PT_ERR_INVALID
    assert L.pt_write_png8(None, out.ctypes.data, 4, 4) == PT_ERR_INVALID
    assert L.pt_write_png8(str(tmp_path / "x.png").encode(), None, 4, 4) == PT_ERR_INVALID
    assert L.pt_write_png8(str(tmp_path / "x.png").encode(), out.ctypes.data, 0, 4) == PT_ERR_INVALID
    assert L.pt_write_png8(str(tmp_path / "no" / "x.png").encode(), out.ctypes.data, 4, 4) == -4   # PT_ERR_IO
