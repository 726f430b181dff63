"""Host side of the spatial variance estimate of short histories, without a
GPU: pt_spatial_variance_host (the header code the kernel compiles,
csrc/pt_denoise.h spatial_var_pixel) against the independent numpy-float32
restatement of tests/spatial_var_ref.py, bit for bit; the argument checks; a
checkerboard whose answer is derived by hand; and the stand-alone program."""
import ctypes
import subprocess

import numpy as np
import pytest

import native
import ptamd
import spatial_var_ref as S
from support import same

PT_OK, PT_ERR_INVALID = 0, -1
F = np.float32
SIZES = [(16, 16), (37, 23), (64, 48)]
RADII = [1, 2, 3]


def test_symbols_and_defaults():
    L = ptamd.lib()
    for name in ("pt_spatial_var_default_params", "pt_spatial_variance_host", "pt_spatial_variance",
                 "pt_temporal_denoise_spatial"):
        assert hasattr(L, name), name
        assert name in ptamd.EXPORTS
    assert L.pt_abi_version() == 3
    p = ptamd.spatial_var_default_params()
    assert (p.below, p.radius, p.sigma_normal, p.sigma_depth) == (2, 1, F(1.0), F(0.5))
    assert (p.below, p.radius, p.sigma_normal, p.sigma_depth) == tuple(
        x if k < 2 else F(x) for k, x in enumerate(S.DEFAULTS))
    assert L.pt_spatial_var_default_params(None) == PT_ERR_INVALID


def _neighbour(mask, dx, dy):
    """mask shifted so that out[y, x] = mask[y + dy, x + dx] (False outside)."""
    H, W = mask.shape
    out = np.zeros_like(mask)
    ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
    yq, xq = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
    out[ys, xs] = mask[yq, xq]
    return out


def holds(d, W, H):
    """Which of the hostile cases the inputs d hold, for a threshold of 2."""
    l, g, miss = d["length"], d["guide"], d["miss"]
    short = l < 2
    four = [(1, 0), (-1, 0), (0, 1), (0, -1)]
    beside = lambda a, b: any(np.any(a & _neighbour(b, dx, dy)) for dx, dy in four)
    up, down = (g[..., 2] > 0) & ~miss, (g[..., 2] < 0) & ~miss
    out = {
        "ones among long": bool(np.any(l == 1) and np.any(l >= 8) and np.any((l == 2) | (l == 3))),
        "one sample has no variance": bool(np.all(d["variance"][l == 1] == 0) and np.any(d["variance"] > 0)),
        "four edges": bool(np.any(short[0]) and np.any(short[-1]) and np.any(short[:, 0]) and np.any(short[:, -1])),
        "short hit beside a miss": beside(short & ~miss, miss),
        "short miss beside a hit": beside(short & miss, ~miss),
        "short miss beside a miss": beside(short & miss, miss),
        "normal flip": beside(short & up, down) and beside(short & down, up),
        "tile without a short pixel": False,
        "tile with a short corner only": False,
    }
    if d["tile_none"] is not None:
        (nx, ny), (cx, cy) = d["tile_none"], d["tile_corner"]
        assert nx % 16 == 0 and ny % 16 == 0 and cx % 16 == 0 and cy % 16 == 0
        out["tile without a short pixel"] = not np.any(short[ny:ny + 16, nx:nx + 16])
        t = short[cy:cy + 16, cx:cx + 16]
        out["tile with a short corner only"] = bool(t[0, 0] and np.count_nonzero(t) == 1 and cx > 0 and cy > 0
                                                    and not miss[cy, cx])
    return out


def test_make_inputs_hold_every_hostile_case():
    for W, H in SIZES:
        h = holds(S.make_inputs(W, H, 100 * W + H), W, H)
        missing = [k for k, v in h.items() if not v]
        if W > 32:          # more than two tile columns: everything, in one frame
            assert not missing, (W, H, missing)
        else:               # a single tile: the two tile cases are frames of their own
            assert missing == ["tile without a short pixel", "tile with a short corner only"], (W, H, missing)
    # the single-tile frames of the two tile cases
    none, corner = S.make_inputs(16, 16, 7, "none"), S.make_inputs(16, 16, 7, "corner")
    assert not np.any(none["length"] < 8)
    assert corner["length"][0, 0] == 1 and np.count_nonzero(corner["length"] < 8) == 1


def _inputs():
    for W, H in SIZES:
        yield W, H, "", S.make_inputs(W, H, 100 * W + H)
    for only in ("none", "corner"):
        yield 16, 16, only, S.make_inputs(16, 16, 7, only)


@pytest.mark.parametrize("radius", RADII)
def test_host_matches_restatement(radius):
    for W, H, tag, d in _inputs():
        for params in (None if radius == 1 else (2, radius, 1.0, 1.0), (4, radius, 0.5, 0.25), (65536, radius, 0.25, 1.0)):
            got = ptamd.spatial_variance_host(d["moments"], d["length"], d["variance"], d["guide"], W, H, params)
            ref = S.spatial_variance(d["moments"], d["length"], d["variance"], d["guide"], W, H,
                                     S.DEFAULTS if params is None else params)
            assert np.all(np.isfinite(got)) and np.all(got >= 0)
            same(got, ref, f"{W}x{H} {tag} {params}")
            below = S.DEFAULTS[0] if params is None else params[0]
            keep = d["length"] >= below
            same(got[keep], d["variance"][keep], "pixels at or above the threshold")
            if tag == "none" and below <= 8:
                same(got, d["variance"], "no short pixel: the variance itself")
            elif not tag:
                assert np.any(got[~keep] > 0)


def test_argument_checks():
    L = ptamd.lib()
    W, H = 16, 16
    d = S.make_inputs(W, H, 1)
    m, l, v, g = (np.ascontiguousarray(d[k], F).reshape(-1) for k in ("moments", "length", "variance", "guide"))
    out = np.full(W * H, -7.0, F)

    def call(params=None, w=W, h=H, **over):
        a = {"m": m.ctypes.data, "l": l.ctypes.data, "v": v.ctypes.data, "g": g.ctypes.data, "out": out.ctypes.data}
        a.update(over)
        p = None if params is None else ctypes.byref(ptamd.SpatialVarParams(*params))
        return L.pt_spatial_variance_host(a["m"], a["l"], a["v"], a["g"], w, h, p, a["out"])

    assert call() == PT_OK
    for k in ("m", "l", "v", "g", "out"):
        assert call(**{k: None}) == PT_ERR_INVALID, k
    for k, a in (("m", m), ("l", l), ("v", v), ("g", g)):
        assert call(out=a.ctypes.data) == PT_ERR_INVALID, k                       # the output is an input
    for w, h in [(0, 16), (16, 0), (-1, 16)]:
        assert call(w=w, h=h) == PT_ERR_INVALID
    inf, nan = float("inf"), float("nan")
    for bad in [(65537, 1, 1.0, 1.0), (2, 0, 1.0, 1.0), (2, 4, 1.0, 1.0), (2, -1, 1.0, 1.0),
                (2, 1, 0.0, 1.0), (2, 1, -1.0, 1.0), (2, 1, inf, 1.0), (2, 1, nan, 1.0), (2, 1, 1e-30, 1.0), (2, 1, 1e30, 1.0),
                (2, 1, 1.0, 0.0), (2, 1, 1.0, -1.0), (2, 1, 1.0, inf), (2, 1, 1.0, nan), (2, 1, 1.0, 1e-30), (2, 1, 1.0, 1e30)]:
        assert call(params=bad) == PT_ERR_INVALID, bad
    for good in [(0, 1, 1.0, 1.0), (65536, 3, 1e-18, 1e18), (2, 2, 1e18, 1e-18)]:
        assert call(params=good) == PT_OK, good
    for below in (0, 1):                                                           # select no pixel
        out[:] = -7.0
        assert call(params=(below, 3, 0.5, 0.5)) == PT_OK
        same(out, v, f"below {below}")
    with pytest.raises(ptamd.PTError):
        ptamd.spatial_variance_host(d["moments"], d["length"][:-1], d["variance"], d["guide"], W, H)


@pytest.mark.parametrize("W,H", [(16, 16), (19, 17)])
def test_checkerboard_has_a_known_answer(W, H):
    """Flat guide (d2n = 0, dz = 0: every tap's exp is 1), one sample
    everywhere (every weight 1 * len = 1), L alternating a = 1 and b = 10 on a
    checkerboard, moments {L, L * L}, radius 1.  An interior pixel's nine taps
    are five of its own L (itself and the diagonals) and four of the other:
      centre a:  s1 = 5 + 40 = 45, M1 = 45 / 9 = 5;  s2 = 5 + 400 = 405, M2 = 45;  M2 - M1 * M1 = 20
      centre b:  s1 = 50 + 4 = 54, M1 = 6;           s2 = 500 + 4 = 504, M2 = 56;  56 - 36 = 20
    (p (1 - p) (a - b)^2 with p = 5/9: 20/81 * 81).  An edge pixel (six taps)
    and a corner (four) have as many of either L: M1 = 5.5, M2 = 50.5, 50.5 -
    30.25 = 20.25.  Every sum and quotient is exact in float32; len_p = 1."""
    a, b = F(1.0), F(10.0)
    ys, xs = np.mgrid[0:H, 0:W]
    Lum = np.where((xs + ys) & 1, b, a).astype(F)
    moments = np.stack([Lum, Lum * Lum], -1)
    length, variance = np.ones((H, W), F), np.zeros((H, W), F)
    guide = np.zeros((H, W, 4), F)
    guide[..., 2], guide[..., 3] = 1.0, 3.0
    got = ptamd.spatial_variance_host(moments, length, variance, guide, W, H, (2, 1, 1.0, 1.0))
    want = np.full((H, W), 20.25, F)
    want[1:-1, 1:-1] = 20.0
    same(got, want, "checkerboard")
    same(ptamd.spatial_variance_host(moments, length, variance, guide, W, H, (1, 1, 1.0, 1.0)), variance, "below 1")


def test_stand_alone_check_program(tmp_path):
    """tests/spatial_var_check.cpp (the program sanitizer runs use), built
    plainly against the library and run."""
    exe = native.against_library("spatial_var_check", tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.startswith("ok:")
