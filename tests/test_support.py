"""tests/support.py: the one bitwise comparison every parity test goes through,
and the PFM reader."""
import numpy as np
import pytest

from support import bits, read_pfm, same, same_nan

F = np.float32


def _nan(payload):
    return np.array([0x7FC00000 | payload], np.uint32).view(F)


def test_same_accepts_equal_bits():
    a = np.array([[0.0, -0.0, 1.5, np.inf], [-np.inf, 1e-45, 3.0, -2.0]], F)
    same(a, a.copy(), "equal")
    same(a[:, ::2], a[:, ::2].copy(), "not contiguous")


def test_same_tells_the_zeros_apart():
    with pytest.raises(AssertionError, match="1 of 2 floats differ"):
        same(np.array([0.0, 1.0], F), np.array([-0.0, 1.0], F), "zeros")


def test_same_compares_nan_payloads():
    same(_nan(5), _nan(5), "the same NaN")
    assert np.isnan(_nan(5)[0]) and np.isnan(_nan(6)[0]) and bits(_nan(5))[0] != bits(_nan(6))[0]
    with pytest.raises(AssertionError, match="differ"):
        same(_nan(5), _nan(6), "two NaNs")


def test_same_nan_takes_any_nan_for_a_nan_and_nothing_else():
    neg = np.array([0xFFC00000], np.uint32).view(F)
    a = np.concatenate([_nan(5), [F(1.5), F(-0.0), F(np.inf)]]).astype(F)
    a[0] = _nan(5)[0]
    b = a.copy()
    b[0] = neg[0]
    same_nan(a, b, "another sign and payload")
    with pytest.raises(AssertionError, match="NaN pattern differs in 1 of 4"):
        same_nan(a, np.array([1.0, 1.5, -0.0, np.inf], F), "a number for a NaN")
    with pytest.raises(AssertionError, match="NaN pattern differs"):
        same_nan(np.array([np.inf], F), _nan(0), "inf is not NaN")
    with pytest.raises(AssertionError, match="1 of 4 floats differ"):
        same_nan(a, np.concatenate([a[:2], [F(0.0), F(np.inf)]]).astype(F), "the zeros apart")
    with pytest.raises(AssertionError):
        same_nan(np.zeros((2, 3), F), np.zeros((3, 2), F), "shape")


def test_same_never_broadcasts():
    a = np.arange(6, dtype=F)
    with pytest.raises(AssertionError, match="shape"):
        same(a.reshape(2, 3), a.reshape(3, 2), "transposed shape")
    row = np.arange(4, dtype=F)
    with pytest.raises(AssertionError, match="8 floats .* against 4"):
        same(np.stack([row, row]), row, "a row against two of it")   # equal wherever numpy would broadcast
    with pytest.raises(AssertionError):
        same(np.zeros((2, 4, 1), F), np.zeros((2, 4), F), "a trailing axis")


def test_same_takes_a_flat_frame_against_a_shaped_one():
    a = np.arange(8, dtype=F).reshape(2, 4)
    same(a, a.reshape(-1).copy(), "flat want")
    same(a.reshape(-1).copy(), a, "flat got")


def test_same_names_the_first_difference():
    got = np.arange(24, dtype=F).reshape(2, 3, 4)
    want = got.copy()
    want[1, 0, 2], want[1, 2, 3] = 99.0, np.nan
    for g, w in ((got, want), (got.reshape(-1), want), (got, want.reshape(-1))):   # unravelled in the shaped operand
        with pytest.raises(AssertionError) as e:
            same(g, w, "frame 7")
        text = str(e.value)
        assert text.startswith("frame 7: 2 of 24 floats differ")
        assert "first at (1, 0, 2): got 14.0" in text and "want 99.0" in text
        assert "max |diff| 85.0" in text                                            # over the finite pairs


def test_read_pfm_round_trip(tmp_path):
    img = (np.arange(18, dtype=F).reshape(2, 3, 3) - F(4.5)) * F(0.25)           # 3 wide, 2 high
    path = tmp_path / "a.pfm"
    with open(path, "wb") as f:
        f.write(b"PF\n3 2\n-1.0\n" + img.astype("<f4").tobytes())
    got = read_pfm(str(path))
    assert got.shape == (2, 3, 3)
    same(got, img, "pfm")
    with open(path, "wb") as f:
        f.write(b"PF\n3 2\n1.0\n" + img.astype(">f4").tobytes())
    with pytest.raises(AssertionError):
        read_pfm(str(path))                                                         # big-endian files are refused
