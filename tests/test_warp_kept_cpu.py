"""CPU: the properties of the resampling that h264bsdmiWarpKeptPictures relies on, checked on the numpy model the GPU tests compare with
(tests/warp_model.py), and warp_coefficients against the exact rational inverse."""
from fractions import Fraction

import numpy as np
import pytest

import background_model as bm
import warp_model as wm

W, H = 48, 32
N = W * H * 3 // 2


def _random(seed, n=N):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _blended(seed, W=W, H=H):
    """a background with a valid, busy fraction"""
    b = wm.Background(W, H)
    for k in range(3):
        b.blend(_random(seed + k, W * H * 3 // 2), 2)
    return b


def _shifted(plane, dx, dy):
    """plane[y + dy, x + dx] with clamped indices"""
    h, w = plane.shape
    return plane[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


def test_the_identity_changes_no_byte():
    b = _blended(1)
    hi, lo = b.hi.copy(), b.lo.copy()
    assert b.warp(wm.IDENTITY) == (1, 0)
    assert np.array_equal(b.hi, hi) and np.array_equal(b.lo, lo)
    k = wm.Background(W, H)
    k.keep(_random(5))
    hi = k.hi.copy()
    assert k.warp(wm.IDENTITY, window=(2, 4, 40, 24)) == (1, 0)
    assert np.array_equal(k.hi, hi) and (k.lo == 0x80).all() and not k.lo_valid


@pytest.mark.parametrize("dx, dy", [(2, 0), (0, -2), (-4, 6), (16, -8)])
def test_an_even_translation_is_an_index_shift_on_all_three_planes(dx, dy):
    b = _blended(2)
    S = b.state()
    warped, count = b.warp(wm.translation(dx, dy))
    assert warped == 1
    for k, (src, got) in enumerate(zip(wm.planes(S, W, H), wm.planes(b.state(), W, H))):
        q = 1 if k == 0 else 2
        assert np.array_equal(got, _shifted(src, dx // q, dy // q))
    assert count == W * H - (W - abs(dx)) * (H - abs(dy))


@pytest.mark.parametrize("dx, dy", [(1, 0), (0, 1), (-3, 5), (7, -1)])
def test_an_odd_translation_shifts_luma_and_puts_chroma_at_half_samples(dx, dy):
    b = _blended(3)
    S = b.state()
    b.warp(wm.translation(dx, dy))
    src, got = wm.planes(S, W, H), wm.planes(b.state(), W, H)
    assert np.array_equal(got[0], _shifted(src[0], dx, dy))
    for k in (1, 2):
        # chroma moves by (dx / 2, dy / 2): the floor, and weight 128 towards the next sample on an odd axis; an outside coordinate
        # was clamped to a whole sample before the weight was taken, which the clamped indices of both neighbours reproduce
        fx, fy = dx >> 1, dy >> 1
        a00, a01 = _shifted(src[k], fx, fy), _shifted(src[k], fx + (dx & 1), fy)
        a10, a11 = _shifted(src[k], fx, fy + (dy & 1)), _shifted(src[k], fx + (dx & 1), fy + (dy & 1))
        wx, wy = 128 * (dx & 1), 128 * (dy & 1)
        V = (a00 * (256 - wx) + a01 * wx) * (256 - wy) + (a10 * (256 - wx) + a11 * wx) * wy
        assert np.array_equal(got[k], (V + 32768) >> 16)


def test_half_a_sample_is_the_rounded_mean_of_two_neighbours():
    b = _blended(4)
    Y = wm.planes(b.state(), W, H)[0]
    for coef, (ax, ay) in ((wm.translation(0.5, 0), (1, 0)), (wm.translation(0, 0.5), (0, 1))):
        X, Yc = wm.luma_coordinates(coef, W, H)
        got, outside = wm.resample(Y, X, Yc, 16)
        assert np.array_equal(got, (Y + _shifted(Y, ax, ay) + 1) >> 1)
        assert outside.sum() == (H if ax else W)            # the last column (row) looks half a sample past the edge


def test_the_half_turn_twice_is_the_identity():
    for b in (_blended(6), _blended(7, 16, 16)):
        S = b.state()
        turn = wm.half_turn(b.W, b.H)
        assert b.warp(turn) == (1, 0)
        once = b.state()
        for src, got in zip(wm.planes(S, b.W, b.H), wm.planes(once, b.W, b.H)):
            assert np.array_equal(got, src[::-1, ::-1])
        assert b.warp(turn) == (1, 0)
        assert np.array_equal(b.state(), S)


@pytest.mark.parametrize("seed", range(4))
def test_the_result_stays_within_its_four_neighbours(seed):
    rng = np.random.default_rng(seed)
    S = rng.integers(bm.S_MIN, bm.S_MAX + 1, (H, W)).astype(np.int64)
    coef = (int(rng.integers(-3 * wm.ONE, 3 * wm.ONE)), int(rng.integers(-wm.ONE, wm.ONE)), int(rng.integers(-20 << 16, 20 << 16)),
            int(rng.integers(-wm.ONE, wm.ONE)), int(rng.integers(-3 * wm.ONE, 3 * wm.ONE)), int(rng.integers(-20 << 16, 20 << 16)))
    for X, Y, bits in (wm.luma_coordinates(coef, W, H) + (16,), wm.chroma_coordinates(coef, W, H) + (18,)):
        got, _, V, near = wm.resample(S, X, Y, bits, parts=True)
        assert (np.minimum.reduce(near) <= got).all() and (got <= np.maximum.reduce(near)).all()
        assert V.min() >= 0 and (V + 32768).max() < 2 ** 32


def test_the_blend_fits_an_unsigned_32_bit_lane_on_a_saturated_state():
    S = np.full((H, W), 65535, np.int64)
    for coef in (wm.IDENTITY, wm.translation(0.5, 0.5), wm.translation(-0.25, 7.75), (70000, 3000, -12345, -2000, 61000, 99999)):
        X, Y = wm.luma_coordinates(coef, W, H)
        got, _, V, _ = wm.resample(S, X, Y, 16, parts=True)
        assert (V == 65535 * 65536).all() and (V + 32768).max() < 2 ** 32 and (got == 65535).all()


@pytest.mark.parametrize("dx, dy", [(W + 3, 0), (-(W + 8), 0), (0, H + 1), (0, -(H + 20))])
def test_a_translation_larger_than_the_picture_is_wholly_outside(dx, dy):
    b = _blended(8)
    S = b.state()
    assert b.warp(wm.translation(dx, dy)) == (1, W * H)
    for src, got in zip(wm.planes(S, W, H), wm.planes(b.state(), W, H)):
        if dx:
            assert np.array_equal(got, np.repeat(src[:, -1 if dx > 0 else 0][:, None], got.shape[1], axis=1))       # constant rows
        else:
            assert np.array_equal(got, np.repeat(src[-1 if dy > 0 else 0][None, :], got.shape[0], axis=0))          # constant columns
    c, fresh = _blended(8), wm.Background(W, H)
    cur = _random(99)
    assert c.warp(wm.translation(dx, dy), wm.CURRENT, current=cur) == (1, W * H)
    fresh.blend(cur, 4)
    assert np.array_equal(c.hi, fresh.hi) and np.array_equal(c.lo, fresh.lo)


def test_outside_the_window_nothing_changes_and_current_needs_a_picture():
    b = _blended(9)
    S = b.state()
    x0, y0, w, h = 2, 4, 40, 24
    assert b.warp(wm.translation(3, -2), window=(x0, y0, w, h))[0] == 1
    for k, (src, got) in enumerate(zip(wm.planes(S, W, H), wm.planes(b.state(), W, H))):
        q = 1 if k == 0 else 2
        inside = np.zeros(src.shape, bool)
        inside[y0 // q:(y0 + h) // q, x0 // q:(x0 + w) // q] = True
        assert np.array_equal(got[~inside], src[~inside]) and not np.array_equal(got[inside], src[inside])
    assert b.warp(wm.IDENTITY, wm.CURRENT) == (0, 0) and wm.Background(W, H).warp(wm.IDENTITY) == (0, 0)


THETAS = [((1.0, 0.0, 5.0), (0.0, 1.0, -3.0)), ((0.97 * np.cos(0.05), -0.97 * np.sin(0.05), 8.25), (0.97 * np.sin(0.05), 0.97 * np.cos(0.05), -5.5)),
          ((0.0, -1.0, 100.0), (1.0, 0.0, 0.0)), ((4.0, 0.0, 0.0), (0.0, 4.0, 0.0)), ((0.25, 0.0, 3.0), (0.0, 0.25, -1.0)),
          ((1.0, 0.3, -2.0), (0.0, 1.0, 7.0)), ((1.0 / 3.0, 0.125, 1000.7), (-0.2, 0.9, -1234.56))]


def test_warp_coefficients_are_the_exact_inverse_within_one_unit(built):
    got = built.warp_coefficients(np.array(THETAS, np.float64))
    assert len(got) == len(THETAS)
    for theta, row in zip(THETAS, got):
        exact = wm.exact_coefficients(theta)                    # of the float64 values themselves: Fraction(float) is exact
        assert row.dtype == np.int32 and row.shape == (6,)
        for v, q in zip(row.tolist(), exact):
            assert abs(Fraction(v) - q) <= 1
    assert got[0].tolist() == [65536, 0, -5 * 65536, 0, 65536, 3 * 65536]
    assert got[2].tolist() == [0, 65536, 0, -65536, 0, 100 * 65536]
    assert got[3].tolist() == [16384, 0, 0, 0, 16384, 0]


def test_warp_coefficients_nan_singular_and_out_of_range_rows(built):
    nan = float("nan")
    rows = [((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((nan, nan, nan), (nan, nan, nan)), ((1.0, 2.0, 0.0), (2.0, 4.0, 1.0)),
            ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((1.0, 0.0, float("inf")), (0.0, 1.0, 0.0))]
    got = built.warp_coefficients(np.array(rows))
    assert got[0].tolist() == list(wm.IDENTITY) and got[1:] == [None] * 4
    assert wm.exact_coefficients(rows[2]) is None
    assert built.warp_coefficients(np.zeros((0, 2, 3))) == []
    for bad in (((1 / 17.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((1.0, 0.0, 40000.0), (0.0, 1.0, 0.0))):       # a zoom above 16; a shift beyond int32
        with pytest.raises(ValueError):
            built.warp_coefficients(np.array([bad]))
    assert built.warp_coefficients(np.array([((1 / 16.0, 0.0, 0.0), (0.0, 1 / 16.0, 0.0))]))[0].tolist() == [wm.MAX_COEFFICIENT, 0, 0, 0, wm.MAX_COEFFICIENT, 0]
    with pytest.raises(ValueError):
        built.warp_coefficients(np.zeros((2, 3)))


def test_the_python_entry_points_exist_and_refuse_what_the_header_refuses(built):
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 13, 0)
    assert "h264bsdmiWarpKeptPictures" in built.EXPORTED_SYMBOLS
    assert built.WARP_MAX_COEFFICIENT == wm.MAX_COEFFICIENT and built.WARP_OUTSIDE == {"replicate": wm.REPLICATE, "current": wm.CURRENT}
    assert [name for name, _ in built.WarpMap._fields_] == list("abcdef") and [name for name, _ in built.WarpSpec._fields_] == ["maps", "outside", "crop", "count"]
    for kw in (dict(), dict(theta=np.zeros((0, 2, 3)), coefficients=[]), dict(coefficients=[], outside="mirror"),
               dict(coefficients=[wm.IDENTITY]), dict(theta=np.zeros((1, 2, 3)))):
        with pytest.raises(ValueError):
            built.warp_kept([], **kw)
