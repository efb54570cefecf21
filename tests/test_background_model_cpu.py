"""CPU: the properties of the background model that h264bsdmiBlendCurrentPictures relies on, checked on the numpy model the GPU tests
compare with (tests/background_model.py), and the Python entry points' own refusals."""
import numpy as np
import pytest

import background_model as bm

W, H = 16, 16
N = W * H * 3 // 2


def _frame(v):
    return np.full(N, v, np.uint8)


def _random(seed):
    return np.random.default_rng(seed).integers(0, 256, N, dtype=np.uint8)


@pytest.mark.parametrize("k", range(8))
def test_every_state_stays_in_range_and_moves_towards_the_target(k):
    """all 65281 x 256 pairs (S, c): 128 <= S' <= 65408, S' between S and T, and no further from T than S"""
    S = np.arange(bm.S_MIN, bm.S_MAX + 1, dtype=np.int64)[:, None]
    T = bm.target(np.arange(256))[None, :]
    S2 = bm.update(S, T, k)
    assert S2.min() >= bm.S_MIN and S2.max() <= bm.S_MAX
    assert (np.minimum(S, T) <= S2).all() and (S2 <= np.maximum(S, T)).all()
    if k == 0:
        assert (S2 == T).all()
    else:
        assert (np.abs(T - S2) <= np.abs(T - S)).all()
        far = np.abs(T - S) > (1 << (k - 1))
        assert (np.abs(T - S2) < np.abs(T - S))[far].all() and (S2 == S)[~far & (np.abs(T - S) < (1 << (k - 1)))].all()


def test_shift_0_is_a_copy_with_the_fraction_of_a_keep():
    a, b = bm.Background(W, H), bm.Background(W, H)
    a.keep(_random(1))
    assert a.blend(_random(2), 0) == (1, 0)
    b.keep(_random(2))
    assert np.array_equal(a.hi, b.hi) and np.array_equal(a.lo, b.lo) and (a.lo == 0x80).all()


def test_the_first_blend_starts_the_model_with_a_copy():
    a = bm.Background(W, H)
    assert a.blend(_random(3), 5, hold=0, moving_shift=bm.FROZEN) == (0, 0)
    assert np.array_equal(a.hi, _random(3)) and (a.lo == 0x80).all()


@pytest.mark.parametrize("k", range(1, 8))
@pytest.mark.parametrize("start,c", [(0, 255), (255, 0), (0, 1), (255, 254), (7, 200)])
def test_constant_input_brings_hi_to_the_input_and_keeps_it_there(k, start, c):
    a = bm.Background(W, H)
    a.keep(_frame(start))
    steps = bm.settle_steps(k, abs(c - start) * 256)
    assert 0 < steps < 1000
    before = a.state()
    for _ in range(steps):
        a.blend(_frame(c), k)
        now = a.state()
        assert (np.abs(bm.target(c) - now) <= np.abs(bm.target(c) - before)).all()
        before = now
    assert (a.hi == c).all(), (k, start, c, steps, a.hi[0], a.lo[0])
    for _ in range(127):                                        # |T - S| <= 127 now, and shrinks by at least 1 until it rests
        a.blend(_frame(c), k)
        assert (a.hi == c).all()
    settled = a.state()
    a.blend(_frame(c), k)
    assert np.array_equal(a.state(), settled) and (np.abs(bm.target(c) - settled) <= (1 << (k - 1))).all()


def test_the_bound_on_the_settling_steps_is_within_a_tenth_of_what_is_needed():
    """the count the model computes is a bound, and a useful one: the state really needs nine tenths of it"""
    for k in range(1, 8):
        S, T, n = np.int64(bm.S_MIN), bm.target(255), 0
        while (S >> 8) != 255:
            S, n = bm.update(S, T, k), n + 1
        assert n <= bm.settle_steps(k, 255 * 256) <= n + 4 + n // 10, (k, n, bm.settle_steps(k, 255 * 256))


@pytest.mark.parametrize("dy", [0, 1])
@pytest.mark.parametrize("dx", [0, 1])
def test_one_moving_luma_sample_moves_the_chroma_sample_over_it(dx, dy):
    """exactly one luma sample differs, at each position of a 2 x 2 block: it and the Cb and Cr sample over the block are moving and
    take moving_shift 0 (a copy); everything else blends at shift 2"""
    kept, cur = _frame(100), _frame(100)
    x, y = 6 + dx, 10 + dy
    cur[y * W + x] = 140
    cur[W * H:] = 104                                           # every chroma sample differs by 4: not moving by itself
    a = bm.Background(W, H)
    a.keep(kept)
    assert a.blend(cur, 2, hold=39, moving_shift=0) == (1, 1)
    want = np.full(N, 100 * 256 + 128, np.int64)
    want[W * H:] += 4 * 256 // 4
    want[y * W + x] = 140 * 256 + 128
    for plane in range(2):
        want[W * H + plane * (W * H // 4) + (y // 2) * (W // 2) + x // 2] = 104 * 256 + 128
    assert np.array_equal(a.state(), want)
    b = bm.Background(W, H)
    b.keep(kept)
    assert b.blend(cur, 2, hold=40, moving_shift=0) == (1, 0)   # the test is strict: 40 is not above 40
    assert b.state()[y * W + x] == 100 * 256 + 128 + 40 * 256 // 4


def test_frozen_leaves_moving_samples_bit_identical():
    a = bm.Background(W, H)
    a.keep(_random(4))
    a.blend(_random(5), 3)                                       # a state with a fraction
    hi, lo = a.hi.copy(), a.lo.copy()
    assert a.blend(_random(6), 3, hold=0, moving_shift=bm.FROZEN)[0] == 1
    _, moving = bm.moving_masks(_random(6), hi, W, H, 0)
    assert moving.any() and not moving.all()
    assert np.array_equal(a.hi[moving], hi[moving]) and np.array_equal(a.lo[moving], lo[moving])
    still = bm.update(hi.astype(np.int64) * 256 + lo, bm.target(_random(6)), 3)
    assert np.array_equal(a.state()[~moving], still[~moving])
    c = bm.Background(W, H)
    c.keep(_frame(10))
    c.blend(_frame(200), 1, hold=0, moving_shift=bm.FROZEN)      # everything is moving
    assert (c.hi == 10).all() and (c.lo == 0x80).all()


def test_hold_255_means_nothing_is_moving():
    a = bm.Background(W, H)
    a.keep(_frame(0))
    assert a.blend(_frame(255), 1, hold=255, moving_shift=bm.FROZEN) == (1, 0)
    assert (a.state() == 128 + (255 * 256 + 1) // 2).all()


def test_the_python_entry_points_exist_and_refuse_what_the_header_refuses(built):
    assert tuple(int(v) for v in built.__version__.split(".")) >= (0, 8, 0)
    assert built.BLEND_FROZEN == bm.FROZEN
    assert {"h264bsdmiBlendCurrentPictures", "h264bsdmiOutputKeptPictures"} <= set(built.EXPORTED_SYMBOLS)
    for kw in (dict(shift=8), dict(shift=-1), dict(hold=256), dict(moving_shift=9), dict(moving_shift="still"), dict(shift=True)):
        with pytest.raises(ValueError):
            built.blend_pictures([], **kw)
