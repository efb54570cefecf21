"""tests/rounding_model.py held to np.float16 and to the definition of the two uint8 roundings (no GPU): the helper decides which
stored value the GPU tests accept, so it is tested on every finite float16 value and on every uint8 rounding boundary."""
import numpy as np
import pytest

import rounding_model as rd

EPS16, OUT16, IN16 = 2.0 ** -30, 2.0 ** -28, 2.0 ** -31      # below half the finest float16 spacing (2^-25); just outside and inside eps


def _all_f16():
    """every finite float16 value, float64, ascending (one zero), and the value that follows each (65536 after 65504)"""
    h = np.arange(0x10000, dtype=np.uint16).view(np.float16)
    h = np.unique(h[np.isfinite(h)].astype(np.float64))
    assert h.size == 2 * 31743 + 1 and h[-1] == 65504 and h[h > 0][0] == 2.0 ** -24
    return h, np.append(h[1:], rd.F16_TOP)


def test_f16_every_value_is_its_own_rounding_and_decided():
    h, _ = _all_f16()
    want, decided = rd.f16_expected(h, EPS16)
    assert (want.astype(np.float64) == h).all() and decided.all()
    for off in (OUT16, -OUT16):
        want, decided = rd.f16_expected(h + off, EPS16)
        assert (want.astype(np.float64) == h).all() and decided.all()


def test_f16_midpoints_on_below_and_above():
    """between every pair of neighbours, subnormals, zero and the step to infinity included: exactly on the midpoint undecided and
    rounded to the even one; just outside eps decided and rounded to the nearer one; just inside eps undecided"""
    h, nxt = _all_f16()
    top = np.where(nxt == rd.F16_TOP, np.inf, nxt)
    lo = np.append(-np.inf, h)                                      # the same midpoints from below -65504: -65520 rounds to -inf
    for a, b in ((h, top), (lo[:1], h[:1])):
        fa, fb = np.clip(a, -rd.F16_TOP, rd.F16_TOP), np.clip(b, -rd.F16_TOP, rd.F16_TOP)
        mid = (fa + fb) / 2
        with np.errstate(over="ignore"):
            ties = mid.astype(np.float16).astype(np.float64)
        want, decided = rd.f16_expected(mid, EPS16)
        assert not decided.any() and (want.astype(np.float64) == ties).all()
        even = lambda v: (np.where(np.isinf(v), 0x7C00, np.abs(v).astype(np.float16).view(np.uint16)) & 1) == 0      # noqa: E731
        assert (np.where(even(a), a, b) == ties).all()              # np.float16 itself: ties to even (infinity's pattern is even)
        for off, side in ((-OUT16, a), (OUT16, b)):
            want, decided = rd.f16_expected(mid + off, EPS16)
            assert decided.all() and (want.astype(np.float64) == side).all()
        for off in (-IN16, IN16):
            assert not rd.f16_expected(mid + off, EPS16)[1].any()


def test_f16_largest_and_smallest():
    want, decided = rd.f16_expected(np.array([65519.0, 65520.0, 65521.0, 1e9, -65519.0, -65520.0, -1e9, 0.0, 2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -25]), 0.25)
    assert want.astype(np.float64).tolist() == [65504, np.inf, np.inf, np.inf, -65504, -np.inf, -np.inf, 0, 0, 0, 2.0 ** -23]
    assert decided.tolist() == [True, False, True, True, True, False, True] + [False] * 4        # eps 0.25 swallows the subnormal spacing


def test_f16_torch_twin_agrees():
    """test_gpu_tensor_output._f16_rule, the same rule in torch for tensors that stay on the device: same `want`, same `decided`
    with its own eps (one fp32 ulp), on every float16 value, every midpoint and fp32 values next to them"""
    import torch
    from test_gpu_tensor_output import _f16_rule
    h, nxt = _all_f16()
    mid = ((h + nxt) / 2)[:-1]                                      # (65520 rounds to infinity: not a value of these tensors)
    v = np.concatenate([h, mid, np.nextafter(mid.astype(np.float32), np.float32(np.inf)), np.nextafter(mid.astype(np.float32), np.float32(-np.inf)),
                        np.nextafter(np.nextafter(mid.astype(np.float32), np.float32(np.inf)), np.float32(np.inf))]).astype(np.float32)
    eps = np.exp2(np.floor(np.log2(np.maximum(np.abs(v.astype(np.float64)), 2.0 ** -126))) - 23)
    want, decided = rd.f16_expected(v.astype(np.float64), eps)
    got = torch.from_numpy(want.copy())
    within, dec, wrong = _f16_rule(got, torch.from_numpy(v))
    assert within.all() and not wrong.any()
    assert (dec.numpy() == decided).all(), int((dec.numpy() != decided).sum())
    assert decided[:h.size].all() and not decided[h.size:h.size + mid.size].any()
    with np.errstate(over="ignore"):
        off = torch.from_numpy(np.nextafter(want, np.float16(np.inf)))
    assert _f16_rule(off, torch.from_numpy(v))[2].all()


@pytest.mark.parametrize("half_up", [True, False])
def test_u8_boundaries(half_up):
    """k, k + 0.5 and k + 0.5 +- eps (1 +- 1e-3) for k = 0 .. 255"""
    eps = 2e-3
    k = np.arange(256, dtype=np.float64)
    want, decided = rd.u8_expected(k, eps, half_up)
    assert (want == k).all() and decided.all()
    want, decided = rd.u8_expected(k + 0.5, eps, half_up)
    assert not decided.any()
    assert (want == (k + 1 if half_up else k + (k % 2))).all()      # 0.5 -> 1 or 0, 1.5 -> 2, 254.5 -> 255 or 254
    for sign, side in ((-1, k), (1, k + 1)):
        want, decided = rd.u8_expected(k + 0.5 + sign * eps * (1 + 1e-3), eps, half_up)
        assert decided.all() and (want == side).all()
        want, decided = rd.u8_expected(k + 0.5 + sign * eps * (1 - 1e-3), eps, half_up)
        assert not decided.any() and (want == side).all()


def test_decided_is_symmetric_and_empty_from_half_on():
    rng = np.random.default_rng(5)
    k, d = rng.integers(0, 256, 4096).astype(np.float64), rng.uniform(0, 0.5, 4096)
    for eps in (1e-4, 2e-3, 0.1, 0.499):
        up, down = rd.u8_expected(k + 0.5 + d, eps, True)[1], rd.u8_expected(k + 0.5 - d, eps, False)[1]
        assert (up == down).all() and (up == (d > eps)).all()
    x = rng.uniform(0, 255, 4096)
    for eps in (0.5, 0.75):
        assert not rd.u8_expected(x, eps, True)[1].any() and not rd.u8_expected(np.arange(256.0), eps, False)[1].any()
    v = rng.uniform(-3, 3, 4096)
    a, b = rd.f16_expected(v, 1e-5), rd.f16_expected(-v, 1e-5)
    assert (a[1] == b[1]).all() and (a[0] == -b[0]).all()
    assert not rd.f16_expected(v, 1.0)[1].any()                     # half the float16 spacing below 4 is at most 2^-10


def test_the_rule_catches_truncation_and_a_constant_bias():
    """check_u8 / check_f16 on made-up kernels: the right rounding passes; truncation, the other sense on exact ties' neighbours, a
    bias of half a level and round-toward-zero float16 fail"""
    rng = np.random.default_rng(9)
    x = rng.uniform(0, 255, (64, 64, 3))
    assert rd.check_u8(np.floor(x + 0.5), x, 2e-3, True) > 0.99
    assert rd.check_u8(np.rint(x), x, 2e-3, False) > 0.99
    for wrong in (np.floor(x), np.floor(x + 0.9), np.rint(x + 0.4)):
        with pytest.raises(AssertionError):
            rd.check_u8(wrong, x, 2e-3, True)
    v = rng.uniform(-2.2, 2.7, (64, 64, 3))
    nearest = v.astype(np.float16).astype(np.float64)
    assert rd.check_f16(nearest, v, 1e-5, 1e-5) > 0.9
    toward_zero = np.where(np.abs(nearest) > np.abs(v), np.nextafter(v.astype(np.float16), np.float16(0)).astype(np.float64), nearest)
    assert (np.abs(toward_zero - v) <= rd.f16_ulp(v)).all()        # what the comparison accepted before
    with pytest.raises(AssertionError):
        rd.check_f16(toward_zero, v, 1e-5, 1e-5)
