"""The last statement of a tensor-pull kernel, as a rule a test can hold it to (pure numpy, no GPU): which uint8 or float16 value
the model's float64 value must round to, and where that is DECIDED — the value lies further than eps from every point at which the
rounding changes, so a kernel whose pre-rounding value is within eps of the model's cannot legitimately store anything else.

The rule: a decided element equals `want` exactly; an undecided one keeps the bound the comparison had before (uint8 within 1,
float16 within one float16 ulp + tol).  eps is never taken from the kernel under test: it is the tolerance the float32 tests hold the
same kernel's pre-rounding value to, brought to the output's scale.  tests/test_rounding_model.py holds this file to np.float16."""
import numpy as np

U8_FLOOR, F16_FLOOR = 0.95, 0.5     # the least share of decided elements a comparison counts with (check_share)
F16_TOP = 65536.0                   # where float16 would continue: (65504 + 65536) / 2 = 65520 is the midpoint that rounds to infinity


def u8_expected(x, eps, half_up):
    """x: float64 on the 0 .. 255 scale, after the clamp.  (want, decided): floor(x + 0.5) (half_up: the reference colour) or
    np.rint(x) (halves to even: the matrix colours), and whether x lies more than eps from every half-integer"""
    x = np.asarray(x, np.float64)
    want = np.floor(x + 0.5) if half_up else np.rint(x)
    return want, np.abs(x - np.floor(x) - 0.5) > eps


def f16_expected(v, eps):
    """v: finite float64.  (want, decided): v rounded to the nearest float16, ties to even (np.float16; +-inf from 65520 on), and
    whether v lies more than eps from both midpoints between want and its float16 neighbours.  The neighbours are nextafter's, so
    the subnormals (spacing 2^-24 down to 0, midpoints +-2^-25 around 0) need no case of their own; beyond +-65504 the next value
    is taken as +-65536, and an infinite `want` has its one midpoint at +-65520."""
    v = np.asarray(v, np.float64)
    assert np.isfinite(v).all()
    f64 = lambda h: np.clip(h.astype(np.float64), -F16_TOP, F16_TOP)        # noqa: E731  (+-inf -> +-65536)
    with np.errstate(over="ignore"):
        want = v.astype(np.float16)
        up, down = f64(np.nextafter(want, np.float16(np.inf))), f64(np.nextafter(want, np.float16(-np.inf)))
    w = f64(want)
    mid_up = np.where(w >= F16_TOP, np.inf, (w + up) / 2)
    mid_down = np.where(w <= -F16_TOP, -np.inf, (w + down) / 2)
    return want, (np.abs(v - mid_up) > eps) & (np.abs(v - mid_down) > eps)


def f16_ulp(v):
    """the float16 unit in the last place at |v| (2^-24 below 2^-14), float64"""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(a)) - 10)


def check_u8(got, x, eps, half_up, what=""):
    """got: float64 of the uint8 tensor, x: the model before rounding.  Asserts the rule, prints and returns the decided share"""
    want, decided = u8_expected(x, eps, half_up)
    assert got.shape == want.shape, what
    d = np.abs(got - want)
    share = float(decided.mean())
    print(f"{what} u8 eps {eps:.3g}: decided {share:.4f}, undecided that differ {int((d[~decided] != 0).sum())} of {int((~decided).sum())}")
    assert d.max() <= 1, (what, d.max())
    assert (d[decided] == 0).all(), (what, "decided elements differ", int((d[decided] != 0).sum()), x[decided & (d != 0)][:6])
    return share


def check_f16(got, v, eps, tol, what=""):
    """got: float64 of the float16 tensor, v: the model's float64 value.  Asserts the rule (undecided: |got - v| <= ulp + tol),
    prints and returns the decided share"""
    want, decided = f16_expected(v, eps)
    assert got.shape == want.shape, what
    w = want.astype(np.float64)
    wrong = got != w
    d, ulp = np.abs(got - v), f16_ulp(v)
    share = float(decided.mean())
    print(f"{what} f16 eps {eps:.3g}: decided {share:.4f}, undecided that differ {int(wrong[~decided].sum())} of {int((~decided).sum())}")
    assert (d <= ulp + tol).all(), (what, (d / ulp).max())
    assert not wrong[decided].any(), (what, "decided elements differ", int(wrong[decided].sum()), v[decided & wrong][:6])
    return share


def check_share(shares, dt, what=""):
    """the condition on a family x filter x colour: at least one of its comparisons decided U8_FLOOR / F16_FLOOR of its elements"""
    floor = U8_FLOOR if dt == "u8" else F16_FLOOR
    assert shares and max(shares) >= floor, (what, dt, "no comparison decides enough elements", shares)
