"""The resampling of h264bsdmiWarpKeptPictures in numpy int64 (test infrastructure), on the background model of
tests/background_model.py: I420 coded frames, flat uint8 arrays hi and lo, Y[H, W] then Cb and Cr [H/2, W/2].

A map is six integers a b c d e f in 16.16 fixed point, from OUTPUT to SOURCE in luma samples of the window (x0, y0, w, h; all even).
For the output luma sample (x, y) of the window:
    X = a x + b y + c,  Y = d x + e y + f            outside = X < 0 or X > (w-1) << 16 or Y < 0 or Y > (h-1) << 16
    X, Y clamped;  x0 = X >> 16, x1 = min(x0 + 1, w - 1), fx = (X >> 8) & 255;  y likewise
    V = (S00 (256 - fx) + S01 fx)(256 - fy) + (S10 (256 - fx) + S11 fx) fy;     S' = (V + 32768) >> 16
with S = 256 hi + lo (lo reads as 128 where it is not valid).  The chroma sample (cx, cy) sits at luma (2 cx + 1/2, 2 cy + 1/2): in
units of 2^-18 chroma sample U = 2 (a 2cx + b 2cy + c) + a + b - 65536, V' likewise with d e f; clamped to (w/2, h/2), index U >> 18,
weight (U >> 10) & 255; outside on its own U, V'.  CURRENT: an output sample whose source was outside takes T = 256 c + 128 of the
current picture's sample at the output position.  Outside the window nothing changes.  hi is always written, lo only where valid."""
import numpy as np

import background_model as bm

REPLICATE, CURRENT = 0, 1           # H264BSDMI_WARP_*
ONE = 65536
MAX_COEFFICIENT = 16 * ONE          # |a|, |b|, |d|, |e|
IDENTITY = (ONE, 0, 0, 0, ONE, 0)


def translation(dx, dy):
    """output (x, y) takes source (x + dx, y + dy), dx, dy in samples (any multiple of 2^-16)"""
    return (ONE, 0, int(round(dx * ONE)), 0, ONE, int(round(dy * ONE)))


def half_turn(w, h):
    return (-ONE, 0, (w - 1) << 16, 0, -ONE, (h - 1) << 16)


def luma_coordinates(coef, w, h):
    """X, Y [h, w] int64 in units of 2^-16 luma sample"""
    a, b, c, d, e, f = (int(v) for v in coef)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return a * x + b * y + c, d * x + e * y + f


def chroma_coordinates(coef, cw, ch):
    """U, V' [ch, cw] int64 in units of 2^-18 chroma sample"""
    a, b, c, d, e, f = (int(v) for v in coef)
    cy, cx = np.mgrid[0:ch, 0:cw].astype(np.int64)
    return 2 * (a * 2 * cx + b * 2 * cy + c) + a + b - ONE, 2 * (d * 2 * cx + e * 2 * cy + f) + d + e - ONE


def axis(X, size, bits):
    """(i0, i1, weight, outside) of coordinates X in units of 2^-bits sample on an axis of `size` samples"""
    top = (size - 1) << bits
    outside = (X < 0) | (X > top)
    X = np.clip(X, 0, top)
    i0 = X >> bits
    return i0, np.minimum(i0 + 1, size - 1), (X >> (bits - 8)) & 255, outside


def resample(S, X, Y, bits, parts=False):
    """the plane S [h, w] (int64 states) read at X, Y: (S' [h, w], outside [h, w] bool); parts: also V and the four neighbours"""
    h, w = S.shape
    x0, x1, fx, ox = axis(X, w, bits)
    y0, y1, fy, oy = axis(Y, h, bits)
    s00, s01, s10, s11 = S[y0, x0], S[y0, x1], S[y1, x0], S[y1, x1]
    V = (s00 * (256 - fx) + s01 * fx) * (256 - fy) + (s10 * (256 - fx) + s11 * fx) * fy
    out = (V + 32768) >> 16
    return (out, ox | oy, V, (s00, s01, s10, s11)) if parts else (out, ox | oy)


def planes(flat, W, H):
    """views Y [H, W], Cb, Cr [H/2, W/2] of a flat I420 array"""
    n = W * H
    return flat[:n].reshape(H, W), flat[n:n + n // 4].reshape(H // 2, W // 2), flat[n + n // 4:].reshape(H // 2, W // 2)


def warp_state(S, W, H, coef, outside=REPLICATE, window=None, current=None):
    """a whole I420 state S (flat int64) through the map: (S' flat int64, luma samples of the window whose source was outside)"""
    x0, y0, w, h = window or (0, 0, W, H)
    assert not (x0 | y0 | w | h) & 1 and w > 0 and h > 0 and x0 + w <= W and y0 + h <= H
    a, b, c, d, e, f = (int(v) for v in coef)
    assert max(abs(a), abs(b), abs(d), abs(e)) <= MAX_COEFFICIENT and all(-2 ** 31 <= v < 2 ** 31 for v in (c, f))
    out = np.array(S, np.int64, copy=True)
    T = bm.target(current) if outside == CURRENT else None
    count = 0
    for k, (src, dst) in enumerate(zip(planes(np.asarray(S, np.int64), W, H), planes(out, W, H))):
        if k == 0:
            win = (slice(y0, y0 + h), slice(x0, x0 + w))
            X, Y = luma_coordinates(coef, w, h)
            res, outs = resample(src[win], X, Y, 16)
            count = int(outs.sum())
        else:
            win = (slice(y0 // 2, (y0 + h) // 2), slice(x0 // 2, (x0 + w) // 2))
            X, Y = chroma_coordinates(coef, w // 2, h // 2)
            res, outs = resample(src[win], X, Y, 18)
        if outside == CURRENT:
            res = np.where(outs, planes(T, W, H)[k][win], res)
        dst[win] = res
    return out, count


class Background(bm.Background):
    """tests/background_model.py's kept picture with the warp: lo_valid is what the library knows of lo (a blend sets it, a plain
    keep clears it: lo then reads as 128 and is not written)"""

    def __init__(self, W, H):
        super().__init__(W, H)
        self.lo_valid = False

    def keep(self, cur):
        super().keep(cur)
        self.lo_valid = False

    def blend(self, cur, shift, hold=255, moving_shift=None):
        res = super().blend(cur, shift, hold, moving_shift)         # (a model that starts goes through keep(): valid from here on)
        self.lo_valid = True
        return res

    def warp(self, coefficients, outside=REPLICATE, window=None, current=None):
        """(warped, luma samples of the window whose source was outside)"""
        if self.hi is None or (outside == CURRENT and current is None):
            return 0, 0
        lo = self.lo if self.lo_valid else np.full(self.lo.shape, 0x80, np.uint8)
        S = self.hi.astype(np.int64) * 256 + lo
        S2, count = warp_state(S, self.W, self.H, coefficients, outside, window, None if current is None else np.asarray(current, np.uint8))
        assert S2.min() >= bm.S_MIN and S2.max() <= bm.S_MAX
        self.hi = (S2 >> 8).astype(np.uint8)
        if self.lo_valid:
            self.lo = (S2 & 255).astype(np.uint8)
        return 1, count


def exact_coefficients(theta):
    """the exact rational inverse of one transform kept -> current ((p, q, tx), (s, t, ty)) of ints, floats or Fractions, times 65536:
    six Fractions a b c d e f, or None when it is singular"""
    from fractions import Fraction
    (p, q, tx), (s, t, ty) = [[Fraction(v) for v in row] for row in theta]
    det = p * t - q * s
    if det == 0:
        return None
    return [v * ONE / det for v in (t, -q, q * ty - t * tx, -s, p, s * tx - p * ty)]
