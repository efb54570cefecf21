"""The background model of h264bsdmiBlendCurrentPictures in numpy (test infrastructure), on I420 coded frames as the decoder returns
them: flat uint8 arrays, Y[H, W] then Cb and Cr [H/2, W/2].

The state of a sample is S = 256 hi + lo; `hi` is the kept picture, `lo` the fraction.  With the current sample c, T = 256 c + 128 and
a shift k in 0..7:  S' = S + floor((T - S + 2^(k-1)) / 2^k), and k = 0 gives S' = T.  A luma sample is moving when |c - hi| > hold, a
chroma sample when one of the four luma samples it covers is; still samples take `shift`, moving ones `moving_shift`, or stay as they
are (FROZEN).  The moving test uses the state from before the update."""
import math

import numpy as np

FROZEN = 8                          # H264BSDMI_BLEND_FROZEN
S_MIN, S_MAX = 128, 65408           # T of c = 0 and of c = 255: S never leaves this range


def update(S, T, k):
    """S' of int arrays S, T (or ints) for shifts k (an int, or an array of ints 0..7 of the same shape)"""
    S, T, k = np.asarray(S, np.int64), np.asarray(T, np.int64), np.asarray(k, np.int64)
    return S + ((T - S + ((1 << k) >> 1)) >> k)           # >> of a negative int64 is the arithmetic shift: floor


def target(c):
    return np.asarray(c, np.int64) * 256 + 128


def moving_masks(cur, hi, W, H, hold):
    """(luma [H, W] bool, the whole frame in I420 order bool): which samples are moving"""
    n = W * H
    luma = np.abs(cur[:n].astype(np.int64) - hi[:n].astype(np.int64)).reshape(H, W) > hold
    chroma = luma.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3)).reshape(-1)
    return luma, np.concatenate([luma.reshape(-1), chroma, chroma])


class Background:
    """the kept picture of one instance: hi, lo (uint8, I420 order) or nothing yet.  keep() and blend() are the two calls; blend()
    returns (blended, moving luma samples)"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.hi = self.lo = None

    def keep(self, cur):
        self.hi = np.array(cur, dtype=np.uint8, copy=True)
        self.lo = np.full(cur.shape, 0x80, np.uint8)

    def state(self):
        return self.hi.astype(np.int64) * 256 + self.lo

    def blend(self, cur, shift, hold=255, moving_shift=None):
        assert 0 <= shift <= 7 and 0 <= hold <= 255 and (moving_shift is None or 0 <= moving_shift <= 7 or moving_shift == FROZEN)
        cur = np.asarray(cur, np.uint8)
        assert cur.shape == (self.W * self.H * 3 // 2,)
        if self.hi is None:
            self.keep(cur)                                  # the model starts: S = T, nothing is moving
            return 0, 0
        if moving_shift is None:
            moving_shift = shift
        luma, moving = moving_masks(cur, self.hi, self.W, self.H, hold)
        S = self.state()
        k = np.where(moving, 0 if moving_shift == FROZEN else moving_shift, shift)
        S2 = update(S, target(cur), k)
        if moving_shift == FROZEN:
            S2 = np.where(moving, S, S2)
        assert S2.min() >= S_MIN and S2.max() <= S_MAX
        self.hi, self.lo = (S2 >> 8).astype(np.uint8), (S2 & 255).astype(np.uint8)
        return 1, int(luma.sum())


def settle_steps(k, e0):
    """An upper bound of the updates with shift k (1..7) after which hi equals a constant input c, from a state with |T - S| = e0.
    With e = T - S and r = 2^(k-1), one update gives e' = e - floor((e + r) / 2^k).  floor(x) >= x - (2^k - 1) / 2^k, so for e > 0
    e' <= e (1 - 2^-k) + (r - 1) / 2^k, and for e < 0, floor(x) <= x gives |e'| <= |e| (1 - 2^-k) + r / 2^k: either way
    |e'| - r <= (|e| - r) (1 - 2^-k).  hi == c as soon as |e| <= 127 (S then lies in [256 c + 1, 256 c + 255]), and r <= 64: the
    smallest n with (e0 - r) (1 - 2^-k)^n + r <= 127, and one more for the rounding of this very computation."""
    r = 1 << (k - 1)
    if e0 <= 127:
        return 0
    return int(math.ceil(math.log((127 - r) / (e0 - r)) / math.log(1.0 - 2.0 ** -k))) + 1
