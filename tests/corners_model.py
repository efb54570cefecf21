"""numpy model of h264bsdmiOutputCornerPoints (include/h264bsd_mi355x.h): the records of boxes of one luma plane, in exact integers
(int64 throughout: |S| < 2^54; the square root is math.isqrt).  Written for clarity, not speed.  Everything is in the coordinates of
the source window, which is what the regions and the points of a record use: pass the window's samples, L[wy0:wy1, wx0:wx1]."""
import math
import struct

import numpy as np

MIN_EIGEN, HARRIS = "min_eigen", "harris"
PAD = 12                                                 # more than nms + block // 2 + 1 at their largest (7 + 2 + 1)

_isqrt = np.frompyfunc(math.isqrt, 1, 1)


def record_bytes(max_points):
    return 32 + 16 * max_points


def gradients(win):
    """(gx, gy) int64 of the window replicated at its border, at every sample up to PAD - 1 outside it: index [v + PAD - 1, u + PAD - 1]"""
    L = np.pad(np.asarray(win).astype(np.int64), PAD, mode="edge")
    gx = (L[:-2, 2:] + 2 * L[1:-1, 2:] + L[2:, 2:]) - (L[:-2, :-2] + 2 * L[1:-1, :-2] + L[2:, :-2])
    gy = (L[2:, :-2] + 2 * L[2:, 1:-1] + L[2:, 2:]) - (L[:-2, :-2] + 2 * L[:-2, 1:-1] + L[:-2, 2:])
    return gx, gy


def box_sum(P, b):
    """the sums of P over the b x b samples centred on every sample that has them all: b // 2 fewer on every side"""
    h = b // 2
    H, W = P.shape
    out = np.zeros((H - 2 * h, W - 2 * h), np.int64)
    for dy in range(b):
        for dx in range(b):
            out += P[dy:dy + H - 2 * h, dx:dx + W - 2 * h]
    return out


def tensor(win, block):
    """(A, B, C) int64 [H, W] at the window's samples"""
    gx, gy = gradients(win)
    H, W = np.asarray(win).shape
    o = PAD - 1 - block // 2
    return tuple(box_sum(p, block)[o:o + H, o:o + W] for p in (gx * gx, gy * gy, gx * gy))


def scores(win, score, block):
    """S int64 [H, W]"""
    A, B, C = tensor(win, block)
    if score == HARRIS:
        return 16 * (A * B - C * C) - (A + B) * (A + B)
    root = _isqrt(((A - B) * (A - B) + 4 * C * C).astype(object)).astype(np.int64)
    return A + B - root


def candidates(S, nms, min_score):
    """bool [H, W]: S > min_score, and no other window sample within Chebyshev distance nms beats it"""
    H, W = S.shape
    ok = S > min_score
    big = np.pad(S, nms, mode="constant")
    inside = np.pad(np.ones((H, W), bool), nms, mode="constant")
    for dy in range(-nms, nms + 1):
        for dx in range(-nms, nms + 1):
            if dy == 0 and dx == 0:
                continue
            q = big[nms + dy:nms + dy + H, nms + dx:nms + dx + W]
            there = inside[nms + dy:nms + dy + H, nms + dx:nms + dx + W]
            earlier = dy < 0 or (dy == 0 and dx < 0)
            ok &= ~(there & ((q > S) | ((q == S) & earlier)))
    return ok


class Window:
    """one source window, one score and block: the scores are computed once, the candidates once per (nms, min_score)"""

    def __init__(self, win, score=MIN_EIGEN, block=3):
        self.win = np.asarray(win)
        self.S = scores(self.win, score, block)
        gx, gy = gradients(self.win)
        H, W = self.win.shape
        self.g2 = (gx * gx + gy * gy)[PAD - 1:PAD - 1 + H, PAD - 1:PAD - 1 + W]
        self._cand = {}

    def candidates(self, nms, min_score=0):
        if (nms, min_score) not in self._cand:
            self._cand[nms, min_score] = candidates(self.S, nms, min_score)
        return self._cand[nms, min_score]

    def points(self, box, nms, min_score=0):
        """(count, energy, [(x, y, score), ...]) of box = (x, y, w, h): all candidates in T = box ∩ window, in the record's order"""
        H, W = self.win.shape
        x, y, w, h = box
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
        if x1 <= x0 or y1 <= y0:
            return 0, 0, []
        ys, xs = np.nonzero(self.candidates(nms, min_score)[y0:y1, x0:x1])
        pts = sorted(((int(xx) + x0, int(yy) + y0, int(self.S[yy + y0, xx + x0])) for yy, xx in zip(ys, xs)), key=lambda p: (-p[2], p[1], p[0]))
        return (x1 - x0) * (y1 - y0), int(self.g2[y0:y1, x0:x1].sum()), pts

    def record(self, box, nms, max_points, min_score=0):
        """the record's bytes"""
        count, energy, pts = self.points(box, nms, min_score)
        written = min(len(pts), max_points)
        out = struct.pack("<IIIIQQ", count, len(pts), written, 0, energy, 0)
        out += b"".join(struct.pack("<iiq", *p) for p in pts[:written])
        return out + bytes(16 * (max_points - written))
