"""numpy model of h264bsdmiOutputRegionShift (include/h264bsd_mi355x.h): the record of one box of two luma planes.

kept, cur: [H, W] uint8 luma planes of two coded frames of the same size.  The box lies in the kept picture and is the template, T =
box ∩ window; for every displacement |dx|, |dy| <= R the sum over T of |kept(u, v) - cur(clamp(u + dx), clamp(v + dy))|, the current
picture clamped at the WINDOW.  Written naively: a loop over the (2R + 1)^2 displacements with clamped indices.  The answer is the
smallest SAD; ties go to the smallest dx^2 + dy^2, then the smallest dy, then the smallest dx.  A box that misses the window gives
count 0, (0, 0), ties = D^2 and an all-zero surface."""
import numpy as np


def record_bytes(radius, surface):
    D = 2 * radius + 1
    return 32 + (4 * (D * D + 1) if surface else 0)


class Record:
    def __init__(self, count, D, dx, dy, best, still, ties, surface):
        self.count, self.D, self.dx, self.dy, self.best, self.still, self.ties, self.surface = count, D, dx, dy, best, still, ties, surface

    def bytes(self, surface):
        """the record as the call writes it, little endian"""
        head = np.array([self.count, self.D, self.dx & 0xFFFFFFFF, self.dy & 0xFFFFFFFF, self.best, self.still, self.ties, 0], np.uint64)
        words = np.concatenate([head, self.surface.reshape(-1).astype(np.uint64), np.zeros(1, np.uint64)]) if surface else head
        assert (words < 2 ** 32).all()
        return words.astype("<u4").tobytes()


def record(kept, cur, window, box, R):
    """window (x0, y0, w, h) in the coded frame; box (x, y, w, h) relative to the window"""
    assert kept.shape == cur.shape and kept.ndim == 2
    wx, wy, ww, wh = window
    x, y, w, h = box
    x0, x1 = max(x, 0), min(x + w, ww)
    y0, y1 = max(y, 0), min(y + h, wh)
    D = 2 * R + 1
    sad = np.zeros((D, D), np.int64)
    if x1 <= x0 or y1 <= y0:
        return Record(0, D, 0, 0, 0, 0, D * D, sad)
    t = kept[wy + y0:wy + y1, wx + x0:wx + x1].astype(np.int64)
    for dy in range(-R, R + 1):
        rows = wy + np.clip(np.arange(y0, y1) + dy, 0, wh - 1)
        for dx in range(-R, R + 1):
            cols = wx + np.clip(np.arange(x0, x1) + dx, 0, ww - 1)
            sad[dy + R, dx + R] = np.abs(t - cur[rows[:, None], cols[None, :]].astype(np.int64)).sum()
    best = int(sad.min())
    _, dy, dx = min((dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if sad[dy + R, dx + R] == best)
    return Record(t.size, D, dx, dy, best, int(sad[R, R]), int((sad == best).sum()), sad)
