"""numpy model of h264bsdmiOutputRegionChange (include/h264bsd_mi355x.h): the record of one box of two pictures.

The planes are stats_model.channels() of two I420 coded frames of the same size (the current picture and the kept one): d = current -
kept per channel at every luma position of box ∩ window, in int64.  record(): count, and per channel sad (sum of |d|), ssd (of d * d),
sum (of d, signed), max (of |d|), above (#(|d| > threshold[c])) and hist of |d| (bin = |d| >> (8 - log2 bins)).  A box that misses the
window gives all zeros."""
import numpy as np

from stats_model import BINS, CHANNELS  # noqa: F401


def record_bytes(source, bins):
    C = CHANNELS[source]
    return 8 + 32 * C + 4 * C * bins


class Record:
    def __init__(self, count, sad, ssd, sum_, max_, above, hist):
        self.count, self.sad, self.ssd, self.sum, self.max, self.above, self.hist = count, sad, ssd, sum_, max_, above, hist


def record(cur, kept, window, box, bins, threshold=(0, 0, 0)):
    """cur, kept: [C, H, W] planes; window (x0, y0, w, h) in the coded frame; box (x, y, w, h) relative to the window"""
    assert cur.shape == kept.shape
    C = cur.shape[0]
    wx, wy, ww, wh = window
    x, y, w, h = box
    x0, x1 = max(x, 0), min(x + w, ww)
    y0, y1 = max(y, 0), min(y + h, wh)
    hist = np.zeros((C, bins), np.int64) if bins else None
    zero = np.zeros(C, np.int64)
    if x1 <= x0 or y1 <= y0:
        return Record(0, zero, zero.copy(), zero.copy(), zero.copy(), zero.copy(), hist)
    a = cur[:, wy + y0:wy + y1, wx + x0:wx + x1].reshape(C, -1).astype(np.int64)
    b = kept[:, wy + y0:wy + y1, wx + x0:wx + x1].reshape(C, -1).astype(np.int64)
    d = a - b
    ad = np.abs(d)
    if bins:
        shift = 8 - int(np.log2(bins))
        for c in range(C):
            hist[c] = np.bincount(ad[c] >> shift, minlength=bins)
    thr = np.asarray(list(threshold)[:C], np.int64)[:, None]
    return Record(d.shape[1], ad.sum(1), (d * d).sum(1), d.sum(1), ad.max(1), (ad > thr).sum(1), hist)
