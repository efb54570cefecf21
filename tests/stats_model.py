"""numpy model of h264bsdmiOutputRegionStats (include/h264bsd_mi355x.h): the record of one box of one picture.

The picture is the I420 coded frame the host path returns (Decoder.next_output_picture): W x H luma bytes, then Cb and Cr of
W/2 x H/2.  channels(): the 8-bit channel planes of a source over the CODED frame — "ycbcr" pairs luma sample (X, Y) with chroma
sample (X >> 1, Y >> 1), "rgb" reads the bytes of pyoracle.oracle_convert (the reference's integer BT.601 conversion, which pairs
them the same way).  record(): count, sum, sumsq, min, max and hist over box ∩ window, all integers."""
import numpy as np

CHANNELS = {"y": 1, "ycbcr": 3, "rgb": 3}
BINS = (0, 16, 32, 64, 128, 256)


def record_bytes(source, bins):
    C = CHANNELS[source]
    return 8 + 24 * C + 4 * C * bins


def channels(i420, W, H, source):
    """[C, H, W] uint8 planes of the coded frame"""
    i420 = np.asarray(i420, dtype=np.uint8).reshape(-1)
    assert i420.size == W * H * 3 // 2
    Y = i420[:W * H].reshape(H, W)
    if source == "y":
        return Y[None]
    if source == "ycbcr":
        cb = i420[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
        cr = i420[W * H * 5 // 4:].reshape(H // 2, W // 2)
        return np.stack([Y, cb.repeat(2, 0).repeat(2, 1), cr.repeat(2, 0).repeat(2, 1)])
    assert source == "rgb"
    from oracle import pyoracle
    px = np.asarray(pyoracle.oracle_convert(0, W, H, i420), dtype=np.uint32).reshape(H, W)      # RGBA: R in the low byte
    return np.stack([(px & 255), (px >> 8) & 255, (px >> 16) & 255]).astype(np.uint8)


class Record:
    def __init__(self, count, sum_, sumsq, min_, max_, hist):
        self.count, self.sum, self.sumsq, self.min, self.max, self.hist = count, sum_, sumsq, min_, max_, hist


def record(planes, window, box, bins):
    """planes: channels(); window (x0, y0, w, h) in the coded frame; box (x, y, w, h) relative to the window"""
    C = planes.shape[0]
    wx, wy, ww, wh = window
    x, y, w, h = box
    x0, x1 = max(x, 0), min(x + w, ww)
    y0, y1 = max(y, 0), min(y + h, wh)
    hist = np.zeros((C, bins), np.int64) if bins else None
    if x1 <= x0 or y1 <= y0:
        return Record(0, np.zeros(C, np.int64), np.zeros(C, np.int64), np.full(C, 255, np.int64), np.zeros(C, np.int64), hist)
    v = planes[:, wy + y0:wy + y1, wx + x0:wx + x1].reshape(C, -1).astype(np.int64)
    if bins:
        shift = 8 - int(np.log2(bins))
        for c in range(C):
            hist[c] = np.bincount(v[c] >> shift, minlength=bins)
    return Record(v.shape[1], v.sum(1), (v * v).sum(1), v.min(1), v.max(1), hist)
