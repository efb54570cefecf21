"""float64 model of h264bsdmiOutputTensorRegions (include/h264bsd_mi355x.h): a region is "convert the picture, pad it, crop it,
resample the crop".  The converted window comes from the caller ([wh, ww, C] float64: the oracle's 8-bit values or
tests/colour_model.py's colour), the resampling is tests/resize_model.py's, with the box in the place of the source window."""
import math

import numpy as np

import resize_model as rm


def sample_pad(pad, reference):
    """the value S takes outside the window, per channel: REFERENCE floor(255 pad + 0.5) on the 8-bit scale, otherwise pad itself
    (pad is a float32 in h264bsdmi_resize_spec)"""
    p = np.asarray([float(np.float32(x)) for x in pad], np.float64)
    return np.floor(255 * p + 0.5) if reference else p


def crop_padded(v, box, fill):
    """[h, w, C]: the box (x, y, w, h; x, y relative to the window and of any sign) of the window v [wh, ww, C] extended by fill[c]"""
    x, y, w, h = box
    wh, ww, C = v.shape
    fill = np.asarray(fill, np.float64)[:C]
    s = np.empty((h, w, C))
    s[:] = fill
    xa, xb, ya, yb = max(x, 0), min(x + w, ww), max(y, 0), min(y + h, wh)
    if xa < xb and ya < yb:
        s[ya - y:yb - y, xa - x:xb - x] = v[ya:yb, xa:xb]
    return s


def region(v, box, size, filt, fit="stretch", fill=(0.0, 0.0, 0.0), fma=False):
    """the inner rectangle of one region: ((left, top, iw, ih), [ih, iw, C] float64) for an output of size = (H, W)"""
    s = crop_padded(v, box, fill)
    H, W = size
    left, top, iw, ih = rm.letterbox(W, H, box[2], box[3]) if fit == "letterbox" else (0, 0, W, H)
    return (left, top, iw, ih), rm.resample_hwc(s, (ih, iw), filt, fma)


def whole_outside(box, ww, wh):
    x, y, w, h = box
    return x >= ww or y >= wh or x + w <= 0 or y + h <= 0
