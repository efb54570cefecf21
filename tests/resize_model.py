"""float64 model of h264bsdmiNextOutputTensorBatchResize's geometry (include/h264bsd_mi355x.h): torch's antialiased weights, the
letterbox rectangle, and the resampling of a [h, w, C] picture with them.  tests/test_tensor_resize.py holds it to
torch.nn.functional.interpolate(..., antialias=True); tests/test_gpu_tensor_resize.py holds the kernel to it."""
import math

import numpy as np

INTERP = {"bilinear": 2, "bicubic": 4}


def triangle(x):
    x = np.abs(x)
    return np.where(x < 1, 1 - x, 0.0)


def keys_cubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1,
                    np.where(x < 2, ((a * x - 5 * a) * x + 8 * a) * x - 4 * a, 0.0))


def aa_weights(n_in, n_out, mode):
    """[n_out, n_in] float64 matrix of torch's antialiased weights (each row sums to 1)"""
    scale = n_in / n_out
    support = INTERP[mode] / 2 * max(scale, 1.0)
    filt = triangle if mode == "bilinear" else keys_cubic
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        center = scale * (i + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        j = np.arange(xmin, xmax)
        w = filt((j - center + 0.5) / max(scale, 1.0))
        m[i, xmin:xmax] = w / w.sum()
    return m


def tap_counts(n_in, n_out, mode):
    """the number of taps of each output index"""
    return (aa_weights(n_in, n_out, mode) != 0).sum(axis=1)


def bilinear_weights(n_in, n_out, fma=False):
    """[n_out, n_in] of torch's bilinear without antialiasing (align_corners=False), coordinates in float32 as the kernels compute them:
    rounded after every operation, or (fma, the reference colour's path) (o + 0.5) * scale - 0.5 rounded once"""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    if fma:         # the product of two float32 values is exact in float64
        f = np.maximum(((o + np.float32(0.5)).astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32), np.float32(0))
    else:
        f = np.maximum((o + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0))
    i0 = f.astype(np.int64)
    lam = (f - i0.astype(np.float32)).astype(np.float64)
    m = np.zeros((n_out, n_in))
    m[np.arange(n_out), i0] += 1 - lam
    m[np.arange(n_out), np.minimum(i0 + 1, n_in - 1)] += lam
    return m


def weights(n_in, n_out, filt, fma=False):
    """filt: "bilinear" (no antialiasing), "bilinear_aa" or "bicubic_aa" (the H264BSDMI_FILTER_* names)"""
    if filt == "bilinear":
        return bilinear_weights(n_in, n_out, fma)
    return aa_weights(n_in, n_out, filt[:-3])


def resample_hwc(v, size, filt, fma=False):
    """[h, w, C] float64 resampled to size = (H, W)"""
    wy = weights(v.shape[0], size[0], filt, fma)
    wx = weights(v.shape[1], size[1], filt, fma)
    t = np.tensordot(wy, v, axes=(1, 0))                        # [H, w, C]
    return np.ascontiguousarray(np.tensordot(wx, t, axes=(1, 1)).transpose(1, 0, 2))


def letterbox(W, H, w, h):
    """(left, top, iw, ih) of a w x h window in a W x H output"""
    s = min(W / w, H / h)
    iw = min(max(math.floor(w * s + 0.5), 1), W)
    ih = min(max(math.floor(h * s + 0.5), 1), H)
    return (W - iw) // 2, (H - ih) // 2, iw, ih


def pad_value(pad, dtype, mean=0.0, std=1.0):
    """the border value of one output channel as the tensor holds it (float32 for floats, before the dtype's rounding); pad, mean and
    std are float32 in h264bsdmi_resize_spec / h264bsdmi_tensor_spec"""
    pad, mean, std = (float(np.float32(x)) for x in (pad, mean, std))
    if dtype == "u8":
        return float(math.floor(255 * pad + 0.5))
    return float(np.float32((pad - mean) / std))
