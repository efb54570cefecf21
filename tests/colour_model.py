"""float64 model of h264bsdmiNextOutputTensorBatchColour's arithmetic (include/h264bsd_mi355x.h): the contract that
tests/test_tensor_colour.py and tests/test_gpu_tensor_colour.py hold the kernels to.

Per source pixel: Y', Pb, Pr from the 8-bit samples by range, R, G, B by the matrix's Kr / Kb, each clamped to [0, 1]; CH_Y is Y'
clamped.  Chroma nearest (x >> 1, y >> 1) or bilinear at (x / 2, y / 2 - 1/4), neighbours clamped to the source window's chroma.
Resizing interpolates those values with torch's bilinear source coordinates (align_corners=False, computed in float32 without
contraction, as the kernel does); then floats are (v - mean) / std and U8 rint(255 v), halves to even."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593), "fcc": (0.30, 0.11),
         "smpte240": (0.212, 0.087)}


def ypbpr(Y, Cb, Cr, full):
    Y, Cb, Cr = (np.asarray(a, np.float64) for a in (Y, Cb, Cr))
    if full:
        return Y / 255, (Cb - 128) / 255, (Cr - 128) / 255
    return (Y - 16) / 219, (Cb - 128) / 224, (Cr - 128) / 224


def rgb(Y, Cb, Cr, matrix, full):
    """[..., 3] float64 R, G, B in [0, 1] of 8-bit (possibly upsampled) samples"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    y, pb, pr = ypbpr(Y, Cb, Cr, full)
    r = y + 2 * (1 - kr) * pr
    b = y + 2 * (1 - kb) * pb
    g = y - (2 * kb * (1 - kb) / kg) * pb - (2 * kr * (1 - kr) / kg) * pr
    return np.clip(np.stack([r, g, b], axis=-1), 0, 1)


def luma(Y, full):
    return np.clip(ypbpr(Y, 0, 0, full)[0], 0, 1)


def planes(frame, W, H):
    """Y [H, W], Cb, Cr [H / 2, W / 2] of a host I420 frame"""
    f = np.asarray(frame, np.uint8)
    y = f[: W * H].reshape(H, W)
    cb = f[W * H: W * H + W * H // 4].reshape(H // 2, W // 2)
    cr = f[W * H + W * H // 4: W * H + W * H // 2].reshape(H // 2, W // 2)
    return y, cb, cr


def upsample(c, x0, y0, w, h, chroma):
    """[h, w] float64 chroma of the window's luma samples, from the full chroma plane c"""
    cx0, cy0, cw, ch = x0 // 2, y0 // 2, w // 2, h // 2
    win = c[cy0: cy0 + ch, cx0: cx0 + cw].astype(np.float64)
    xs, ys = np.arange(w), np.arange(h)
    if chroma == "nearest":
        return win[ys[:, None] // 2, xs[None, :] // 2]
    i0 = xs // 2
    i1 = np.minimum(i0 + (xs & 1), cw - 1)
    r0 = ys // 2
    r1 = np.where(ys & 1, np.minimum(r0 + 1, ch - 1), np.maximum(r0 - 1, 0))
    row = lambda r: 0.5 * (win[r[:, None], i0[None, :]] + win[r[:, None], i1[None, :]])     # noqa: E731
    return 0.75 * row(r0) + 0.25 * row(r1)


def colour_hwc(frame, geo, matrix, full, chroma, channels="RGB"):
    """[h, w, C] float64 values in [0, 1] (no alpha) of a host I420 frame's window; geo = (W, H, x0, y0, w, h)"""
    W, H, x0, y0, w, h = geo
    y, cb, cr = planes(frame, W, H)
    Y = y[y0: y0 + h, x0: x0 + w]
    if channels == "Y":
        return luma(Y, full)[:, :, None]
    v = rgb(Y, upsample(cb, x0, y0, w, h, chroma), upsample(cr, x0, y0, w, h, chroma), matrix, full)
    return v[:, :, ::-1] if channels in ("BGR", "BGRA") else v


def _coords(n_out, n_in):
    """torch's bilinear source indices and weights (align_corners=False), in float32 without contraction"""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    f = np.maximum((o + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0))
    i0 = f.astype(np.int64)
    lam = (f - i0.astype(np.float32)).astype(np.float64)
    return i0, np.minimum(i0 + 1, n_in - 1), lam


def resize_hwc(v, size):
    """bilinear resize of [h, w, C] float64 to size = (H, W)"""
    y0, y1, ly = _coords(size[0], v.shape[0])
    x0, x1, lx = _coords(size[1], v.shape[1])
    lx, ly = lx[None, :, None], ly[:, None, None]
    top = (1 - lx) * v[y0][:, x0] + lx * v[y0][:, x1]
    bot = (1 - lx) * v[y1][:, x0] + lx * v[y1][:, x1]
    return (1 - ly) * top + ly * bot


def output(v, dtype, mean=(0, 0, 0), std=(1, 1, 1), channels="RGB"):
    """the values the tensor holds, [h, w, C'] float64 (C' includes alpha): floats (v - mean) / std, u8 rint(255 v)"""
    C = v.shape[2]
    if dtype == "u8":
        out = np.rint(np.round(255 * v, 9))     # exact halves stay halves (float64 noise of 255 * (Y / 255)), rounded to even
    else:
        out = (v - np.asarray(mean[:C], np.float64)) / np.asarray(std[:C], np.float64)
    if channels in ("RGBA", "BGRA"):
        out = np.concatenate([out, np.full(out.shape[:2] + (1,), 255.0 if dtype == "u8" else 1.0)], axis=2)
    return out


def expected(frame, geo, matrix, full, chroma, dtype, layout="NCHW", channels="RGB", mean=(0, 0, 0), std=(1, 1, 1), size=None):
    """the model's tensor slice of one picture, float64, in the layout's shape"""
    v = colour_hwc(frame, geo, matrix, full, chroma, channels)
    if size is not None:
        v = resize_hwc(v, size)
    out = output(v, dtype, mean, std, channels)
    return np.ascontiguousarray(out.transpose(2, 0, 1) if layout == "NCHW" else out)
