"""float64 model of h264bsdmiOutputTensorRemap (include/h264bsd_mi355x.h): a converted window sampled through a float32 coordinate
map.  The converted window comes from the caller ([h, w, C] float64: the oracle's 8-bit values or tests/colour_model.py's colour).
The clamp, the floor and NEAREST's sum are fp32 operations on the map's fp32 values, exactly as the header specifies them; the
weight is the real difference between the clamped value and its floor, and the blend is in float64."""
import numpy as np

F32 = np.float32


def coordinates(c, n, mode, border):
    """per map value c (float32, finite) along an axis of n samples: (i0, i1, l) — the two neighbour indices (int64, possibly -1 or
    n: outside) and the float64 weight of i1.  NEAREST: i1 = i0 and l = 0."""
    c = np.asarray(c, F32)
    lo, hi = (F32(0), F32(n - 1)) if border == "replicate" else (F32(-1), F32(n))
    cc = np.minimum(np.maximum(c, lo), hi).astype(F32)
    if mode == "nearest":
        i0 = np.floor((cc + F32(0.5)).astype(F32)).astype(np.int64)        # the sum rounded in fp32
        return i0, i0, np.zeros(c.shape, np.float64)
    f = np.floor(cc).astype(F32)
    # the weight as a real number.  The fp32 difference the kernel takes is this exactly wherever cc >= 0; for -1 < cc < 0 (CONSTANT
    # only) cc + 1 may need one bit more than fp32 has, and the kernel's weight is this rounded to nearest: off by at most 2^-25
    l = cc.astype(np.float64) - f.astype(np.float64)
    i0 = f.astype(np.int64)
    return i0, i0 + 1, l


def remap(v, m, mode="bilinear", border="constant", fill=(0.0, 0.0, 0.0), fma=False):
    """v: [h, w, C] float64, the converted window; m: [H, W, 2] float32, x then y; fill: S outside the window per channel
    (region_model.sample_pad).  Returns ([H, W, C] float64, [H, W] bool): the interpolated samples, and the mask of the PADDED
    pixels — those whose coordinates are not finite, which hold the pad under the output's scale instead (their samples are 0 here).
    fma: the REFERENCE blend hy (hx v00 + lx v01) + ly (hx v10 + lx v11) instead of a + l (b - a) along the rows, then between them."""
    assert m.dtype == np.float32 and m.ndim == 3 and m.shape[2] == 2
    h, w, C = v.shape
    fill = np.asarray(fill, np.float64)[:C]
    padded = ~(np.isfinite(m[:, :, 0]) & np.isfinite(m[:, :, 1]))
    mx, my = np.where(padded, F32(0), m[:, :, 0]), np.where(padded, F32(0), m[:, :, 1])
    x0, x1, lx = coordinates(mx, w, mode, border)
    y0, y1, ly = coordinates(my, h, mode, border)

    def S(x, y):
        if border == "replicate":           # only x0 + 1 = w can lie outside, with weight 0: its index is clamped
            return v[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside[:, :, None], v[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], fill[None, None, :])

    v00, v01, v10, v11 = S(x0, y0), S(x1, y0), S(x0, y1), S(x1, y1)
    lx, ly = lx[:, :, None], ly[:, :, None]
    if fma:
        out = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
    else:
        top, bot = v00 + lx * (v01 - v00), v10 + lx * (v11 - v10)
        out = top + ly * (bot - top)
    out[padded] = 0.0
    return out, padded


def near_rounding_boundary(v255, eps=2e-3):
    """U8: which values, on the 0 .. 255 scale before rounding, lie within eps of k + 1/2 — only those may round either way"""
    return np.abs(v255 - np.floor(v255) - 0.5) <= eps


def barrel(H, W, w, h, k=0.35, reach=5.0):
    """a smooth barrel-distortion map [H, W, 2] float32 over a w x h window: the output grid stretched over the window plus `reach`
    samples on every side, pulled towards the centre by (1 + k r^2) / (1 + k r_corner^2), so that
    the corner pixels land `reach` samples outside the window; fractional coordinates throughout"""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, t = 2 * (j + 0.5) / W - 1, 2 * (i + 0.5) / H - 1
    r2 = (u * u + t * t) / 2
    s = (1 + k * r2) / (1 + k * ((1 - 1 / W) ** 2 + (1 - 1 / H) ** 2) / 2)          # 1 at the corner pixels
    x = (w - 1) / 2 + u * s * ((w - 1) / 2 + reach) / (1 - 1 / W)
    y = (h - 1) / 2 + t * s * ((h - 1) / 2 + reach) / (1 - 1 / H)
    return np.stack([x, y], axis=-1).astype(np.float32)
