"""Model of the motion export, from capture-mode frame jobs alone.

side_info(jobs): what h264bsdmiSetMotionExport keeps beside every frame buffer, rebuilt in Python by the rules of
include/h264bsd_mi355x.h / engine.hip (motion_keep_item): per picture in decode order the dense per-4x4-block arrays of the frame
buffer it was decoded into.  The vectors come from capi.job_mvs, i.e. from the host parser, which the pixel suites pin to the
reference; what this model adds is everything behind the parser: which job speaks for a slot, validity, ages.

motion_region(side, window, box, size, ...): float64 / integer model of h264bsdmiOutputMotionRegions for one region.
"""

import numpy as np

import h264bsd_amd as hb

FJ_MB_INTER, FJ_MB_CONCEAL_P = 0, 5
PLANES = ("mv", "valid", "age", "qp")


class Side:
    """the side information of one picture: mv int16 [4 hmb, 4 wmb, 2] (quarter samples), valid bool, age and qp uint8 [4 hmb, 4 wmb],
    kind uint8 [hmb, wmb]; pic_seq / slot of the job that wrote it; jobs: how many jobs rendered the picture"""

    def __init__(self, mv, valid, age, qp, kind, pic_seq, slot, jobs):
        self.mv, self.valid, self.age, self.qp, self.kind, self.pic_seq, self.slot, self.jobs = mv, valid, age, qp, kind, pic_seq, slot, jobs


def _blocks(per_mb, hmb, wmb):
    """[n_mbs, 4, 4, ...] (raster 4x4 inside the macroblock) -> [4 hmb, 4 wmb, ...] raster over the picture"""
    rest = per_mb.shape[3:]
    return per_mb.reshape(hmb, wmb, 4, 4, *rest).swapaxes(1, 2).reshape(4 * hmb, 4 * wmb, *rest)


def job_side(job, ages):
    """the arrays of ONE job; ages[k]: the age of a reference to slot k as it stands before this job"""
    h = hb.job_header(job)
    n, wmb, hmb, n_slots = h["n_mbs"], h["width_mbs"], h["height_mbs"], h["n_slots"]
    rec = np.frombuffer(job, dtype=np.uint8, count=n * 32, offset=h["rec_off"]).reshape(n, 32)
    kind, qp = rec[:, 0], rec[:, 1]
    ref = rec[:, 16:20].astype(np.int64)                                      # per 8x8 quadrant, raster
    conceal = kind == FJ_MB_CONCEAL_P
    ref = np.where(conceal[:, None], ref[:, :1], ref)
    quad_valid = ((kind == FJ_MB_INTER) | conceal)[:, None] & (ref < n_slots)
    quad_age = np.where(quad_valid, np.asarray(ages + [0] * 256, dtype=np.int64)[ref], 0)
    q_of_blk = np.array([(b // 8) * 2 + (b % 4) // 2 for b in range(16)])     # blk = 4 by + bx
    valid = quad_valid[:, q_of_blk].reshape(n, 4, 4)
    age = quad_age[:, q_of_blk].reshape(n, 4, 4).astype(np.uint8)
    mv = hb.job_mvs(job).reshape(n, 4, 4, 2).copy()                           # zero for everything that is not FJ_MB_INTER
    mv[~valid] = 0
    qpb = np.repeat(qp[:, None], 16, axis=1).reshape(n, 4, 4)
    return (_blocks(mv, hmb, wmb), _blocks(valid, hmb, wmb), _blocks(age, hmb, wmb), _blocks(qpb, hmb, wmb), kind.reshape(hmb, wmb).copy())


def side_info(jobs, starts=None):
    """one Side per PICTURE in decode order (ghost jobs are pre-passes of the picture that follows in the same slot: they write
    nothing).  The side information of a slot is that of the last non-ghost job decoded into it; the age of a reference = pic_seq of
    the job minus pic_seq of the last non-ghost job that wrote the referenced slot since the sequence began, clamped to [0, 255]; 0
    when that slot has not been written, or is the picture's own.  A new sequence forgets the table: starts = the indices of the
    first job of every sequence (the number of jobs there were when h264bsdDecode returned H264BSD_HDRS_RDY: the decoder
    reconfigures its sink with the next slice); None: wherever the frame size or the number of slots changes."""
    out, table, geo, pending = [], {}, None, 0
    for i, job in enumerate(jobs):
        h = hb.job_header(job)
        g = (h["width_mbs"], h["height_mbs"], h["n_slots"])
        if (i in starts) if starts is not None else (geo is not None and g != geo):
            table = {}
        geo = g
        pending += 1
        if h["ghost"]:
            continue
        cur, seq = h["cur_slot"], h["pic_seq"]
        ages = [min(max(seq - table[k], 0), 255) if k in table and k != cur else 0 for k in range(h["n_slots"])]
        out.append(Side(*job_side(job, ages), seq, cur, pending))
        table[cur] = seq
        pending = 0
    return out


def side_of_slot(jobs, slot, starts=None):
    """the side information beside frame buffer `slot` after `jobs`: that of the last job decoded into it that is no ghost"""
    return [s for s in side_info(jobs, starts) if s.slot == slot][-1]


def letterbox(W, H, w, h):
    """the inner rectangle (left, top, iw, ih) of a w x h box in a W x H output (include/h264bsd_mi355x.h, FIT_LETTERBOX)"""
    s = min(W / w, H / h)
    iw = min(max(int(np.floor(w * s + 0.5)), 1), W)
    ih = min(max(int(np.floor(h * s + 0.5)), 1), H)
    return (W - iw) // 2, (H - ih) // 2, iw, ih


def footprint_blocks(box, rect, window):
    """AREA: the largest number of 4x4 blocks under one output pixel's clipped footprint (T of the error bound)"""
    x, y, w, h = box
    _, _, iw, ih = rect
    return (int(np.ceil(w / iw / 4)) + 1) * (int(np.ceil(h / ih / 4)) + 1)


def _axis_nearest(n_out, off, n_box, n_in, origin, n_win):
    """per output index of the inner rectangle: (inside the window, block index in the frame)"""
    i = np.arange(n_out, dtype=np.int64)
    u = ((2 * i + 1) * n_box) // (2 * n_in)
    p = off + u
    inside = (p >= 0) & (p < n_win)
    return inside, np.where(inside, (origin + p) >> 2, 0)


def _axis_area(n_in, off, n_box, origin, n_win, n_blocks):
    """per output index of the inner rectangle: weights [n_in, n_blocks] = the length a block shares with the clipped footprint"""
    i = np.arange(n_in, dtype=np.float64)
    f0 = off + (i * n_box) / n_in
    f1 = off + ((i + 1) * n_box) / n_in
    c0 = np.maximum(f0, 0.0) + origin
    c1 = np.minimum(f1, float(n_win)) + origin
    b = 4.0 * np.arange(n_blocks, dtype=np.float64)
    wgt = np.minimum(c1[:, None], b[None, :] + 4.0) - np.maximum(c0[:, None], b[None, :])
    return np.where((wgt > 0) & (c1 > c0)[:, None], wgt, 0.0)


def motion_region(side, window, box, size, fit="stretch", sampler="nearest", units="source", per_picture=False, planes=PLANES,
                  f32_steps=False):
    """One region: side a Side; window (x0, y0, W, H) in luma samples of the coded frame; box (x, y, w, h) relative to the window;
    size (height, width) of the output.  Returns (rect, values [height, width, C] float64, scale [height, width, 2] float64: the
    largest |dx| and |dy| of a valid block under each pixel, after per_picture and units, for error bounds).  f32_steps: per_picture's division
    and the unit scaling rounded to float32 where the kernel rounds (NEAREST is then reproduced exactly)."""
    x0, y0, W, H = window
    x, y, w, h = box
    OH, OW = size
    left, top, iw, ih = letterbox(OW, OH, w, h) if fit == "letterbox" else (0, 0, OW, OH)
    mvq = side.mv.astype(np.float64) / 4.0
    age = side.age.astype(np.float64)
    if per_picture:
        div = np.maximum(age, 1.0)[..., None]
        mvq = (mvq.astype(np.float32) / div.astype(np.float32)).astype(np.float64) if f32_steps else mvq / div
    if units == "output":
        sc = (np.float32(iw) / np.float32(w), np.float32(ih) / np.float32(h)) if f32_steps else (iw / w, ih / h)
    else:
        sc = (1.0, 1.0)
    valid = side.valid.astype(np.float64)
    qp = side.qp.astype(np.float64)
    inner = np.zeros((ih, iw, 5))
    mag = np.zeros((ih, iw, 2))
    if sampler == "nearest":
        in_x, kx = _axis_nearest(iw, x, w, iw, x0, W)
        in_y, ky = _axis_nearest(ih, y, h, ih, y0, H)
        m = in_y[:, None] & in_x[None, :]
        g = np.ix_(ky, kx)
        inner[..., 0:2] = mvq[g] * m[..., None]
        inner[..., 2] = valid[g] * m
        inner[..., 3] = age[g] * m
        inner[..., 4] = qp[g] * m
        mag = np.abs(mvq[g]) * m[..., None]
    else:
        hb4, wb4 = valid.shape
        wx = _axis_area(iw, x, w, x0, W, wb4)                  # [iw, wb4]
        wy = _axis_area(ih, y, h, y0, H, hb4)                  # [ih, hb4]
        s_all = wy.sum(1)[:, None] * wx.sum(1)[None, :]
        s_valid = wy @ valid @ wx.T
        with np.errstate(invalid="ignore", divide="ignore"):
            for c in range(2):
                inner[..., c] = np.where(s_valid > 0, (wy @ (mvq[..., c] * valid) @ wx.T) / s_valid, 0.0)
            inner[..., 3] = np.where(s_valid > 0, (wy @ (age * valid) @ wx.T) / s_valid, 0.0)
            inner[..., 4] = np.where(s_all > 0, (wy @ qp @ wx.T) / s_all, 0.0)
        inner[..., 2] = s_valid / ((w / iw) * (h / ih))
        a = np.abs(mvq) * valid[..., None]
        for r in range(ih):                                     # the largest magnitude under each footprint
            rows = np.nonzero(wy[r] > 0)[0]
            if not len(rows):
                continue
            col_max = a[rows.min():rows.max() + 1].max(axis=0)
            for c in range(iw):
                cols = np.nonzero(wx[c] > 0)[0]
                if len(cols):
                    mag[r, c] = col_max[cols.min():cols.max() + 1].max()
    if f32_steps:
        inner[..., 0] = (inner[..., 0].astype(np.float32) * np.float32(sc[0])).astype(np.float64)
        inner[..., 1] = (inner[..., 1].astype(np.float32) * np.float32(sc[1])).astype(np.float64)
    else:
        inner[..., 0] *= float(sc[0])
        inner[..., 1] *= float(sc[1])
    chans = [c for name, cs in (("mv", (0, 1)), ("valid", (2,)), ("age", (3,)), ("qp", (4,))) if name in planes for c in cs]
    out = np.zeros((OH, OW, len(chans)))
    out[top:top + ih, left:left + iw] = inner[..., chans]
    scale = np.zeros((OH, OW, 2))
    scale[top:top + ih, left:left + iw] = mag * np.array([abs(float(sc[0])), abs(float(sc[1]))])
    return (left, top, iw, ih), out, scale


def whole_window(info_or_side, crop, cropping=None):
    """(x0, y0, W, H): the SPS cropping window (cropping = Decoder.cropping_params()) when crop, else the coded frame"""
    hb4, wb4 = info_or_side.valid.shape
    if crop and cropping and cropping[0]:
        _, left, cw, top, ch = cropping
        return left, top, cw, ch
    return 0, 0, 4 * wb4, 4 * hb4


def native_size(window):
    return (window[3] + 3) // 4, (window[2] + 3) // 4
