"""Pictures with chosen samples (test infrastructure): a baseline stream whose macroblocks are all I_PCM carries any picture
verbatim, so a test can decide what the pixel-consuming kernels read.

pcm_stream() writes one SPS, one PPS and one IDR I slice per picture on top of h264writer's BitWriter / write_sps / write_pps.  The
slice header bits are followed by mb_type ue(25) and pcm_alignment_zero_bits; from then on every macroblock starts byte-aligned, so
each further one is the two bytes 0D 00 (ue(25) = 0000 11010, then seven alignment bits) and 384 raw bytes: 256 luma, 64 Cb, 64 Cr in
raster order (7.3.5).  The body is assembled with numpy and emulation prevention (7.4.1) is one regular-expression pass: there is no
per-sample Python loop.  Written from the H.264 specification."""
import ctypes
import re

import numpy as np

from h264writer import BitWriter, write_pps, write_sps

_EMULATION = re.compile(rb"\x00\x00(?=[\x00-\x03])")


def _macroblocks(Y, Cb, Cr):
    """[n_mbs, 384] uint8: the samples of every macroblock in raster order of macroblocks"""
    H, W = Y.shape
    hmb, wmb = H // 16, W // 16
    y = Y.reshape(hmb, 16, wmb, 16).transpose(0, 2, 1, 3).reshape(hmb * wmb, 256)
    cb = Cb.reshape(hmb, 8, wmb, 8).transpose(0, 2, 1, 3).reshape(hmb * wmb, 64)
    cr = Cr.reshape(hmb, 8, wmb, 8).transpose(0, 2, 1, 3).reshape(hmb * wmb, 64)
    return np.concatenate([y, cb, cr], axis=1)


def pcm_stream(pictures, crop=None, idc=1, level=51, groups=None, omit=None):
    """An Annex-B stream that decodes to exactly `pictures`, a list of (Y[H, W], Cb[H/2, W/2], Cr[H/2, W/2]) uint8 arrays, H and W
    multiples of 16.  poc_type 2, one reference frame, deblocking_control 1; crop: (left, right, top, bottom) in chroma samples
    (frame_crop_*_offset).  Every picture is an IDR I slice (slice_type 7) with its own idr_pic_id.  idc is
    disable_deblocking_filter_idc: with 0 the offsets are 0 and, I_PCM having QP 0, alpha is 0 and the filter changes no sample, but the
    picture is a filtered one for whoever decodes it.
    groups: an explicit macroblock-to-slice-group map (one group number per macroblock, 0 .. at most 7, every number up to the
    largest in use: slice_group_map_type 6); every picture is then one slice per group, in ascending group order, each holding the
    group's macroblocks in raster order.  omit: {picture index: the groups whose slice NAL unit is left out of that picture} — a
    decoder finds those macroblocks missing when the next picture begins and conceals them."""
    Y0 = np.asarray(pictures[0][0])
    H, W = Y0.shape
    assert H % 16 == 0 and W % 16 == 0 and H and W and idc in (0, 1, 2)
    sps = dict(poc_type=2, num_ref_frames=1, wmb=W // 16, hmb=H // 16, crop=crop, level=level, log2_max_frame_num=4)
    pps = dict(deblocking_control=1)
    n_mbs = (H // 16) * (W // 16)
    if groups is None:
        members = [np.arange(n_mbs)]
    else:
        groups = [int(g) for g in groups]
        assert len(groups) == n_mbs and sorted(set(groups)) == list(range(max(groups) + 1)) and 1 <= max(groups) <= 7
        pps["fmo"] = dict(type=6, groups=max(groups) + 1, ids=groups)
        members = [np.nonzero(np.array(groups) == g)[0] for g in range(max(groups) + 1)]
    omit = omit or {}
    out = [write_sps(sps), write_pps(pps, sps)]
    for k, (Y, Cb, Cr) in enumerate(pictures):
        Y, Cb, Cr = (np.ascontiguousarray(p, dtype=np.uint8) for p in (Y, Cb, Cr))
        assert Y.shape == (H, W) and Cb.shape == Cr.shape == (H // 2, W // 2)
        all_mbs = _macroblocks(Y, Cb, Cr)
        for g, member in enumerate(members):
            if g in omit.get(k, ()):
                continue
            bw = BitWriter()
            bw.ue(int(member[0])); bw.ue(7); bw.ue(0)          # first_mb_in_slice, slice_type, pic_parameter_set_id
            bw.u(4, 0)                                         # frame_num
            bw.ue(k & 0xFFFF)                                  # idr_pic_id
            bw.u(1, 0); bw.u(1, 0)                             # no_output_of_prior_pics, long_term_reference_flag
            bw.se(0)                                           # slice_qp_delta
            bw.ue(idc)
            if idc != 1:
                bw.se(0); bw.se(0)                             # slice_alpha_c0_offset_div2, slice_beta_offset_div2
            bw.ue(25)                                          # mb_type I_PCM of the slice's first macroblock
            bw.align_zero()
            mbs = all_mbs[member]
            body = np.empty((mbs.shape[0], 386), dtype=np.uint8)
            body[:, 0], body[:, 1] = 0x0D, 0x00
            body[:, 2:] = mbs
            rbsp = bw.bytes() + body.reshape(-1)[2:].tobytes() + b"\x80"
            out.append(b"\x00\x00\x00\x01\x65" + _EMULATION.sub(b"\x00\x00\x03", rbsp))
    return b"".join(out)


def i420(picture):
    """concat(Y, Cb, Cr): the coded frame a decoder returns for `picture`"""
    return np.concatenate([np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in picture])


def flat(W, H, y, cb, cr):
    return (np.full((H, W), y, np.uint8), np.full((H // 2, W // 2), cb, np.uint8), np.full((H // 2, W // 2), cr, np.uint8))


def cube_pictures():
    """Two 4096 x 2048 pictures that hold every (Y, Cb, Cr) triple once: chroma sample (cx, cy) of picture p has Cb = cx & 255 and
    Cr = cy & 255, and the four luma samples under it are 4 q + dx + 2 dy with q = (cx >> 8) + 8 (cy >> 8) + 32 p"""
    cx, cy = np.arange(2048)[None, :], np.arange(1024)[:, None]
    Cb = np.broadcast_to(cx & 255, (1024, 2048)).astype(np.uint8)
    Cr = np.broadcast_to(cy & 255, (1024, 2048)).astype(np.uint8)
    x, y = np.arange(4096)[None, :], np.arange(2048)[:, None]
    q = (x >> 9) + 8 * (y >> 9)
    pics = []
    for p in range(2):
        pics.append(((4 * (q + 32 * p) + (x & 1) + 2 * (y & 1)).astype(np.uint8), Cb, Cr))
    return pics


def triples(picture):
    """[H, W] int64: Y << 16 | Cb << 8 | Cr at every luma position (chroma sample (x >> 1, y >> 1))"""
    Y, Cb, Cr = picture
    return (Y.astype(np.int64) << 16) | (Cb.astype(np.int64).repeat(2, 0).repeat(2, 1) << 8) | Cr.astype(np.int64).repeat(2, 0).repeat(2, 1)


def steps(W, H, seed=0):
    """Hard 0 / 255 edges in luma, chroma 128: the picture is cut in four column bands — vertical bars whose widths grow 1, 1, 2, 2,
    3, 3, ... (one-sample lines included), a one-sample checkerboard, horizontal bars of the same widths, and 5 x 3 blocks of 0 or
    255 drawn from `seed`"""
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    edges = np.cumsum(np.repeat(np.arange(1, 64), 2))
    bars = lambda v: (np.searchsorted(edges, v, side="right") & 1).astype(bool)
    rnd = np.random.default_rng(seed).integers(0, 2, (H // 3 + 1, W // 5 + 1)).astype(bool)[y // 3, x // 5]
    band = np.broadcast_to(4 * x // W, (H, W))
    kinds = [np.broadcast_to(bars(x), (H, W)), ((x + y) & 1).astype(bool), np.broadcast_to(bars(y), (H, W)), rnd]
    on = np.choose(band, kinds)
    return (np.where(on, 255, 0).astype(np.uint8), np.full((H // 2, W // 2), 128, np.uint8), np.full((H // 2, W // 2), 128, np.uint8))


def reference_formula(Y, Cb, Cr):
    """(R, G, B) uint8 of the reference's integer BT.601 conversion (limited range) of int arrays of one shape"""
    c, d, e = Y.astype(np.int64) - 16, Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    clip = lambda v: np.clip(v, 0, 255).astype(np.uint8)
    return clip((298 * c + 409 * e + 128) >> 8), clip((298 * c - 100 * d - 208 * e + 128) >> 8), clip((298 * c + 516 * d + 128) >> 8)


def formula_convert(fmt, picture):
    """[H, W] uint32: what h264bsdConvertToRGBA / BGRA / YCbCrA (fmt 0 / 1 / 2) give for `picture`, from reference_formula():
    little-endian bytes R G B 255, B G R 255 or Y Cb Cr 255"""
    Y, Cb, Cr = picture
    cb, cr = Cb.repeat(2, 0).repeat(2, 1), Cr.repeat(2, 0).repeat(2, 1)
    if fmt == 2:
        b0, b1, b2 = Y, cb, cr
    else:
        R, G, B = reference_formula(Y, cb, cr)
        b0, b1, b2 = (R, G, B) if fmt == 0 else (B, G, R)
    return b0.astype(np.uint32) | (b1.astype(np.uint32) << 8) | (b2.astype(np.uint32) << 16) | np.uint32(0xFF000000)


def decode_oracle(data):
    """the coded frames of `data` in output order, through the product's host parser (capture mode) and the CPU pixel oracle"""
    import h264bsd_amd
    from oracle import pyoracle
    state, frames = {"dpb": None}, []

    def on_job(blob):
        if state["dpb"] is None:
            state["dpb"] = pyoracle.OracleDpb(blob)
        state["dpb"].decode(blob)

    dec = h264bsd_amd.Decoder(1, capture=on_job)
    buf = ctypes.create_string_buffer(data, len(data))
    off = stall = 0
    while off < len(data):
        r, rb = dec.decode(ctypes.addressof(buf) + off, len(data) - off)
        stall = stall + 1 if rb == 0 else 0                 # (HDRS_RDY reads nothing: the same bytes are offered again)
        assert r < h264bsd_amd.H264BSD_ERROR and stall <= 3, (r, rb, off)
        off += rb
        if r == h264bsd_amd.H264BSD_PIC_RDY:
            while True:
                o = dec.next_output_info()
                if o is None:
                    break
                frames.append(np.array(state["dpb"].slots[o[0]][:state["dpb"].frame_bytes], copy=True))
    dec.close()
    return frames
