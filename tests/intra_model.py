"""Intra reconstruction as a plain integer model (test infrastructure): Python ints and lists, no numpy arithmetic, no C.

A third statement of the arithmetic, next to k_frame_intra (h264bsd_amd/csrc/kernels/k_frame_intra.hip.h) and recon_intra* /
mb_residual (oracle/pixel_oracle.c), written from the standard (ITU-T H.264 03/2005, clauses cited at each function; samples are
named p[x, y] as there) and from the reference:

  neighbour availability of a 4x4 block   6.4.10.4, 8.3.1.2      src/h264bsd_intra_prediction.c:1388-1491 (Get4x4NeighbourPels),
                                                                 :701-843 (h264bsdIntra4x4Prediction: block 5 asks mbC)
  Intra4x4 prediction                     8.3.1.2.1 - 8.3.1.2.9  :1493-1842
  Intra16x16 prediction                   8.3.3.1 - 8.3.3.4      :1000-1158
  chroma prediction                       8.3.4.1 - 8.3.4.4      :1160-1386
  Intra16x16 luma DC                      8.5.10 (8.5.6 order)   src/h264bsd_transform.c:255-338 (h264bsdProcessLumaDc)
  chroma DC                               8.5.11                 src/h264bsd_transform.c:359-401 (h264bsdProcessChromaDc)
  scaling and transform of a 4x4 block    8.5.12                 src/h264bsd_transform.c:97-234 (h264bsdProcessBlock; :184-188 is the
                                                                 residual range [-512, 511], outside of which this model raises)
  which blocks of a macroblock there are                         src/h264bsd_macroblock_layer.c:1340-1421 (ProcessResidual; :1366-1374
                                                                 with totalCoeff[24] == 0 is the RAW form of the luma DC)

reconstruct(job, base) gives the un-deblocked picture of a finished frame job (framejob.h) whose macroblocks are Intra4x4, Intra16x16
and I_PCM; every other macroblock is taken from `base`, a picture passed in.  Macroblocks are decoded in address order, the blocks of
one in the order of 6.4.3.  It also returns a census: how often the picture takes each named case (CLASSES) and each enumerated cell,
which tests/test_intra_jobs.py holds the hand-built set INTRA_SET to.

RULES holds the few choices that tests patch in memory, one at a time, to show that the set tells a wrong rule from the right one."""
import struct
from collections import Counter

A_, B_, C_, D_ = 1, 2, 4, 8                                  # FJ_AVAIL_* (framejob.h): left, above, above-right, above-left
I4x4, I16x16, IPCM = 1, 2, 3                                 # FjMbRec.kind
DC_BLOCK, CHROMA_DC_BLOCK, DC_RAW = 1 << 24, 1 << 25, 1 << 26

# Table 8-315 / equation 8-314, v(m, 0..2): positions (even, even), (odd, odd), the others
NORM_ADJUST = [(10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23)]

RULES = {
    "tr_of_block5": lambda avail: bool(avail & C_),          # the above-right samples of block 5 are macroblock C's
    "tr_replica": lambda row: row[3],                        # 8.3.1.2: p[x, -1], x = 4..7 not available -> p[3, -1]
    "luma_dc_round": lambda q6: 1 << (1 - q6),               # 8-326: the rounding term below QP 12
    "chroma_dc_halve": lambda v: v >> 1,                     # 8-330
    "chroma_dc_block1_first": "above",                       # 8.3.4.3: the block with xO > 0, yO == 0 prefers the samples above
    "plane_b_round": 32,                                     # 8-134
    "i16_dc_absent": lambda level0: 0,                       # no DC block: the DC of every Intra16x16 block is 0
    "clip_lo": lambda v: max(0, v),                          # Clip1 (5-3)
    "clip_hi": lambda v: min(255, v),
    "reject_out_of_range": True,                             # (False: count what random jobs reach, whose levels ignore the range)
}

SUM_KINDS = ("i4", "i16", "chroma")
CLASSES = (["i4_tr_differs_mode3", "i4_tr_differs_mode7", "i4_dc_left_missing_differs", "i4_dc_top_missing_differs",
            "i16_dc_left_missing_differs", "i16_dc_top_missing_differs"] +
           [f"{pl}_plane_{v}_{s}" for pl in ("luma", "chroma") for v in "bc" for s in ("neg", "zero", "pos")] +
           [f"{pl}_plane_{w}" for pl in ("luma", "chroma") for w in ("below0", "above255", "extreme")] +
           [f"luma_dc_q6_{q}_{s}" for q in ("0", "1", "ge2") for s in ("neg_odd", "neg_even", "pos")] +
           ["chroma_dc_q6_0_neg_odd", "raw_dc", "i16_dc_only", "i16_ac_only", "i16_dc_and_ac", "i16_no_residual",
            "residual_near_min", "residual_near_max"] +
           [f"{k}_sum_{w}" for k in SUM_KINDS for w in ("below0", "above255", "exact0", "exact255")])


def clip1(v):
    return RULES["clip_hi"](RULES["clip_lo"](v))


# ------------------------------------------------------------------ the job
def job_view(job):
    wmb, hmb = struct.unpack_from("<HH", job, 8)
    n, = struct.unpack_from("<I", job, 12)
    rec_off, = struct.unpack_from("<I", job, 20)
    coef_off, = struct.unpack_from("<I", job, 36)
    recs = []
    for a in range(n):
        r = job[rec_off + 32 * a:rec_off + 32 * a + 32]
        coded, coef_idx = struct.unpack_from("<II", r, 8)
        modes = [(r[24 + (z >> 1)] >> (4 * (z & 1))) & 15 for z in range(16)]
        recs.append(dict(kind=r[0], qp_y=r[1], qp_c=r[2], avail=r[3], l16=r[4] & 3, chroma=(r[4] >> 2) & 3, coded=coded, coef_idx=coef_idx, modes=modes))
    return wmb, hmb, recs, coef_off


def _block(job, coef_off, idx):
    return list(struct.unpack_from("<16h", job, coef_off + 32 * idx))


# ------------------------------------------------------------------ residual, 8.5
def _matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(len(b))) for j in range(len(b[0]))] for i in range(len(a))]


def luma_dc(levels, qp, seen=None):
    """8.5.10: the 4x4 block c of DC levels (raster) -> dcY[i][j], the DC of the luma block in row i, column j (8-324 .. 8-326)"""
    m = [[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]]
    f = _matmul(_matmul(m, [levels[4 * i:4 * i + 4] for i in range(4)]), m)
    scale, q6 = NORM_ADJUST[qp % 6][0], qp // 6
    out = [[0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            v = f[i][j] * scale
            out[i][j] = v << (q6 - 2) if qp >= 12 else (v + RULES["luma_dc_round"](q6)) >> (2 - q6)
            if seen is not None:
                sign = "pos" if v > 0 else "neg_odd" if v < 0 and v % 2 else "neg_even" if v < 0 else None
                if sign: seen["luma_dc_q6_%s_%s" % (min(q6, 2) if q6 < 2 else "ge2", sign)] += 1
    return out


def chroma_dc(levels, qp, seen=None):
    """8.5.11: c = [[c0, c1], [c2, c3]] -> dcC (8-328 .. 8-330), in the raster order of the four chroma blocks"""
    m = [[1, 1], [1, -1]]
    f = _matmul(_matmul(m, [levels[0:2], levels[2:4]]), m)
    scale, q6 = NORM_ADJUST[qp % 6][0], qp // 6
    out = []
    for i in range(2):
        for j in range(2):
            v = f[i][j] * scale
            if seen is not None and q6 == 0 and v < 0 and v % 2: seen["chroma_dc_q6_0_neg_odd"] += 1
            out.append(RULES["chroma_dc_halve"](v << q6))
    return out


def residual_block(levels, qp, dc=None, seen=None):
    """8.5.12: 16 levels (raster) -> r[y][x].  dc: the already scaled DC (Intra16x16 luma and chroma), which replaces d[0][0] (8-331).
    Raises where the reference reports an error: a residual sample outside [-512, 511]."""
    d = [[0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            v = NORM_ADJUST[qp % 6][0 if i % 2 == 0 and j % 2 == 0 else 1 if i % 2 == 1 and j % 2 == 1 else 2]
            d[i][j] = (levels[4 * i + j] * v) << (qp // 6)
    if dc is not None:
        d[0][0] = dc
    f = [[0] * 4 for _ in range(4)]
    for i in range(4):                                       # 8-338 .. 8-345: every row
        e = [d[i][0] + d[i][2], d[i][0] - d[i][2], (d[i][1] >> 1) - d[i][3], d[i][1] + (d[i][3] >> 1)]
        f[i] = [e[0] + e[3], e[1] + e[2], e[1] - e[2], e[0] - e[3]]
    r = [[0] * 4 for _ in range(4)]
    for j in range(4):                                       # 8-346 .. 8-353: every column, then 8-354
        g = [f[0][j] + f[2][j], f[0][j] - f[2][j], (f[1][j] >> 1) - f[3][j], f[1][j] + (f[3][j] >> 1)]
        h = [g[0] + g[3], g[1] + g[2], g[1] - g[2], g[0] - g[3]]
        for i in range(4):
            r[i][j] = (h[i] + 32) >> 6
    lo, hi = min(min(row) for row in r), max(max(row) for row in r)
    if (lo < -512 or hi > 511) and RULES["reject_out_of_range"]:
        raise ValueError(f"residual {lo} .. {hi} leaves [-512, 511]")
    if seen is not None:
        if -512 <= lo <= -512 + 8: seen["residual_near_min"] += 1
        if 511 - 8 <= hi <= 511: seen["residual_near_max"] += 1
    return r


ZERO = [0] * 16


def luma_xy(z):
    """6.4.3: the upper-left luma sample of block luma4x4BlkIdx = z inside its macroblock"""
    return 8 * ((z // 4) % 2) + 4 * ((z % 4) % 2), 8 * ((z // 4) // 2) + 4 * ((z % 4) // 2)


def mb_residual(job, coef_off, rec, seen=None):
    """(luma[16][16], [cb[8][8], cr[8][8]]) of one Intra4x4 / Intra16x16 macroblock, from its coefficient blocks in their stored order"""
    at, coded, qp, qc = rec["coef_idx"], rec["coded"], rec["qp_y"], rec["qp_c"]
    luma = [[0] * 16 for _ in range(16)]
    dcy = None
    if rec["kind"] == I16x16:
        n_ac = bin(coded & 0xFFFF).count("1")
        if coded & DC_BLOCK:
            lv = _block(job, coef_off, at); at += 1
            if coded & DC_RAW:
                dcy = [lv[4 * i:4 * i + 4] for i in range(4)]
                if seen is not None: seen["raw_dc"] += 1
            else:
                dcy = luma_dc(lv, qp, seen)
        if seen is not None:
            seen[("i16_dc_and_ac" if n_ac else "i16_dc_only") if coded & DC_BLOCK else ("i16_ac_only" if n_ac else "i16_no_residual")] += 1
    for z in range(16):
        x0, y0 = luma_xy(z)
        lv = ZERO
        if (coded >> z) & 1:
            lv = _block(job, coef_off, at); at += 1
        if rec["kind"] == I16x16:
            dc = dcy[y0 // 4][x0 // 4] if dcy is not None else RULES["i16_dc_absent"]((lv[0] * NORM_ADJUST[qp % 6][0]) << (qp // 6))
            r = residual_block(lv, qp, dc, seen)
        else:
            r = residual_block(lv, qp, None, seen)
        for y in range(4): luma[y0 + y][x0:x0 + 4] = r[y]
    chroma = [[[0] * 8 for _ in range(8)] for _ in range(2)]
    dcc = [0] * 8
    if coded & CHROMA_DC_BLOCK:
        lv = _block(job, coef_off, at); at += 1
        dcc = chroma_dc(lv[0:4], qc, seen) + chroma_dc(lv[4:8], qc, seen)
    for k in range(8):
        lv = ZERO
        if (coded >> (16 + k)) & 1:
            lv = _block(job, coef_off, at); at += 1
        r = residual_block(lv, qc, dcc[k], seen)
        x0, y0 = 4 * (k & 1), 4 * ((k >> 1) & 1)
        for y in range(4): chroma[k >> 2][y0 + y][x0:x0 + 4] = r[y]
    if seen is not None:
        if coded & 0x100FFFF: seen[("qp_y", qp)] += 1
        if coded & 0x2FF0000: seen[("qp_c", qc)] += 1
    return luma, chroma


# ------------------------------------------------------------------ Intra4x4 prediction, 8.3.1.2
def pred4x4(mode, p):
    """p: {(x, y): sample} of the 13 neighbouring samples that are available (after the above-right substitution);
    returns pred[y][x].  A mode that reads a sample that is not there raises KeyError: the job is not a valid one."""
    P = lambda x, y: p[(x, y)]
    top = all((x, -1) in p for x in range(4))
    left = all((-1, y) in p for y in range(4))
    out = [[0] * 4 for _ in range(4)]
    for y in range(4):
        for x in range(4):
            if mode == 0:                                    # 8.3.1.2.1 vertical
                v = P(x, -1)
            elif mode == 1:                                  # 8.3.1.2.2 horizontal
                v = P(-1, y)
            elif mode == 2:                                  # 8.3.1.2.3 DC
                if top and left: v = (sum(P(i, -1) for i in range(4)) + sum(P(-1, j) for j in range(4)) + 4) >> 3
                elif left: v = (sum(P(-1, j) for j in range(4)) + 2) >> 2
                elif top: v = (sum(P(i, -1) for i in range(4)) + 2) >> 2
                else: v = 1 << 7
            elif mode == 3:                                  # 8.3.1.2.4 diagonal down left
                v = (P(6, -1) + 3 * P(7, -1) + 2) >> 2 if x == 3 and y == 3 else (P(x + y, -1) + 2 * P(x + y + 1, -1) + P(x + y + 2, -1) + 2) >> 2
            elif mode == 4:                                  # 8.3.1.2.5 diagonal down right
                if x > y: v = (P(x - y - 2, -1) + 2 * P(x - y - 1, -1) + P(x - y, -1) + 2) >> 2
                elif x < y: v = (P(-1, y - x - 2) + 2 * P(-1, y - x - 1) + P(-1, y - x) + 2) >> 2
                else: v = (P(0, -1) + 2 * P(-1, -1) + P(-1, 0) + 2) >> 2
            elif mode == 5:                                  # 8.3.1.2.6 vertical right
                zvr, s = 2 * x - y, x - (y >> 1)
                if zvr in (0, 2, 4, 6): v = (P(s - 1, -1) + P(s, -1) + 1) >> 1
                elif zvr in (1, 3, 5): v = (P(s - 2, -1) + 2 * P(s - 1, -1) + P(s, -1) + 2) >> 2
                elif zvr == -1: v = (P(-1, 0) + 2 * P(-1, -1) + P(0, -1) + 2) >> 2
                else: v = (P(-1, y - 1) + 2 * P(-1, y - 2) + P(-1, y - 3) + 2) >> 2
            elif mode == 6:                                  # 8.3.1.2.7 horizontal down
                zhd, s = 2 * y - x, y - (x >> 1)
                if zhd in (0, 2, 4, 6): v = (P(-1, s - 1) + P(-1, s) + 1) >> 1
                elif zhd in (1, 3, 5): v = (P(-1, s - 2) + 2 * P(-1, s - 1) + P(-1, s) + 2) >> 2
                elif zhd == -1: v = (P(-1, 0) + 2 * P(-1, -1) + P(0, -1) + 2) >> 2
                else: v = (P(x - 1, -1) + 2 * P(x - 2, -1) + P(x - 3, -1) + 2) >> 2
            elif mode == 7:                                  # 8.3.1.2.8 vertical left
                s = x + (y >> 1)
                v = (P(s, -1) + P(s + 1, -1) + 1) >> 1 if y % 2 == 0 else (P(s, -1) + 2 * P(s + 1, -1) + P(s + 2, -1) + 2) >> 2
            elif mode == 8:                                  # 8.3.1.2.9 horizontal up
                zhu, s = x + 2 * y, y + (x >> 1)
                if zhu > 5: v = P(-1, 3)
                elif zhu == 5: v = (P(-1, 2) + 3 * P(-1, 3) + 2) >> 2
                elif zhu % 2 == 0: v = (P(-1, s) + P(-1, s + 1) + 1) >> 1
                else: v = (P(-1, s) + 2 * P(-1, s + 1) + P(-1, s + 2) + 2) >> 2
            else:
                raise ValueError(f"Intra4x4PredMode {mode}")
            out[y][x] = v
    return out


def block_availability(z, avail):
    """(left, top, corner, above-right) of block z under the macroblock's availability bits: 6.4.10.4 with 6.4.11 — a neighbouring
    location inside the macroblock is available when its block comes earlier in the order of 6.4.3, one to the right of the
    macroblock (x > 15, y >= 0) never is, and above the macroblock x <= 15 is macroblock B, x > 15 macroblock C"""
    x0, y0 = luma_xy(z)
    left = x0 > 0 or bool(avail & A_)
    top = y0 > 0 or bool(avail & B_)
    if x0 > 0 and y0 > 0: corner = True
    elif y0 > 0: corner = bool(avail & A_)
    elif x0 > 0: corner = bool(avail & B_)
    else: corner = bool(avail & D_)
    if y0 == 0: tr = bool(avail & B_) if x0 + 4 <= 15 else RULES["tr_of_block5"](avail)
    elif x0 + 4 > 15: tr = False
    else: tr = z not in (3, 11)                              # the only blocks whose above-right block inside the macroblock comes later
    return left, top, corner, tr


def _recon_i4x4(Y, wmb, hmb, mbx, mby, rec, res, done, seen):
    for z in range(16):
        bx, by = luma_xy(z)
        x0, y0 = 16 * mbx + bx, 16 * mby + by
        mode = rec["modes"][z]
        left, top, corner, tr = block_availability(z, rec["avail"])
        p = {}
        if top:
            for x in range(4): p[(x, -1)] = Y[y0 - 1][x0 + x]
            if tr:
                if x0 + 7 >= 16 * wmb: raise ValueError("the job calls samples to the right of the picture available")
                for x in range(4, 8): p[(x, -1)] = Y[y0 - 1][x0 + x]
            else:
                for x in range(4, 8): p[(x, -1)] = RULES["tr_replica"]([Y[y0 - 1][x0 + i] if x0 + i < 16 * wmb else None for i in range(8)])
        if left:
            for y in range(4): p[(-1, y)] = Y[y0 + y][x0 - 1]
        if corner:
            p[(-1, -1)] = Y[y0 - 1][x0 - 1]
        pred = pred4x4(mode, p)
        if seen is not None:
            seen[("i4", z, mode, left, top, corner, tr)] += 1
            # a wrong above-right rule shows only where the samples that really lie there (final ones: those of the macroblock row
            # above) give another prediction
            if mode in (3, 7) and top and not tr and by == 0 and y0 > 0 and x0 + 7 < 16 * wmb and done(x0 + 4, y0 - 1):
                q = dict(p)
                for x in range(4, 8): q[(x, -1)] = Y[y0 - 1][x0 + x]
                if pred4x4(mode, q) != pred: seen["i4_tr_differs_mode%d" % mode] += 1
            if mode == 2 and left != top:
                q = dict(p)
                if not left and x0 > 0 and done(x0 - 1, y0):
                    for y in range(4): q[(-1, y)] = Y[y0 + y][x0 - 1]
                    if pred4x4(2, q) != pred: seen["i4_dc_left_missing_differs"] += 1
                if not top and y0 > 0 and done(x0, y0 - 1):
                    for x in range(4): q[(x, -1)] = Y[y0 - 1][x0 + x]
                    if pred4x4(2, q) != pred: seen["i4_dc_top_missing_differs"] += 1
        for y in range(4):
            for x in range(4):
                Y[y0 + y][x0 + x] = _add(pred[y][x], res[by + y][bx + x], seen, "i4")


def _add(pred, res, seen, kind):
    u = pred + res
    if seen is not None:
        if u < 0: seen[kind + "_below0"] = 1
        elif u > 255: seen[kind + "_above255"] = 1
        elif u == 0: seen[kind + "_exact0"] = 1
        elif u == 255: seen[kind + "_exact255"] = 1
    return clip1(u)


# ------------------------------------------------------------------ Intra16x16 (8.3.3) and chroma (8.3.4) prediction
def _plane(p, size, seen, name):
    """8.3.3.4 (size 16) and 8.3.4.4 (size 8, 4:2:0): p maps (x, -1), (-1, y) and (-1, -1) to samples"""
    half = size // 2
    H = sum((x + 1) * (p[(half + x, -1)] - p[(half - 2 - x, -1)]) for x in range(half))
    V = sum((y + 1) * (p[(-1, half + y)] - p[(-1, half - 2 - y)]) for y in range(half))
    k = 5 if size == 16 else 34
    a = 16 * (p[(-1, size - 1)] + p[(size - 1, -1)])
    b = (k * H + RULES["plane_b_round"]) >> 6
    c = (k * V + 32) >> 6
    raw = [[(a + b * (x - (half - 1)) + c * (y - (half - 1)) + 16) >> 5 for x in range(size)] for y in range(size)]
    if seen is not None:
        top = sum(x + 1 for x in range(half)) * 255            # |H| when one half of the border is 0 and the other 255
        extreme = max((k * top + 32) >> 6, -((k * -top + 32) >> 6))
        for v, s in ((b, "b"), (c, "c")):
            seen[f"{name}_plane_{s}_{'neg' if v < 0 else 'pos' if v > 0 else 'zero'}"] += 1
        if min(map(min, raw)) < 0: seen[name + "_plane_below0"] += 1
        if max(map(max, raw)) > 255: seen[name + "_plane_above255"] += 1
        if max(abs(b), abs(c)) >= extreme - 1: seen[name + "_plane_extreme"] += 1
    return [[clip1(v) for v in row] for row in raw]


def _borders(P, x0, y0, size, avail):
    p = {}
    if avail & B_:
        for x in range(size): p[(x, -1)] = P[y0 - 1][x0 + x]
    if avail & A_:
        for y in range(size): p[(-1, y)] = P[y0 + y][x0 - 1]
    if avail & D_:
        p[(-1, -1)] = P[y0 - 1][x0 - 1]
    return p


def _dc16(p, left, top):
    """8.3.3.3"""
    st, sl = sum(p[(x, -1)] for x in range(16)) if top else 0, sum(p[(-1, y)] for y in range(16)) if left else 0
    return (st + sl + 16) >> 5 if top and left else (sl + 8) >> 4 if left else (st + 8) >> 4 if top else 1 << 7


def _recon_i16x16(Y, mbx, mby, rec, res, done, seen):
    x0, y0, avail, mode = 16 * mbx, 16 * mby, rec["avail"], rec["l16"]
    left, top = bool(avail & A_), bool(avail & B_)
    p = _borders(Y, x0, y0, 16, avail)
    if mode == 0: pred = [[p[(x, -1)] for x in range(16)] for _ in range(16)]
    elif mode == 1: pred = [[p[(-1, y)]] * 16 for y in range(16)]
    elif mode == 2:
        dc = _dc16(p, left, top)
        pred = [[dc] * 16 for _ in range(16)]
        if seen is not None and left != top:
            q = dict(p)
            if not left and x0 > 0 and done(x0 - 1, y0):
                for y in range(16): q[(-1, y)] = Y[y0 + y][x0 - 1]
                if _dc16(q, True, True) != dc: seen["i16_dc_left_missing_differs"] += 1
            if not top and y0 > 0 and done(x0, y0 - 1):
                for x in range(16): q[(x, -1)] = Y[y0 - 1][x0 + x]
                if _dc16(q, True, True) != dc: seen["i16_dc_top_missing_differs"] += 1
    else: pred = _plane(p, 16, seen, "luma")
    if seen is not None: seen[("i16", mode, left, top)] += 1
    for y in range(16):
        for x in range(16):
            Y[y0 + y][x0 + x] = _add(pred[y][x], res[y][x], seen, "i16")


def _recon_chroma(P, mbx, mby, rec, res, seen, count):
    x0, y0, avail, mode = 8 * mbx, 8 * mby, rec["avail"], rec["chroma"]
    left, top = bool(avail & A_), bool(avail & B_)
    p = _borders(P, x0, y0, 8, avail)
    if mode == 0:                                            # 8.3.4.1 - 8.3.4.3: DC per 4x4 block at (xO, yO)
        pred = [[0] * 8 for _ in range(8)]
        for kk in range(4):
            xo, yo = 4 * (kk % 2), 4 * (kk // 2)
            st = sum(p[(xo + x, -1)] for x in range(4)) if top else 0
            sl = sum(p[(-1, yo + y)] for y in range(4)) if left else 0
            if (xo, yo) == (0, 0) or (xo > 0 and yo > 0):
                dc = (st + sl + 4) >> 3 if top and left else (st + 2) >> 2 if top else (sl + 2) >> 2 if left else 1 << 7
            else:
                first = RULES["chroma_dc_block1_first"] if yo == 0 else "left"
                if first == "above": dc = (st + 2) >> 2 if top else (sl + 2) >> 2 if left else 1 << 7
                else: dc = (sl + 2) >> 2 if left else (st + 2) >> 2 if top else 1 << 7
            for y in range(4): pred[yo + y][xo:xo + 4] = [dc] * 4
            if count: seen[("chroma_dc", kk, left, top)] += 1
    elif mode == 1: pred = [[p[(-1, y)]] * 8 for y in range(8)]                  # 8.3.4.2 horizontal
    elif mode == 2: pred = [[p[(x, -1)] for x in range(8)] for _ in range(8)]    # 8.3.4.1 vertical  (intra_chroma_pred_mode 2)
    else: pred = _plane(p, 8, seen if count else None, "chroma")
    if count: seen[("chroma", mode, left, top)] += 1
    for y in range(8):
        for x in range(8):
            P[y0 + y][x0 + x] = _add(pred[y][x], res[y][x], seen, "chroma")


# ------------------------------------------------------------------ the picture
def planes_of(frame, wmb, hmb):
    """[Y, Cb, Cr] as lists of rows of Python ints, from an I420 frame (anything indexable that holds wmb * hmb * 384 bytes)"""
    W, H = 16 * wmb, 16 * hmb
    f = [int(v) for v in bytes(bytearray(frame))]
    out, at = [], 0
    for w, h in ((W, H), (W // 2, H // 2), (W // 2, H // 2)):
        out.append([f[at + w * y:at + w * y + w] for y in range(h)])
        at += w * h
    return out


def i420_bytes(picture):
    return bytes(v for P in picture for row in P for v in row)


def reconstruct(job, base=None, census=True):
    """(I420 bytes of the un-deblocked picture, Counter): Intra4x4, Intra16x16 and I_PCM macroblocks are reconstructed here, every
    other macroblock is what `base` (an I420 frame) holds.  Before anything is decoded every intra macroblock of the picture is
    filled with 77, so that nothing of `base` but its other macroblocks reaches the result."""
    wmb, hmb, recs, coef_off = job_view(job)
    pic = planes_of(base, wmb, hmb) if base is not None else [[[77] * (16 * wmb) for _ in range(16 * hmb)]] + [[[77] * (8 * wmb) for _ in range(8 * hmb)] for _ in range(2)]
    intra = [r["kind"] in (I4x4, I16x16, IPCM) for r in recs]
    assert base is not None or all(intra), "a picture with other macroblocks needs a base picture"
    for a in range(wmb * hmb):
        if intra[a]:
            for P, s in zip(pic, (16, 8, 8)):
                for y in range(s): P[s * (a // wmb) + y][s * (a % wmb):s * (a % wmb) + s] = [77] * s
    counts = Counter()
    for a, rec in enumerate(recs):
        if not intra[a]:
            continue
        mbx, mby = a % wmb, a // wmb
        done = lambda x, y: not intra[(y // 16) * wmb + x // 16] or (y // 16) * wmb + x // 16 < a       # luma position: a final sample
        if rec["kind"] == IPCM:
            raw = job[coef_off + 32 * rec["coef_idx"]:coef_off + 32 * rec["coef_idx"] + 384]
            at = 0
            for P, s in zip(pic, (16, 8, 8)):
                for y in range(s): P[s * mby + y][s * mbx:s * mbx + s] = list(raw[at + s * y:at + s * y + s])
                at += s * s
            continue
        seen = Counter() if census else None
        luma, chroma = mb_residual(job, coef_off, rec, seen)
        if rec["kind"] == I4x4: _recon_i4x4(pic[0], wmb, hmb, mbx, mby, rec, luma, done, seen)
        else: _recon_i16x16(pic[0], mbx, mby, rec, luma, done, seen)
        for k in range(2): _recon_chroma(pic[1 + k], mbx, mby, rec, chroma[k], seen, census and k == 0)
        if census:
            for kind in SUM_KINDS:                                     # per macroblock: does it take the case at all
                for w in ("below0", "above255", "exact0", "exact255"):
                    if seen.pop(f"{kind}_{w}", 0): seen[f"{kind}_sum_{w}"] = 1
            counts.update(seen)
    return i420_bytes(pic), counts


# ------------------------------------------------------------------ what the rules allow: the cells that a set must reach
def i4_modes_allowed(left, top, corner):
    """8.3.1.2: vertical, diagonal down left and vertical left need the samples above; horizontal and horizontal up the left ones;
    the three modes that use the corner need all of them; DC needs nothing"""
    return [2] + ([0, 3, 7] if top else []) + ([1, 8] if left else []) + ([4, 5, 6] if top and left and corner else [])


def cells():
    """every cell of the enumerated classes: Intra4x4 (z, mode, left, top, corner, above-right) over the 16 availability masks,
    Intra16x16 and chroma (mode, A, B), chroma DC (block, A, B)"""
    out = set()
    for avail in range(16):
        left, top, corner = bool(avail & A_), bool(avail & B_), bool(avail & D_)
        for z in range(16):
            l, t, c, tr = block_availability(z, avail)
            out |= {("i4", z, m, l, t, c, tr) for m in i4_modes_allowed(l, t, c)}
        out |= {("i16", m, left, top) for m in [2] + ([0] if top else []) + ([1] if left else []) + ([3] if left and top and corner else [])}
        out |= {("chroma", m, left, top) for m in [0] + ([1] if left else []) + ([2] if top else []) + ([3] if left and top and corner else [])}
        out |= {("chroma_dc", kk, left, top) for kk in range(4)}
    return out
