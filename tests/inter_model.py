"""Inter reconstruction as a plain integer model (test infrastructure): Python ints and lists, no numpy arithmetic, no C.

A third statement of the arithmetic, next to the three inter kernels (k_recon_inter_lb / _lq in kernels/k_recon_inter_lanes.hip.h on
kernels/inter_lane_block.hip.h, k_recon_inter in kernels/k_recon_inter.hip.h) and recon_inter / mb_residual (oracle/pixel_oracle.c), written
from the standard (ITU-T H.264 03/2005; samples are named as in Figure 8-4) and from the reference:

  luma sample interpolation      8.4.2.2.1 (8-241 .. 8-261, Table 8-12)   src/h264bsd_reconstruct.c (h264bsdInterpolate*, h264bsdPredictSamples)
  chroma sample interpolation    8.4.2.2.2 (8-266)                        src/h264bsd_reconstruct.c (h264bsdInterpolateChroma*)
  samples outside the picture    8.4.2.2 (8-239, 8-240: Clip3 of the coordinates)   src/h264bsd_reconstruct.c (h264bsdFillBlock)
  chroma DC                      8.5.11                                   src/h264bsd_transform.c (h264bsdProcessChromaDc)
  scaling and transform          8.5.12                                   src/h264bsd_transform.c (h264bsdProcessBlock)

j is computed from the HORIZONTAL sums aa, bb, b1, s1, gg, hh, as 8-247 writes it first; the kernels and the oracle go through the vertical
ones.  The residual of a block is intra_model.residual_block / chroma_dc, which state 8.5.11 and 8.5.12 already; peaks() repeats the two
butterflies only to look at their intermediates.

reconstruct(job, slots, base) gives the un-deblocked picture of a finished frame job (framejob.h): every inter macroblock is predicted
from the pictures in `slots` with the vector of each 4x4 block and the reference of its quadrant, its residual added and clipped; every
other macroblock is what `base` holds.  It also returns a census, per inter list of the job (uni: one vector, quad: one per quadrant, gen:
anything finer; copy: the whole-sample copies that no inter kernel sees) and, for the interpolation classes, per letter of Table 8-12:
how often the picture takes each case of CLASSES, which tests/test_inter_jobs.py holds the hand-built set INTER_SET to.

The bound of h264bsd_amd/csrc/hd_resid.c (bounds()) is no part of the standard.  It is stated here from its definition: the largest block's
sum of level magnitudes times the largest scale of the QP, for chroma plus the largest magnitude a scaled DC can have; at most 32735."""
import struct
from collections import Counter

import intra_model
from intra_model import NORM_ADJUST

LETTERS = (("G", "a", "b", "c"), ("d", "e", "f", "g"), ("h", "i", "j", "k"), ("n", "p", "q", "r"))      # Table 8-12: [yFracL][xFracL]
LISTS = ("uni", "quad", "gen")
H_LETTERS, V_LETTERS, J_LETTERS = "abcefgpqr", "dhnegprik", "fijkq"      # use b or s; use h or m; use j
LIMIT = 32735
NEAR = 32700                                                 # "at an end of 16 bits": within 67 of it
FAR = 32000                                                  # both halves of one register beyond this, with opposite signs

EXACT_ENDS = ["hsum_min", "hsum_max", "vsum_min", "vsum_max", "jsum_min", "jsum_max"]
PREDICTION = EXACT_ENDS + ["half_clip_lo", "half_clip_hi", "j_clip_lo", "j_clip_hi", "avg_round_up", "avg_0_0", "avg_255_255",
                           "chroma_tie", "chroma_all_0", "chroma_all_255"]
RESIDUAL = ["bound_last_step", "corner_hi", "corner_lo", "halves_opposite", "cdc_at_bound", "cdc_neg_odd_below_qpc_6", "cdc_neg_odd_decides_a_sample", "wide_in_range",
            "residual_511", "residual_m512", "sum_below0", "sum_above255", "sum_exact0", "sum_exact255"]
CLASSES = PREDICTION + RESIDUAL


def clip1(v):
    return 0 if v < 0 else 255 if v > 255 else v


def tap(a, b, c, d, e, f):
    """the six-tap filter (1, -5, 20, 20, -5, 1) of 8-241 / 8-242"""
    return a - 5 * b + 20 * c + 20 * d - 5 * e + f


# ------------------------------------------------------------------ 8.4.2.2.1: one luma sample
def luma_sample(S, x, y, xf, yf, seen=None):
    """predPartL[x, y] at whole-sample position (x, y) = G of the reference with fraction (xf, yf); S(x, y) is the reference sample at a
    location, 8-239 / 8-240 applied by the caller.  Figure 8-4: E F G H I J the row of G, A C G M R T its column; b, s the horizontal half
    samples right of G and of M, h, m the vertical ones below G and below H, j the centre."""
    letter = LETTERS[yf][xf]

    def note(cls):
        if seen is not None:
            seen[cls] += 1
            seen[("letter", letter, cls)] += 1

    def hsum(yy):                                            # b1 of the row yy (8-241): E - 5F + 20G + 20H - 5I + J
        v = tap(S(x - 2, yy), S(x - 1, yy), S(x, yy), S(x + 1, yy), S(x + 2, yy), S(x + 3, yy))
        if v == -2550: note("hsum_min")
        elif v == 10710: note("hsum_max")
        return v

    def vsum(xx):                                            # h1 of the column xx (8-242): A - 5C + 20G + 20M - 5R + T
        v = tap(S(xx, y - 2), S(xx, y - 1), S(xx, y), S(xx, y + 1), S(xx, y + 2), S(xx, y + 3))
        if v == -2550: note("vsum_min")
        elif v == 10710: note("vsum_max")
        return v

    def half(v):                                             # 8-243, 8-244
        r = (v + 16) >> 5
        if r < 0: note("half_clip_lo")
        elif r > 255: note("half_clip_hi")
        return clip1(r)

    def avg(p, q):                                           # 8-250 .. 8-261
        if (p + q) & 1: note("avg_round_up")
        elif p == q == 0: note("avg_0_0")
        elif p == q == 255: note("avg_255_255")
        return (p + q + 1) >> 1

    def j():                                                 # 8-247, first form: aa - 5 bb + 20 b1 + 20 s1 - 5 gg + hh, then 8-248
        j1 = tap(hsum(y - 2), hsum(y - 1), hsum(y), hsum(y + 1), hsum(y + 2), hsum(y + 3))
        if j1 == -214200: note("jsum_min")
        elif j1 == 475320: note("jsum_max")
        r = (j1 + 512) >> 10
        if r < 0: note("j_clip_lo")
        elif r > 255: note("j_clip_hi")
        return clip1(r)

    G = S(x, y)
    b, s, h, m = (lambda: half(hsum(y))), (lambda: half(hsum(y + 1))), (lambda: half(vsum(x))), (lambda: half(vsum(x + 1)))
    if letter == "G": return G
    if letter == "a": return avg(G, b())
    if letter == "b": return b()
    if letter == "c": return avg(S(x + 1, y), b())           # H
    if letter == "d": return avg(G, h())
    if letter == "h": return h()
    if letter == "n": return avg(S(x, y + 1), h())           # M
    if letter == "e": return avg(b(), h())
    if letter == "g": return avg(b(), m())
    if letter == "p": return avg(h(), s())
    if letter == "r": return avg(m(), s())
    if letter == "j": return j()
    if letter == "f": return avg(b(), j())
    if letter == "i": return avg(h(), j())
    if letter == "k": return avg(j(), m())
    return avg(j(), s())                                     # q


def luma_block(win, xf, yf, seen=None):
    """the 4x4 block whose 9x9 window win[r][c] holds rows y - 2 .. y + 6 of columns x - 2 .. x + 6"""
    S = lambda x, y: win[y + 2][x + 2]
    return [[luma_sample(S, x, y, xf, yf, seen) for x in range(4)] for y in range(4)]


# ------------------------------------------------------------------ 8.4.2.2.2: one chroma sample
def chroma_sample(S, x, y, xf, yf, seen=None):
    A, B, C, D = S(x, y), S(x + 1, y), S(x, y + 1), S(x + 1, y + 1)
    v = (8 - xf) * (8 - yf) * A + xf * (8 - yf) * B + (8 - xf) * yf * C + xf * yf * D      # 8-266
    if seen is not None:
        seen[("cfrac", xf, yf)] += 1
        if v & 63 == 32: seen["chroma_tie"] += 1
        if A == B == C == D == 0: seen["chroma_all_0"] += 1
        elif A == B == C == D == 255: seen["chroma_all_255"] += 1
    return (v + 32) >> 6


# ------------------------------------------------------------------ 8.5.11, 8.5.12 and the 16-bit bound
def peaks(levels, qp, dc=None):
    """(lowest, highest) intermediate of the transform of 8.5.12 — every scaled level, every butterfly output of the row and of the
    column pass, every sum with the rounding term 32 — and h[i][j] + 32, the value each sample is shifted down from"""
    d = [[(levels[4 * i + j] * NORM_ADJUST[qp % 6][0 if i % 2 == 0 and j % 2 == 0 else 1 if i % 2 and j % 2 else 2]) << (qp // 6) for j in range(4)] for i in range(4)]
    if dc is not None: d[0][0] = dc
    every = [v for row in d for v in row]
    f = []
    for i in range(4):
        e = [d[i][0] + d[i][2], d[i][0] - d[i][2], (d[i][1] >> 1) - d[i][3], d[i][1] + (d[i][3] >> 1)]
        f.append([e[0] + e[3], e[1] + e[2], e[1] - e[2], e[0] - e[3]])
        every += e + f[i]
    last = [[0] * 4 for _ in range(4)]
    for j in range(4):
        g = [f[0][j] + f[2][j], f[0][j] - f[2][j], (f[1][j] >> 1) - f[3][j], f[1][j] + (f[3][j] >> 1)]
        h = [g[0] + g[3], g[1] + g[2], g[1] - g[2], g[0] - g[3]]
        every += g + [g[0] + 32, g[1] + 32]
        for i in range(4): last[i][j] = h[i] + 32
    every += [v for row in last for v in row]
    return min(every), max(every), last


def bounds(luma, cdc, cac, qp_y, qp_c):
    """(bound of the luma blocks, bound of the chroma blocks, one luma scale step, one chroma AC step, one chroma DC step): luma / cac are
    lists of level blocks, cdc the eight DC levels or None"""
    step_l, step_c = NORM_ADJUST[qp_y % 6][1] << (qp_y // 6), NORM_ADJUST[qp_c % 6][1] << (qp_c // 6)
    step_d = NORM_ADJUST[qp_c % 6][0] << max(qp_c // 6 - 1, 0)
    sum_l = max([sum(abs(v) for v in b) for b in luma], default=0)
    sum_c = max([sum(abs(v) for v in b) for b in cac], default=0)
    sum_d = max(sum(abs(v) for v in cdc[0:4]), sum(abs(v) for v in cdc[4:8])) if cdc is not None else 0
    return sum_l * step_l, sum_c * step_c + sum_d * step_d, step_l, step_c, step_d


def bound_ok(luma, cdc, cac, qp_y, qp_c):
    bl, bc = bounds(luma, cdc, cac, qp_y, qp_c)[:2]
    return bl <= LIMIT and bc <= LIMIT


def job_view(job):
    """(wmb, hmb, records, coef_off, {macroblock: list name}) of a finished job; the record of an inter macroblock holds its sixteen vectors
    (raster 4x4 blocks) under "mv", that of any other macroblock None"""
    wmb, hmb = struct.unpack_from("<HH", job, 8)
    n, = struct.unpack_from("<I", job, 12)
    rec_off, = struct.unpack_from("<I", job, 20)
    coef_off, = struct.unpack_from("<I", job, 36)
    gen_off, n_gen = struct.unpack_from("<II", job, 68)
    mvx_off, = struct.unpack_from("<I", job, 104)
    lists = {}
    for i in range(n_gen):
        mb, uniform = struct.unpack_from("<HB", job, gen_off + 16 * i)
        lists[mb] = {1: "uni", 2: "quad", 0: "gen"}[uniform]
    recs = []
    for a in range(n):
        r = job[rec_off + 32 * a:rec_off + 32 * a + 32]
        coded, coef_idx = struct.unpack_from("<II", r, 8)
        rec = dict(kind=r[0], qp_y=r[1], qp_c=r[2], coded=coded, coef_idx=coef_idx, slots=list(r[16:20]), mv=None)
        if r[0] == 0:
            if r[4] & 0x40:                                  # FJ_PRED_UNIFORM_MV: the one vector is in the record
                rec["mv"] = [struct.unpack_from("<hh", r, 24)] * 16
            else:
                idx, = struct.unpack_from("<I", r, 28)
                rec["mv"] = [struct.unpack_from("<hh", job, mvx_off + 64 * idx + 4 * k) for k in range(16)]
        recs.append(rec)
    return wmb, hmb, recs, coef_off, lists


def mb_blocks(job, coef_off, rec):
    """({z: levels}, the eight chroma DC levels or None, {k: levels}) of an inter macroblock, from its blocks in their stored order"""
    at, coded = rec["coef_idx"], rec["coded"]
    block = lambda i: list(struct.unpack_from("<16h", job, coef_off + 32 * i))
    luma, cdc, cac = {}, None, {}
    for z in range(16):
        if (coded >> z) & 1: luma[z] = block(at); at += 1
    if coded & intra_model.CHROMA_DC_BLOCK: cdc = block(at)[0:8]; at += 1
    for k in range(8):
        if (coded >> (16 + k)) & 1: cac[k] = block(at); at += 1
    return luma, cdc, cac


def mb_residual(luma, cdc, cac, qp_y, qp_c, seen=None):
    """(luma[16][16], [cb[8][8], cr[8][8]]) of an inter macroblock.  Raises where the reference reports an error (intra_model.residual_block)
    unless intra_model.RULES["reject_out_of_range"] is off."""
    Y = [[0] * 16 for _ in range(16)]
    C = [[[0] * 8 for _ in range(8)] for _ in range(2)]
    bl, bc, step_l, step_c, step_d = bounds(list(luma.values()), cdc, list(cac.values()), qp_y, qp_c)
    ok = bl <= LIMIT and bc <= LIMIT
    lasts_l, lasts_c, dcs = {}, {}, [0] * 8
    for z, lv in luma.items():
        x0, y0 = intra_model.luma_xy(z)
        r = intra_model.residual_block(lv, qp_y)
        for y in range(4): Y[y0 + y][x0:x0 + 4] = r[y]
        lo, hi, lasts_l[z] = peaks(lv, qp_y)
        if seen is not None and ok:
            if hi >= NEAR: seen["corner_hi"] += 1
            if lo <= -NEAR: seen["corner_lo"] += 1
    if cdc is not None:
        dcs = intra_model.chroma_dc(cdc[0:4], qp_c) + intra_model.chroma_dc(cdc[4:8], qp_c)
        if seen is not None and qp_c < 6:
            for p in range(2):
                c = cdc[4 * p:4 * p + 4]
                for f in (c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3], c[0] + c[1] - c[2] - c[3], c[0] - c[1] - c[2] + c[3]):     # 8-328
                    v = f * NORM_ADJUST[qp_c % 6][0]
                    if v < 0 and v % 2:
                        seen["cdc_neg_odd_below_qpc_6"] += 1
                        # v >> 1 and the truncating v / 2 differ by one, which reaches the sample only across a step of (dc + 32) >> 6
                        if (v >> 1) % 64 == 31: seen["cdc_neg_odd_decides_a_sample"] += 1
    if cdc is not None or cac:
        for k in range(8):
            lv = cac.get(k, intra_model.ZERO)
            r = intra_model.residual_block(lv, qp_c, dcs[k])
            x0, y0 = 4 * (k & 1), 4 * ((k >> 1) & 1)
            for y in range(4): C[k >> 2][y0 + y][x0:x0 + 4] = r[y]
            lo, hi, lasts_c[k] = peaks(lv, qp_c, dcs[k])
            if seen is not None and ok:
                if hi >= NEAR: seen["corner_hi"] += 1
                if lo <= -NEAR: seen["corner_lo"] += 1
    if seen is not None and (luma or cdc is not None or cac):
        if ok:
            if (luma and LIMIT - bl < step_l) or (cac and LIMIT - bc < step_c) or (cdc is not None and not cac and LIMIT - bc < step_d): seen["bound_last_step"] += 1
            if cdc is not None and LIMIT - bc < step_d and max(abs(v) for v in dcs) > 16383: seen["cdc_at_bound"] += 1
            # one register of the packed transform holds the same position of a luma and of a chroma block: whichever blocks a kernel
            # pairs, all sixteen luma blocks against all eight chroma blocks have a position at opposite ends
            if len(lasts_l) == 16 and len(lasts_c) == 8 and all(
                    any((a[i][j] >= FAR and c[i][j] <= -FAR) or (a[i][j] <= -FAR and c[i][j] >= FAR) for i in range(4) for j in range(4))
                    for a in lasts_l.values() for c in lasts_c.values()):
                seen["halves_opposite"] += 1
            if luma: seen[("qp_y", qp_y)] += 1
            if cdc is not None or cac: seen[("qp_c", qp_c)] += 1
        else:
            flat = [v for P in [Y] + C for row in P for v in row]
            if -512 <= min(flat) and max(flat) <= 511: seen["wide_in_range"] += 1
        flat = [v for P in [Y] + C for row in P for v in row]
        if max(flat) == 511: seen["residual_511"] += 1
        if min(flat) == -512: seen["residual_m512"] += 1
    return Y, C


def _add(pred, res, seen):
    u = pred + res
    if seen is not None and res:
        if u < 0: seen["sum_below0"] += 1
        elif u > 255: seen["sum_above255"] += 1
        elif u == 0: seen["sum_exact0"] += 1
        elif u == 255: seen["sum_exact255"] += 1
    return clip1(u)


# ------------------------------------------------------------------ the picture
def reconstruct(job, slots, base, census=True):
    """(I420 bytes of the un-deblocked picture, Counter): slots = {DPB slot: I420 frame} of the reference pictures, base = an I420 frame that
    supplies every macroblock that is not an inter one.  Census keys: (list, class), (list, "letter", letter, class), (list, "cfrac", xf, yf),
    (list, "qp_y" | "qp_c", value), (list, "macroblocks")."""
    wmb, hmb, recs, coef_off, lists = job_view(job)
    W, H = 16 * wmb, 16 * hmb
    pic = intra_model.planes_of(base, wmb, hmb)
    refs = {}
    counts = Counter()
    for a, rec in enumerate(recs):
        if rec["kind"] != 0:
            continue
        mbx, mby = a % wmb, a // wmb
        name = lists.get(a, "copy")
        seen = Counter() if census else None
        luma, cdc, cac = mb_blocks(job, coef_off, rec)
        RY, RC = mb_residual(luma, cdc, cac, rec["qp_y"], rec["qp_c"], seen)
        for blk in range(16):
            bx, by = blk & 3, blk >> 2
            mvx, mvy = rec["mv"][blk]
            slot = rec["slots"][(by >> 1) * 2 + (bx >> 1)]
            if slot not in refs: refs[slot] = intra_model.planes_of(slots[slot], wmb, hmb)
            P = refs[slot]
            SY = lambda x, y, P=P[0]: P[0 if y < 0 else H - 1 if y >= H else y][0 if x < 0 else W - 1 if x >= W else x]       # 8-239, 8-240
            for y in range(4):
                for x in range(4):
                    xa, ya = 16 * mbx + 4 * bx + x, 16 * mby + 4 * by + y
                    pred = luma_sample(SY, xa + (mvx >> 2), ya + (mvy >> 2), mvx & 3, mvy & 3, seen)
                    pic[0][ya][xa] = _add(pred, RY[4 * by + y][4 * bx + x], seen)
            for c in range(2):
                SC = lambda x, y, P=P[1 + c]: P[0 if y < 0 else H // 2 - 1 if y >= H // 2 else y][0 if x < 0 else W // 2 - 1 if x >= W // 2 else x]
                for y in range(2):
                    for x in range(2):
                        xa, ya = 8 * mbx + 2 * bx + x, 8 * mby + 2 * by + y
                        pred = chroma_sample(SC, xa + (mvx >> 3), ya + (mvy >> 3), mvx & 7, mvy & 7, seen if c == 0 else None)
                        pic[1 + c][ya][xa] = _add(pred, RC[c][2 * by + y][2 * bx + x], seen)
        if census:
            counts[(name, "macroblocks")] += 1
            for key, v in seen.items():
                counts[(name,) + key if isinstance(key, tuple) else (name, key)] += v
    return intra_model.i420_bytes(pic), counts
