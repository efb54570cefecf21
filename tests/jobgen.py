"""Hand-built frame jobs with randomised content (test infrastructure).

Builds the packed per-picture work description of h264bsd_amd/csrc/framejob.h directly — no bitstream, no
parser — so that the kernels can be compared with the CPU oracle on inputs the bundled streams never produce:
all 16 luma / 64 chroma fractional positions, motion vectors far outside the picture, several reference
slots, I_PCM, every intra mode under every neighbour-availability pattern, arbitrary QPs / filter offsets /
per-MB deblocking flags.  The derived sections (schedules) are completed by the product's own
h264bsdmiJobFinalize(), i.e. by the same code the parser uses.
The second half of the file gives pictures structure on purpose (patch_typed, patch_sub8x8, patch_coherent, patch_copy_runs,
patch_window_edges, build_job(smooth=...)): what white-noise motion and content never produce.  The end of it loses macroblocks
(patch_lost, chosen_samples, build_job(pcm=...)): concealed macroblocks under chosen neighbour masks over chosen border samples;
and it describes intra macroblocks one by one (build_job(chosen=...), put_chosen, border_samples, intra_to_range): chosen kind,
availability, modes, QPs and coefficient blocks next to chosen border samples.  The last part does the same for inter reconstruction:
reference pictures of chosen samples (picture_samples, pcm_of: all-I_PCM jobs through build_job(pcm=...)) and inter macroblocks with exact
vectors, references, QPs and level blocks (build_job(inter=...), put_inter)."""
import ctypes
import struct

import numpy as np

QPC = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29,
       30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
Z_X = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]
Z_Y = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]


def z_of(x, y):
    return ((y >> 1) << 3) | ((x >> 1) << 2) | ((y & 1) << 1) | (x & 1)


def _i4_ok(avail, z):
    """the Intra4x4 modes of block z that are valid under the MB-level availability bits"""
    A, B, D = avail & 1, avail & 2, avail & 8
    bx, by = Z_X[z], Z_Y[z]
    left = bx > 0 or A
    top = by > 0 or B
    if bx > 0 and by > 0:
        tl = True
    elif by > 0:
        tl = bool(A)
    elif bx > 0:
        tl = bool(B)
    else:
        tl = bool(D)
    ok = [2]
    if top:
        ok += [0, 3, 7]
    if left:
        ok += [1, 8]
    if top and left and tl:
        ok += [4, 5, 6]
    return ok


def _i4_modes(rng, avail):
    """16 Intra4x4 modes (z order) valid for the MB-level availability bits"""
    return [int(rng.choice(_i4_ok(avail, z))) for z in range(16)]


def _coef_block(rng, ac_only=False, density=0.3, amp=12):
    c = np.zeros(16, dtype=np.int16)
    m = rng.random(16) < density
    c[m] = rng.integers(-amp, amp + 1, int(m.sum()))
    if ac_only:
        c[0] = 0
    return c


def _coef_block_smooth(rng, ac_only=False):
    """the block of a smooth picture: at most one level, of magnitude 1 or 2, at one of the three lowest raster positions"""
    c = np.zeros(16, dtype=np.int16)
    if rng.random() < 0.5:
        c[int(rng.integers(1 if ac_only else 0, 3))] = rng.choice([-2, -1, 1, 2])
    return c


LS2 = [16, 18, 20, 23, 25, 29]      # the largest level scale of qp % 6 (8.5.9), LS0 the scale of the chroma DC
LS0 = [10, 11, 13, 14, 16, 18]


def _to_bound(rng, coefs, first, n_luma, has_cdc, n_cac, qp_y, qp_c):
    """Rescale the levels of an inter macroblock so that the parser's magnitude bound (hd_resid.c: the largest block's sum of level magnitudes x
    the largest scale, <= 32735 per plane) lands within +-15 % of its limit: the macroblocks on either side of FJ_CODED_WIDE, and
    intermediates that use most of 16 bits on the packed side of it."""
    def rescale(lo, hi, scale, extra=0.0):
        blk = coefs[lo:hi].astype(np.int64)
        tot = np.abs(blk).reshape(-1, 16).sum(axis=1).max() if hi > lo else 0      # the bound is per block: the LARGEST block's sum
        if tot == 0:
            return
        target = rng.uniform(0.85, 1.15) * 32735.0 - extra
        f = max(0.0, target) / (tot * scale)
        new = np.clip(np.rint(blk * f), -2047, 2047).astype(np.int16)
        if np.abs(new).sum() == 0:
            new[np.argmax(np.abs(blk))] = 1
        coefs[lo:hi] = new
    o = 16 * first
    rescale(o, o + 16 * n_luma, LS2[qp_y % 6] << (qp_y // 6))
    o += 16 * n_luma
    dc_max = 0.0
    if has_cdc:
        q6 = qp_c // 6
        dc_max = float(np.abs(coefs[o:o + 8].astype(np.int64)).sum() * LS0[qp_c % 6] * (1 << (q6 - 1 if q6 >= 1 else 0)))
        o += 16
    rescale(o, o + 16 * n_cac, LS2[qp_c % 6] << (qp_c // 6), dc_max)


def draw_ramps(rng):
    """the ramp of a smooth picture (_pcm_gradient): per plane a level and the slopes in x and y.  build_job(smooth=True) draws one
    per picture; smooth=<what this returns> gives several pictures of a sequence the same one, so that an I_PCM macroblock
    continues what its inter neighbours fetch from the reference picture"""
    return [(int(rng.integers(0, 590)), *(rng.choice([0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 8], 2) * rng.choice([-1, 1], 2))) for _ in range(3)]


def _pcm_gradient(rng, ramps, mbx, mby):
    """384 I_PCM samples that hold ramps instead of noise, with +-1 of noise on top.  Eight times in ten the macroblock is a window on
    the picture's own ramp (ramps: per plane a level, a slope in x and one in y, folded back at -20 and 275 and cut off at 0 and 255),
    which neighbouring I_PCM macroblocks continue: slopes that run on across a strength-4 edge, and flat runs at 0 and 255
    with a slope next to them, where the filter's clip255 saturates.  Otherwise it is a ramp of its own: per plane a base level
    (often near 0 or near 255) and a slope of up to 6 levels per sample in each direction."""
    out = []
    own = rng.random() >= 0.8
    for plane, size in enumerate((16, 8, 8)):
        yy, xx = np.mgrid[0:size, 0:size]
        if own:
            where = rng.random()
            base = rng.integers(-12, 8) if where < 0.3 else rng.integers(248, 268) if where < 0.6 else rng.integers(20, 236)
            sx, sy = rng.integers(-6, 7, 2) * (rng.random(2) < 0.7)
            v = base + sx * xx + sy * yy
        else:
            g0, sx, sy = ramps[plane]
            v = (g0 + sx * (xx + size * mbx) + sy * (yy + size * mby)) % 590
            v = np.where(v < 295, v, 589 - v) - 20
        out.append(np.clip(v + rng.integers(-1, 2, (size, size)), 0, 255).astype(np.uint8).ravel())
    return np.concatenate(out)


def build_job(lib, rng, wmb, hmb, cur_slot, n_slots, ref_slots, *, p_inter=0.6, p_pcm=0.03, mv_range=None, any_deblock=True, patch=None, near_bound=False,
              smooth=False, extra_blocks=0, pcm=None, chosen=None, inter=None):
    """One random picture.  ref_slots: slots holding valid pictures (empty -> intra only).
    patch(recs, mvs): called on the records [n][32] and the dense vectors [n][16][2] before the job is finished — a finished
    job carries its vectors in the records and the sparse section (framejob.h), the dense array here is only h264bsdmiJobFinalize's input.
    smooth: content that opens the deblocking filter — few and small coefficients, I_PCM macroblocks that hold ramps (_pcm_gradient), so
    that neighbouring samples usually pass the alpha / beta gates at mid QPs.
    extra_blocks: that many more coefficient blocks (one level of +-1 each) behind the last macroblock's; patch is then called as
    patch(recs, mvs, first) with the index of the first of them, for macroblocks it wants to give a coded block (coef_idx, bytes 12..15).
    pcm: {macroblock address: 384 samples (Y[256], Cb[64], Cr[64], raster)} — these macroblocks are I_PCM with exactly those samples.
    chosen: {macroblock address: description of an Intra4x4 / Intra16x16 macroblock (put_chosen)} — these macroblocks are exactly that.
    inter: {macroblock address: description of an inter macroblock (put_inter)} — these macroblocks are exactly that.
    None of pcm, chosen and inter changes what a seed draws for the other macroblocks' records."""
    coef_block = _coef_block_smooth if smooth else _coef_block
    ramps = smooth if isinstance(smooth, list) else draw_ramps(rng) if smooth else None
    n = wmb * hmb
    rec_off, mv_off = 128, 128 + n * 32
    coef_off = mv_off + n * 64
    cap = coef_off + (n * 27 + 2 + extra_blocks) * 32 + (n + 2) * 4 + n * 2 + n * 16 + n * 2 + n * 64 + 4096
    buf = np.zeros(cap, dtype=np.uint8)
    recs = buf[rec_off:rec_off + n * 32].reshape(n, 32)
    mvs = buf[mv_off:mv_off + n * 64].view(np.int16).reshape(n, 16, 2)
    coefs = buf[coef_off:].view(np.int16)
    nblk = 0
    mvr = mv_range if mv_range is not None else (wmb * 16 * 4 + 200)
    for a in range(n):
        x, y = a % wmb, a // wmb
        r = recs[a]
        qp = int(rng.integers(0, 52)) if not smooth or rng.random() < 0.2 else int(rng.integers(18, 52))      # (smooth: mostly QPs at which alpha and beta are not 0)
        cqp = int(rng.integers(-12, 13))
        r[1] = qp
        r[2] = QPC[min(51, max(0, qp + cqp))]
        r[20] = np.int8(cqp).view(np.uint8)
        r[6] = np.int8(2 * rng.integers(-6, 7)).view(np.uint8)
        r[7] = np.int8(2 * rng.integers(-6, 7)).view(np.uint8)
        dbk = 0
        if any_deblock and rng.random() < 0.9:
            dbk = 4 | (1 if x > 0 and rng.random() < 0.9 else 0) | (2 if y > 0 and rng.random() < 0.9 else 0)
        r[5] = dbk
        struct.pack_into("<I", r, 12, nblk)
        u = rng.random()
        coded = 0
        if pcm is not None and a in pcm:
            r[0], r[1], r[2] = 3, 0, QPC[min(51, max(0, cqp))]
            buf[coef_off + 32 * nblk: coef_off + 32 * nblk + 384] = np.asarray(pcm[a], dtype=np.uint8).reshape(384)
            nblk += 12
        elif chosen is not None and a in chosen:
            coded, nblk = put_chosen(r, chosen[a], coefs, nblk, x, y, wmb)
        elif inter is not None and a in inter:
            coded, nblk = put_inter(r, mvs[a], inter[a], coefs, nblk)
        elif ref_slots and u < p_inter:
            r[0] = 0                                                   # inter
            style = rng.random()
            if style < 0.35:                                           # uniform, often whole-sample
                mv = rng.integers(-mvr, mvr + 1, 2)
                if rng.random() < 0.5:
                    mv = (mv // 8) * 8
                mvs[a, :, :] = mv
                r[16:20] = rng.choice(ref_slots)
            else:                                                      # per-4x4 vectors, per-quadrant references
                base = rng.integers(-mvr, mvr + 1, 2)
                mvs[a] = base + rng.integers(-40, 41, (16, 2))
                r[16:20] = rng.choice(ref_slots, 4)
            if rng.random() < 0.5:
                for z in range(16):
                    if rng.random() < 0.3:
                        coefs[16 * nblk:16 * nblk + 16] = coef_block(rng); nblk += 1; coded |= 1 << z
                if rng.random() < 0.5:
                    cdc = np.zeros(16, dtype=np.int16); cdc[:8] = rng.integers(-1, 2, 8) if smooth else rng.integers(-6, 7, 8)
                    coefs[16 * nblk:16 * nblk + 16] = cdc; nblk += 1; coded |= 1 << 25
                    for k in range(8):
                        if rng.random() < 0.3:
                            coefs[16 * nblk:16 * nblk + 16] = coef_block(rng, ac_only=True); nblk += 1; coded |= 1 << (16 + k)
                if near_bound and coded:
                    first = struct.unpack_from("<I", r, 12)[0]
                    _to_bound(rng, coefs, first, bin(coded & 0xFFFF).count("1"), (coded >> 25) & 1, bin((coded >> 16) & 0xFF).count("1"), int(r[1]), int(r[2]))
        elif u < p_inter + p_pcm or (not ref_slots and u < p_pcm):
            r[0] = 3                                                   # I_PCM: 384 raw samples = 12 blocks
            r[1] = 0
            r[2] = QPC[min(51, max(0, cqp))]
            buf[coef_off + 32 * nblk: coef_off + 32 * nblk + 384] = _pcm_gradient(rng, ramps, x, y) if smooth else rng.integers(0, 256, 384, dtype=np.uint8)
            nblk += 12
        else:
            avail = (1 if x > 0 else 0) | (2 if y > 0 else 0) | (4 if y > 0 and x + 1 < wmb else 0) | (8 if x > 0 and y > 0 else 0)
            if rng.random() < 0.3:
                avail &= int(rng.integers(0, 16))                      # pretend slice boundaries
            r[3] = avail
            cmodes = [0] + ([1] if avail & 1 else []) + ([2] if avail & 2 else []) + ([3] if (avail & 11) == 11 else [])
            chroma_mode = int(rng.choice(cmodes))
            if rng.random() < 0.55:
                r[0] = 1                                               # Intra4x4
                modes = _i4_modes(rng, avail)
                for z in range(16):
                    r[24 + (z >> 1)] |= modes[z] << ((z & 1) * 4)
                r[4] = chroma_mode << 2
                for z in range(16):
                    if rng.random() < 0.4:
                        coefs[16 * nblk:16 * nblk + 16] = coef_block(rng); nblk += 1; coded |= 1 << z
            else:
                r[0] = 2                                               # Intra16x16
                lmodes = [2] + ([0] if avail & 2 else []) + ([1] if avail & 1 else []) + ([3] if (avail & 11) == 11 else [])
                r[4] = int(rng.choice(lmodes)) | (chroma_mode << 2)
                if rng.random() < 0.7:
                    coefs[16 * nblk:16 * nblk + 16] = rng.integers(-1, 2, 16) * (rng.random(16) < 0.15) if smooth else rng.integers(-10, 11, 16)
                    nblk += 1; coded |= 1 << 24
                if rng.random() < 0.5:
                    for z in range(16):
                        if rng.random() < 0.5:
                            coefs[16 * nblk:16 * nblk + 16] = coef_block(rng, ac_only=True); nblk += 1; coded |= 1 << z
            if rng.random() < 0.6:
                cdc = np.zeros(16, dtype=np.int16); cdc[:8] = rng.integers(-1, 2, 8) if smooth else rng.integers(-6, 7, 8)
                coefs[16 * nblk:16 * nblk + 16] = cdc; nblk += 1; coded |= 1 << 25
                for k in range(8):
                    if rng.random() < 0.3:
                        coefs[16 * nblk:16 * nblk + 16] = coef_block(rng, ac_only=True); nblk += 1; coded |= 1 << (16 + k)
        struct.pack_into("<I", r, 8, coded)
    if extra_blocks:
        first_extra = nblk
        for _ in range(extra_blocks):
            coefs[16 * nblk + int(rng.integers(0, 3))] = rng.choice([-1, 1]); nblk += 1
    if patch is not None:
        patch(recs, mvs, first_extra) if extra_blocks else patch(recs, mvs)
    struct.pack_into("<IIHHIBBBBIII", buf, 0, 0x314A4648, 0, wmb, hmb, n, cur_slot, 0, n_slots, 0, rec_off, mv_off, 0)
    struct.pack_into("<I", buf, 36, coef_off)
    rc = lib.h264bsdmiJobFinalize(ctypes.c_void_p(buf.ctypes.data), cap, nblk)
    assert rc == 0
    total = struct.unpack_from("<I", buf, 4)[0]
    return bytes(buf[:total])


# ------------------------------------------------------------------ structured pictures (patch= callables of build_job)
# Random jobs have white-noise motion: no macroblock with one vector per quadrant, no partition type but 8x8, no copy run
# longer than one macroblock, hardly a pair of neighbours whose vectors differ by less than 6.  The patches below rewrite
# the inter macroblocks of a picture (draw it with p_inter=1) so that those paths are taken on purpose.
P_SKIP, P_16x16, P_16x8, P_8x16, P_8x8, I_4x4, I_16x16_BASE, I_PCM = 0, 1, 2, 3, 4, 6, 7, 31   # the reference's mbType_e
FJ_COPY_RUN = 8                                                       # framejob.h
NEAR = np.array([-4, -3, 0, 3, 4])                                    # vector differences on both sides of the strength threshold of 4


def _patch_partitions(recs, mvs16, rng):
    """give every inter macroblock of a jobgen picture (records and dense vectors, before the job is finished) a macroblock
    type (Skip / 16x16 / 16x8 / 8x16 / 8x8) with motion and references to match, and the FJ_PARTS_* hint the parser would
    set; returns the types"""
    n = recs.shape[0]
    mvs = mvs16.reshape(n, 4, 4, 2)                                   # [mb][by][bx][xy], raster
    types = []
    for a in range(n):
        if recs[a, 0] != 0:
            types.append(I_4x4 if recs[a, 0] in (1, 3) else I_16x16_BASE)
            continue
        t = int(rng.choice([P_SKIP, P_16x16, P_16x8, P_8x16, P_8x8]))
        base = rng.integers(-40, 41, 2)
        small = lambda: base + rng.integers(-6, 7, 2)                 # differences around the threshold of 4 quarter samples
        refs = recs[a, 16:20].copy()
        if t in (P_SKIP, P_16x16):
            mvs[a, :, :] = small(); refs[:] = refs[0]; parts = 1
        elif t == P_16x8:
            mvs[a, :2] = small(); mvs[a, 2:] = small(); refs[1] = refs[0]; refs[3] = refs[2]; parts = 2
        elif t == P_8x16:
            mvs[a, :, :2] = small(); mvs[a, :, 2:] = small(); refs[2] = refs[0]; refs[3] = refs[1]; parts = 3
        else:
            for by in range(4):
                for bx in range(4): mvs[a, by, bx] = small()
            parts = 0
        recs[a, 16:20] = refs
        recs[a, 4] = (int(recs[a, 4]) & 0x8F) | (parts << 4)
        types.append(t)
    return types


def mb_types(blob):
    """the reference's mbType of every macroblock of a finished job, as far as its deblocking filter tells types apart
    (h264bsd_deblocking.c:1254-1345: intra or not, and for inter macroblocks one partition / 16x8 / 8x16 / anything else):
    the record's kind and FJ_PARTS_* bits say exactly that"""
    n = struct.unpack_from("<I", blob, 12)[0]
    recs = np.frombuffer(blob, dtype=np.uint8, count=n * 32, offset=struct.unpack_from("<I", blob, 20)[0]).reshape(n, 32)
    by_parts = [P_8x8, P_16x16, P_16x8, P_8x16]
    return [by_parts[(int(r[4]) >> 4) & 3] if r[0] == 0 else I_4x4 if r[0] in (1, 3) else I_16x16_BASE for r in recs]


def _uncode(recs, a):
    recs[a, 8:12] = 0


def patch_typed(rng, p_uncoded=0.6, p_damage=0.25):
    """_patch_partitions, most macroblocks without coefficients (a coded block hides the motion rule), and the type that real damage
    produces (pixel_oracle.c bs_of, FJ_PRED_PARTS): a 16x16 / 16x8 / 8x16 TYPE whose vectors nevertheless differ by 4 or more
    inside a partition — the strength of those inner edges must come from the type"""
    def patch(recs, mvs16):
        _patch_partitions(recs, mvs16, rng)
        mvs = mvs16.reshape(-1, 4, 4, 2)
        for a in range(recs.shape[0]):
            if recs[a, 0] != 0:
                continue
            if rng.random() < p_uncoded:
                _uncode(recs, a)
            parts = (int(recs[a, 4]) >> 4) & 3
            if parts and rng.random() < p_damage:
                if rng.random() < 0.5:                                # one vector per quadrant (the quadrant list), or per 4x4 block
                    for q in range(4):
                        mvs[a, 2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2] += rng.choice([-5, -4, 0, 4, 6], 2).astype(np.int16)
                else:
                    mvs[a] += rng.choice([-5, -4, 0, 3, 4], (4, 4, 2)).astype(np.int16)
    return patch


def patch_sub8x8(rng, p_uncoded=0.7):
    """P_8x8 macroblocks (FJ_PARTS_8x8: every inner edge compares motion) whose quadrants are split 8x8 / 8x4 / 4x8 / 4x4, the
    vectors of the sub-partitions NEAR their quadrant's and the quadrants' NEAR the macroblock's; the quadrants mostly share
    their reference"""
    def patch(recs, mvs16):
        mvs = mvs16.reshape(-1, 4, 4, 2)
        for a in range(recs.shape[0]):
            if recs[a, 0] != 0:
                continue
            if rng.random() < p_uncoded:
                _uncode(recs, a)
            base = rng.integers(-24, 25, 2)
            if rng.random() < 0.8:
                recs[a, 16:20] = recs[a, 16]
            recs[a, 4] = int(recs[a, 4]) & 0x8F
            for q in range(4):
                qb = base + rng.choice(NEAR, 2)
                sub = int(rng.integers(0, 4))                         # 8x8, 8x4, 4x8, 4x4
                d = rng.choice(NEAR, (2, 2, 2))
                if sub == 0: d[:] = 0
                elif sub == 1: d[:, 1] = d[:, 0]
                elif sub == 2: d[1, :] = d[0, :]
                mvs[a, 2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2] = qb + d
    return patch


def _steps(rng, shape):
    """values of NEAR, 0 four times in ten: fields in which a macroblock often has BOTH neighbours within 3"""
    return rng.choice(NEAR, shape, p=[0.15, 0.15, 0.4, 0.15, 0.15])


def patch_coherent(rng, wmb, p_coded=0.3, p_split=0.15, whole=False, still=False):
    """One base vector per picture; each macroblock's one vector differs from its left and from its upper neighbour's by a value of
    NEAR per component, its reference is the left (first column: upper) neighbour's with probability
    0.8.  Most macroblocks have no coefficients; p_coded of them get ONE coded 4x4 block on an edge of the macroblock (from
    build_job's extra_blocks), p_split are P_8x8 with some vectors NEAR their one.  whole: every vector on the whole-sample grid of luma
    and chroma (steps of 8: the neighbours then differ by 0 or by more than 4), which makes copy macroblocks of them; still: the base
    vector is zero (the picture mostly repeats its reference in place, next to what its own intra macroblocks add).
    This is what fj_dbk_trivial (hd_core.c) proves strength-free or not, in both of its branches, and the >= 4 of k_dbk."""
    def patch(recs, mvs16, first_extra):
        n = recs.shape[0]
        hmb = n // wmb
        step = 8 if whole else 1
        base = rng.integers(-16, 17, 2) * step * (not still)
        # every component a value that is a step of NEAR away from the left AND from the upper neighbour's (one always exists: the two
        # neighbours are each a step of NEAR away from the upper-left one); no step is the likeliest, so that a macroblock is often
        # within 3 of BOTH neighbours, which the proof needs
        weight = dict(zip((-4, -3, 0, 3, 4), (0.12, 0.12, 0.52, 0.12, 0.12)))
        field = np.zeros((hmb, wmb, 2), dtype=int)
        for y in range(hmb):
            for x in range(wmb):
                for c in range(2):
                    nbs = ([field[y, x - 1, c]] if x else []) + ([field[y - 1, x, c]] if y else [])
                    cands = [v for v in range(-80, 81) if all(v - p in weight for p in nbs)] if nbs else [0]
                    w = np.array([np.prod([weight[v - p] for p in nbs]) for v in cands])
                    field[y, x, c] = rng.choice(cands, p=w / w.sum())
        field = base + field * step
        slots = sorted({int(v) for v in recs[recs[:, 0] == 0][:, 16:20].ravel()})
        extra = first_extra
        for a in range(n):
            if recs[a, 0] != 0:
                continue
            x, y = a % wmb, a // wmb
            nb = a - 1 if x else a - wmb if y else None
            ref = int(recs[nb, 16]) if nb is not None and recs[nb, 0] == 0 and rng.random() < 0.8 else int(rng.choice(slots))
            recs[a, 16:20] = ref
            recs[a, 4] = (int(recs[a, 4]) & 0x8F) | (1 << 4)
            mvs16[a] = field[y, x]
            _uncode(recs, a)
            u = rng.random()
            if u < p_coded:
                bx, by = [(0, int(rng.integers(0, 4))), (3, int(rng.integers(0, 4))), (int(rng.integers(0, 4)), 0), (int(rng.integers(0, 4)), 3)][int(rng.integers(0, 4))]
                struct.pack_into("<I", recs[a], 8, 1 << z_of(bx, by))
                struct.pack_into("<I", recs[a], 12, extra)
                extra += 1
            elif u < p_coded + p_split:
                recs[a, 4] = int(recs[a, 4]) & 0x8F
                mvs16[a] += (_steps(rng, (16, 2)) * (rng.random((16, 1)) < 0.4)).astype(np.int16)
    return patch


def copy_stretches():
    """The stretches of equal copy macroblocks that the structured set lays out, [(length, slot index, (dx, dy) in luma samples, what
    ends it)]: every length 1 .. 2 * FJ_COPY_RUN + 1 with zero motion and 1 .. FJ_COPY_RUN + 2 with a displacement (fj_copy_runs
    cuts them into runs of at most FJ_COPY_RUN), displacements with dx % 4 == 0 and == 2 and with odd and even dy / 2, ended by
    another slot, another vector or a macroblock that is no copy"""
    disp = [(4, 2), (-6, -2), (2, 4), (-8, 8), (16, 0), (-16, -4), (18, 2), (-18, 6), (14, -6), (-2, 0)]
    ends = ["slot", "mv", "noncopy"]
    out = [(length, k % 2, (0, 0), ends[k % 3]) for k, length in enumerate(range(1, 2 * FJ_COPY_RUN + 2))]
    out += [(length, (k + 1) % 2, disp[k % len(disp)], ends[(k + 1) % 3]) for k, length in enumerate(range(1, FJ_COPY_RUN + 3))]
    return out


def _place(a, wmb, n, stretch):
    """where a stretch goes when the layout has reached address a (None: it does not fit any more).  Zero motion: right there, on
    across row ends — those of two or three macroblocks in the last column of a row: a run that starts there and goes on in
    the next row.  Displaced: inside one row where the row is long enough — at its end when dx > 0, so that the run's later
    macroblocks reach across the right border, else at the start of what is left of it (dx < 0 from column 0: the first ones reach
    across the left border)."""
    length, _slot, d, _end = stretch
    if d != (0, 0) and length <= wmb:
        if a % wmb + length > wmb: a += wmb - a % wmb
        if d[0] > 0: a += wmb - a % wmb - length
    elif d == (0, 0) and length in (2, 3) and wmb > 1:
        a += wmb - 1 - a % wmb
    return a if a + length <= n else None


def plan_copy_pictures(sizes):
    """deal copy_stretches() out to pictures of the given sizes [(wmb, hmb)]: the longest first, each to the first picture in which it
    still fits (a displaced one: whose rows hold it), narrow pictures first.  Returns the stretches of every picture, in layout order."""
    plans, at = [[] for _ in sizes], [0] * len(sizes)
    for st in sorted(copy_stretches(), key=lambda st: (st[2] == (0, 0), -st[0])):
        for i in sorted(range(len(sizes)), key=lambda i: (sizes[i][0], sizes[i][0] * sizes[i][1])):
            w, n = sizes[i][0], sizes[i][0] * sizes[i][1]
            a = _place(at[i], w, n, st)
            if a is not None and (st[2] == (0, 0) or st[0] <= w):
                plans[i].append(st)
                at[i] = a + st[0] + 1
                break
        else:
            raise ValueError(f"no room for the stretch {st}")
    return plans


def patch_copy_runs(wmb, stretches=(), whole_picture=None, coded_mb=None):
    """Whole-sample one-vector macroblocks without coefficients, in the given stretches (plan_copy_pictures) laid out in address order
    by _place(); the macroblocks in between keep what build_job drew.  Rows 0 and hmb - 1 with dy != 0 cross the upper and lower
    border.  (A run whose FIRST macroblock is inside the picture and whose later ones cross a border exists for the right border
    only: addresses grow to the right, so it is the first ones that cross the left border, and all of a run cross the upper or
    lower one together.)
    whole_picture = slot: the whole picture is ONE zero-motion stretch from that slot instead; coded_mb: but for that macroblock, which
    gets one coded block (build_job's extra_blocks)."""
    def patch(recs, mvs16, first_extra=None):
        n = recs.shape[0]
        slots = sorted({int(v) for v in recs[recs[:, 0] == 0][:, 16:20].ravel()})

        def put(a, slot, d):
            recs[a, 0], recs[a, 4] = 0, 1 << 4
            recs[a, 8:12] = 0
            recs[a, 16:20] = slot
            mvs16[a] = (4 * d[0], 4 * d[1])

        if whole_picture is not None:
            for a in range(n): put(a, whole_picture, (0, 0))
            if coded_mb is not None:
                struct.pack_into("<I", recs[coded_mb], 8, 1 << 6)
                struct.pack_into("<I", recs[coded_mb], 12, first_extra)
            return
        a = 0
        for st in stretches:
            length, si, d, end = st
            a = _place(a, wmb, n, st)
            slot = slots[si % len(slots)]
            if a and a % wmb: mvs16[a - 1] += (1, 2)                  # (whatever lies in front of it is not its continuation)
            for b in range(a, a + length): put(b, slot, d)
            a += length
            if a >= n: break
            if end == "slot" and len(slots) > 1: put(a, slots[(si + 1) % len(slots)], d)
            elif end == "mv" or end == "slot": put(a, slot, (d[0] + 2, d[1] - 2))
            else: recs[a, 0] = 0; mvs16[a] = (4 * d[0] + 1, 4 * d[1] + 2)         # fractional: the general list
            a += 1
    return patch


FRACTIONS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 2), (3, 1), (2, 3), (1, 2)]    # (fx, fy): whole, horizontal, vertical, both


def window_targets(size):
    """Where patch_window_edges puts one end of a reference window along an axis of `size` luma samples: (plane, end, position) —
    the first column / row of the luma window (block - 2) and of the chroma window at -1, 0, +1, the last (luma: block + 3,
    chroma: block + 1) at size - 2, size - 1, size (chroma: of size / 2): one sample inside, on the edge, one outside."""
    out = []
    for plane, s in (("luma", size), ("chroma", size // 2)):
        out += [(plane, "first", t) for t in (-1, 0, 1)] + [(plane, "last", t) for t in (s - 2, s - 1, s)]
    return out


def copy_targets(size):
    """where patch_window_edges puts the first sample of a copy macroblock's source block along an axis of `size` samples"""
    return [-2, 0, 2, size - 18, size - 16, size - 14]


def block_targets(size):
    """... and the first sample of a whole-sample 4x4 block"""
    return [-1, 0, 1, size - 5, size - 4, size - 3]


def _edge_component(pos, block, target, frac):
    """the vector component (quarter samples) that puts the window of a block of `block` luma samples at luma position `pos` where
    target = (plane, end, position) says, with the luma fraction frac (0..3).  A chroma target fixes mv >> 3; the fraction's
    third bit is then free and set so that the chroma window really reaches one sample further (chroma fraction != 0)."""
    plane, end, t = target
    if plane == "luma":
        whole = t + 2 - pos if end == "first" else t - (block + 2) - pos
        return 4 * whole + frac
    whole = t - pos // 2 if end == "first" else t - block // 2 - pos // 2
    return 8 * whole + (frac if frac else 4 if end == "last" else 0)


def patch_window_edges(rng, wmb, first=0):
    """Every inter macroblock gets reference windows whose ends lie one sample inside, on, and one sample outside a picture border
    (window_targets), horizontally and vertically at once, so corners occur too: the flip between the in-picture fast paths
    and the clamped gathers (lfast / cfast in the staging of k_recon_inter_lb / _lq, the x0 test of k_copy).  Macroblocks take turns between one
    vector (16x16 window), one vector per quadrant (the window of one 8x8 quadrant is placed, the others get vectors NEAR) and
    one per 4x4 block; the fraction class cycles through FRACTIONS.
    Luma inside / chroma outside cannot be placed: the luma window [X - 2, X + B + 2] of a block at X contains twice the
    chroma window [X >> 1, (X >> 1) + B / 2] (2 * (X >> 1) >= X - 1 and 2 * (X >> 1) + B <= X + B), so chroma leaves the
    picture only where luma does.  The other way round (chroma targets) occurs all the time."""
    def patch(recs, mvs16):
        n = recs.shape[0]
        hmb = n // wmb
        tx, ty = window_targets(16 * wmb), window_targets(16 * hmb)
        mvs = mvs16.reshape(n, 4, 4, 2)
        k = nb = nc = first                                         # (nb, nc: the whole-sample 4x4 blocks and the copies take turns of their own)
        for a in range(n):
            if recs[a, 0] != 0:
                continue
            path, j = k % 3, k // 3                                   # 5 and 7 are coprime with 12: the three indices drift apart
            targ_x, targ_y = tx[j % 12], ty[(5 * j + j // 12) % 12]
            fx, fy = FRACTIONS[(7 * j + j // 144) % len(FRACTIONS)]
            k += 1
            if rng.random() < 0.7:
                _uncode(recs, a)
            recs[a, 16:20] = recs[a, 16]
            block = (16, 8, 4)[path]
            bx, by = (0, 0) if path == 0 else (int(rng.integers(0, 16 // block)), int(rng.integers(0, 16 // block)))
            px, py = 16 * (a % wmb) + block * bx, 16 * (a // wmb) + block * by
            mv = np.array([_edge_component(px, block, targ_x, fx), _edge_component(py, block, targ_y, fy)])
            if path == 2 and (fx, fy) == (0, 0):
                # whole samples, per 4x4 block: k_recon_inter reads the block itself where it lies inside the picture — its first
                # sample at -1, 0, +1, its last at size - 2, size - 1, size
                mv = np.array([4 * (block_targets(16 * wmb)[nb % 6] - px), 4 * (block_targets(16 * hmb)[(nb // 6 + nb) % 6] - py)])
                nb += 1
            if path == 0 and (fx, fy) == (0, 0) and j % 2:
                # whole samples: make it a copy macroblock (vector a multiple of 8, no coefficients) whose 16x16 block starts at
                # -2, 0, +2 or ends at size - 2, size, size + 2 (displacements are even): the x0 test of k_copy
                _uncode(recs, a)
                cx, cy = copy_targets(16 * wmb)[nc % 6], copy_targets(16 * hmb)[(nc // 6 + nc) % 6]
                nc += 1
                mv = np.array([4 * (cx - px), 4 * (cy - py)])
            if path == 0:
                mvs[a] = mv; parts = 1
            elif path == 1:
                for q in range(4):
                    mvs[a, 2 * (q >> 1):2 * (q >> 1) + 2, 2 * (q & 1):2 * (q & 1) + 2] = mv + rng.choice(NEAR, 2) + (5, 0)
                mvs[a, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = mv
                parts = 0
            else:
                mvs[a] = mv + rng.choice(NEAR, (4, 4, 2)) + (0, 5)
                mvs[a, by, bx] = mv
                parts = 0
            recs[a, 4] = (int(recs[a, 4]) & 0x8F) | (parts << 4)
    return patch


# ------------------------------------------------------------------ lost macroblocks (patch_lost, chosen_samples)
# No random job holds a concealed macroblock.  patch_lost rewrites the macroblocks that a decoded mask leaves out the way the
# parser's conceal_one (hd_core.c) does when the access unit ends; chosen_samples gives the surviving I_PCM macroblocks (build_job's
# pcm=) the borders that the concealment arithmetic is sensitive to.
FJ_MB_CONCEAL_I, FJ_MB_CONCEAL_P = 4, 5
CONTENTS = ["noise", "split", "flat0", "flat255", "ramp"]


def chosen_samples(content, rng, mbx=0, mby=0):
    """384 samples of one I_PCM macroblock.  noise; split: every border of the macroblock is one half 0 and one half 255 (which way
    round is drawn per plane), the largest "first half minus second half" a side can have, so that two sides together leave 0..255
    in both directions; flat0 / flat255; ramp: a level and slopes of at most half a level per sample, which give the small negative
    odd slopes whose >> 1 rounds down; mixed: one of these, drawn per macroblock."""
    pick = content if content != "mixed" else CONTENTS[int(rng.integers(0, len(CONTENTS)))]
    out = []
    for size in (16, 8, 8):
        yy, xx = np.mgrid[0:size, 0:size]
        if pick == "noise":
            v = rng.integers(0, 256, (size, size))
        elif pick == "split":
            v = 255 * (((xx < size // 2) == (yy < size // 2)) ^ bool(rng.integers(0, 2)))
        elif pick in ("flat0", "flat255"):
            v = np.full((size, size), 0 if pick == "flat0" else 255)
        elif pick == "ramp":
            sx, sy = rng.integers(-2, 3, 2)
            v = int(rng.integers(0, 256)) + (sx * (xx + size * mbx) + sy * (yy + size * mby)) // 4
        else:
            raise ValueError(content)
        out.append(np.clip(v, 0, 255).astype(np.uint8).ravel())
    return np.concatenate(out)


def patch_lost(wmb, hmb, decoded, ref_slot=None):
    """The macroblocks that `decoded` (one truth value per macroblock) leaves out become what conceal_one writes for them, in the
    reference's walking order (conceal_model.walk): zeroed records of kind FJ_MB_CONCEAL_I with avail = the neighbours decoded or
    concealed before them — or, with ref_slot, FJ_MB_CONCEAL_P whose four ref_slot bytes name that slot —, QP 40 / 36, filtered on
    every edge inside the picture, coef_idx = position in the walk.  (FJ_PRED_PHASE2 is the parser's business and stays clear.)
    A surviving intra macroblock no longer has a lost neighbour available, as in a stream, where a macroblock that was never
    decoded belongs to no slice: the availability bits towards lost macroblocks are cleared and a prediction mode that needs one of
    them becomes DC.  (Left set, such a macroblock would wait for the concealed one that in turn waits for it.)"""
    import conceal_model
    order = conceal_model.walk(wmb, hmb, decoded)
    lost = {mb for mb, _ in order}

    def patch(recs, mvs16, first_extra=None):
        n = wmb * hmb
        for a in range(n):
            if a in lost or recs[a, 0] not in (1, 2):
                continue
            x, y = a % wmb, a // wmb
            avail = int(recs[a, 3])
            if x > 0 and a - 1 in lost: avail &= ~1
            if y > 0 and a - wmb in lost: avail &= ~2
            if y > 0 and x + 1 < wmb and a - wmb + 1 in lost: avail &= ~4
            if y > 0 and x > 0 and a - wmb - 1 in lost: avail &= ~8
            recs[a, 3] = avail
            luma, chroma = int(recs[a, 4]) & 3, (int(recs[a, 4]) >> 2) & 3
            if chroma not in [0] + ([1] if avail & 1 else []) + ([2] if avail & 2 else []) + ([3] if (avail & 11) == 11 else []):
                chroma = 0
            if recs[a, 0] == 2:
                if luma not in [2] + ([0] if avail & 2 else []) + ([1] if avail & 1 else []) + ([3] if (avail & 11) == 11 else []):
                    luma = 2
            else:
                for z in range(16):
                    if (int(recs[a, 24 + (z >> 1)]) >> ((z & 1) * 4)) & 15 not in _i4_ok(avail, z):
                        recs[a, 24 + (z >> 1)] = (int(recs[a, 24 + (z >> 1)]) & ~(15 << ((z & 1) * 4))) | (2 << ((z & 1) * 4))
            recs[a, 4] = (int(recs[a, 4]) & 0xF0) | luma | (chroma << 2)
        for k, (a, avail) in enumerate(order):
            recs[a, :] = 0
            mvs16[a] = 0
            recs[a, 1], recs[a, 2] = 40, 36
            recs[a, 5] = 4 | (1 if a % wmb else 0) | (2 if a >= wmb else 0)
            struct.pack_into("<I", recs[a], 12, k)
            if ref_slot is None:
                recs[a, 0], recs[a, 3] = FJ_MB_CONCEAL_I, avail
            else:
                recs[a, 0] = FJ_MB_CONCEAL_P
                recs[a, 16:20] = ref_slot
    return patch


# ------------------------------------------------------------------ chosen intra macroblocks (build_job(chosen=...), border_samples)
# Random jobs draw intra macroblocks with small levels under whatever availability and modes come up.  put_chosen writes the record
# and the coefficient blocks of ONE described macroblock; border_samples gives its I_PCM neighbours the samples that the
# prediction arithmetic is sensitive to; intra_to_range scales levels against tests/intra_model.py's own residual.
BORDERS = ["noise", "ramp", "flat0", "flat255", "step_up", "step_down"]


def natural_avail(x, y, wmb):
    return (1 if x > 0 else 0) | (2 if y > 0 else 0) | (4 if y > 0 and x + 1 < wmb else 0) | (8 if x > 0 and y > 0 else 0)


def put_chosen(r, d, coefs, nblk, x, y, wmb):
    """Write the record r (coef_idx is set already) and the coefficient blocks of the macroblock that the dict d describes; returns
    (coded, nblk).  Keys: kind (1 Intra4x4, 2 Intra16x16); avail (default: what the position gives); qp_y, cqp_off (qp_c follows);
    modes (16, block order) / l16; chroma; luma {z: 16 levels, raster}; luma_dc (16 levels) with raw=True for FJ_CODED_LUMA_DC_RAW;
    chroma_dc (8 levels); chroma_ac {k: 16 levels}.  Nothing is checked here: tests/intra_model.py rejects what is not valid."""
    qp, off = int(d.get("qp_y", 26)), int(d.get("cqp_off", 0))
    r[0], r[1], r[2] = d["kind"], qp, QPC[min(51, max(0, qp + off))]
    r[20] = np.int8(off).view(np.uint8)
    r[3] = d.get("avail", natural_avail(x, y, wmb))
    r[4] = (int(d.get("l16", 0)) if d["kind"] == 2 else 0) | (int(d.get("chroma", 0)) << 2)
    r[24:32] = 0
    if d["kind"] == 1:
        for z, m in enumerate(d["modes"]): r[24 + (z >> 1)] |= m << ((z & 1) * 4)
    coded = 0

    def put(levels, bit):
        nonlocal nblk, coded
        blk = np.zeros(16, dtype=np.int16)
        blk[:len(levels)] = levels
        coefs[16 * nblk:16 * nblk + 16] = blk
        nblk += 1
        coded |= bit
    if d["kind"] == 2 and d.get("luma_dc") is not None:
        put(d["luma_dc"], (1 << 24) | ((1 << 26) if d.get("raw") else 0))
    for z in sorted(d.get("luma", {})): put(d["luma"][z], 1 << z)
    if d.get("chroma_dc") is not None: put(d["chroma_dc"], 1 << 25)
    for k in sorted(d.get("chroma_ac", {})): put(d["chroma_ac"][k], 1 << (16 + k))
    return coded, nblk


def border_samples(content, rng):
    """384 samples of an I_PCM neighbour of a chosen intra macroblock.  step_up: 255 in the lower right quadrant and 0 elsewhere, so that
    the last row and the last column are each half 0, half 255 — next to a corner macroblock of flat0 the largest H and V of plane
    prediction; step_down: its complement (next to flat255 the most negative ones); ramp: a level and slopes of up to 3 per sample"""
    out = []
    for size in (16, 8, 8):
        yy, xx = np.mgrid[0:size, 0:size]
        if content == "noise": v = rng.integers(0, 256, (size, size))
        elif content == "ramp": v = int(rng.integers(0, 256)) + int(rng.integers(-3, 4)) * (xx - size // 2) + int(rng.integers(-3, 4)) * (yy - size // 2)
        elif content == "flat0": v = np.zeros((size, size), int)
        elif content == "flat255": v = np.full((size, size), 255)
        elif content == "step_up": v = 255 * ((xx >= size // 2) & (yy >= size // 2))
        elif content == "step_down": v = 255 - 255 * ((xx >= size // 2) & (yy >= size // 2))
        else: raise ValueError(content)
        out.append(np.clip(v, 0, 255).astype(np.uint8).ravel())
    return np.concatenate(out)


def intra_to_range(levels, qp, towards, dc=None):
    """The analogue of _to_bound for intra macroblocks: the 16 levels times the largest factor (in steps of 1/16) at which
    tests/intra_model.py's own residual of the block stays inside [-512, 511] and its extreme in the direction `towards` (-1: the
    minimum, +1: the maximum) comes as close to that end as the level grid allows.  The levels come back as Python ints."""
    import intra_model
    base = [int(v) for v in levels]
    best = None
    for k in range(1, 64 * 16):
        lv = [max(-2047, min(2047, (v * k) // 16 if v >= 0 else -((-v * k) // 16))) for v in base]
        try:
            r = intra_model.residual_block(lv, qp, dc)
        except ValueError:
            break
        reach = -min(map(min, r)) if towards < 0 else max(map(max, r))
        if best is None or reach >= best[0]: best = (reach, lv)
    return best[1] if best else base


# ------------------------------------------------------------------ chosen reference pictures and chosen inter macroblocks
# Random jobs predict from noise and draw small levels.  picture_samples gives a reference picture the samples that the interpolation
# arithmetic is sensitive to (an all-I_PCM job carries them verbatim); put_inter writes ONE described inter macroblock.
PICTURES = ["flat0", "flat255", "cols+", "cols-", "rows+", "rows-", "lattice+", "lattice-", "checker", "ramp", "dark", "bright"]


def picture_samples(content, wmb, hmb, rng=None):
    """(Y[H][W], Cb, Cr) uint8, every plane of the named content.  With the signs (+, -, +) of period 3 along an axis: cols+ / rows+ are 255
    where the column's / row's sign is +, lattice+ where the signs of column and row agree; the - forms are the complements.  A row of cols+
    gives the six-tap sum 10710 at one phase in three and cols- gives -2550 there; six such rows with the signs (+, -, +, +, -, +) give the
    second-stage sums 475320 and -214200.  checker: one-sample squares of 0 and 255; ramp: 6 x + 5 y - 60 cut off at 0 and 255, so a flat
    run at either end with a slope between; dark / bright: noise in 0 .. 5 / 250 .. 255 (drawn from rng)."""
    out = []
    for w, h in ((16 * wmb, 16 * hmb), (8 * wmb, 8 * hmb), (8 * wmb, 8 * hmb)):
        yy, xx = np.mgrid[0:h, 0:w]
        sx, sy = xx % 3 != 1, yy % 3 != 1
        if content in ("flat0", "flat255"): v = np.full((h, w), 0 if content == "flat0" else 255)
        elif content[:-1] == "cols": v = 255 * (sx == (content[-1] == "+"))
        elif content[:-1] == "rows": v = 255 * (sy == (content[-1] == "+"))
        elif content[:-1] == "lattice": v = 255 * ((sx == sy) == (content[-1] == "+"))
        elif content == "checker": v = 255 * ((xx + yy) & 1)
        elif content == "ramp": v = 6 * xx + 5 * yy - 60
        elif content == "dark": v = rng.integers(0, 6, (h, w))
        elif content == "bright": v = 255 - rng.integers(0, 6, (h, w))
        else: raise ValueError(content)
        out.append(np.clip(v, 0, 255).astype(np.uint8))
    return tuple(out)


def pcm_of(picture):
    """build_job's pcm= for a whole picture (Y, Cb, Cr): {macroblock address: its 384 samples}"""
    Y, Cb, Cr = picture
    hmb, wmb = Y.shape[0] // 16, Y.shape[1] // 16
    out = {}
    for a in range(wmb * hmb):
        x, y = a % wmb, a // wmb
        out[a] = np.concatenate([P[s * y:s * y + s, s * x:s * x + s].ravel() for P, s in ((Y, 16), (Cb, 8), (Cr, 8))])
    return out


def put_inter(r, mv, d, coefs, nblk):
    """Write the record r (coef_idx is set already), the dense vectors mv[16][2] and the coefficient blocks of the inter macroblock that the
    dict d describes; returns (coded, nblk).  Keys: mv — one vector, four (one per quadrant, raster) or sixteen (raster 4x4 blocks), quarter
    samples; slots — one reference slot or four; qp_y, qp_c (both given outright: any pair); luma {z: 16 levels, raster}; chroma_dc (8
    levels: Cb, Cr); chroma_ac {k: 16 levels}.  The FJ_PARTS_* bits follow the vectors and slots.  Nothing is checked here."""
    vec = [tuple(int(c) for c in v) for v in d["mv"]]
    slots = list(d.get("slots", [0]))
    slots = slots * 4 if len(slots) == 1 else slots
    if len(vec) == 1: vec = vec * 16
    elif len(vec) == 4: vec = [vec[(k >> 3) * 2 + ((k & 3) >> 1)] for k in range(16)]
    mv[:] = vec
    quad = [(vec[(q >> 1) * 8 + (q & 1) * 2], slots[q]) for q in range(4)]
    parts = 1 if len(set(quad)) == 1 else 2 if quad[0] == quad[1] and quad[2] == quad[3] else 3 if quad[0] == quad[2] and quad[1] == quad[3] else 0
    if any(vec[k] != vec[(k >> 3) * 8 + ((k & 3) >> 1) * 2] for k in range(16)): parts = 0      # finer than quadrants: P_8x8
    r[0], r[1], r[2] = 0, int(d.get("qp_y", 26)), int(d.get("qp_c", 26))
    r[4] = parts << 4
    r[16:20] = slots
    coded = 0

    def put(levels, bit):
        nonlocal nblk, coded
        blk = np.zeros(16, dtype=np.int16)
        blk[:len(levels)] = levels
        coefs[16 * nblk:16 * nblk + 16] = blk
        nblk += 1
        coded |= bit
    for z in sorted(d.get("luma", {})): put(d["luma"][z], 1 << z)
    if d.get("chroma_dc") is not None: put(d["chroma_dc"], 1 << 25)
    for k in sorted(d.get("chroma_ac", {})): put(d["chroma_ac"][k], 1 << (16 + k))
    return coded, nblk
