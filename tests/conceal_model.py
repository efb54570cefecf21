"""Concealment of lost macroblocks as a plain integer model (test infrastructure): Python ints and numpy indexing, no C.

A third statement of the arithmetic, next to conceal_mb (h264bsd_amd/csrc/kernels/k_frame_intra.hip.h) and conceal_plane
(oracle/pixel_oracle.c), written from the reference (h264bsdConceal and ConcealMb, src/h264bsd_conceal.c:124-260 and 346-637):

  walk()     the order in which the lost macroblocks of a picture are concealed, and which neighbours each one uses
  conceal()  the samples, one plane at a time: per usable side the four sums of a quarter of its border samples, their total and
             "first half minus second half"; the hor / ver / j shifts; the two "opposite sides only" differences; the
             three-coefficient transform; clip255
  census()   which arithmetic cases a picture takes, per concealed plane — what tests/test_concealed_jobs.py holds the
             hand-built set (CONCEALED_SET) to

A picture is (Y[16 hmb, 16 wmb], Cb[8 hmb, 8 wmb], Cr[8 hmb, 8 wmb]); planes() / i420() convert from and to the I420 frame that the
oracle and the replay harness return."""
import numpy as np

LEFT, ABOVE, RIGHT, BELOW = 1, 2, 4, 8                     # FJ_CONC_* (framejob.h)
SIDES = ("ABOVE", "BELOW", "LEFT", "RIGHT")
CLASSES = (["J%d" % j for j in (1, 2, 3, 4)] + ["HOR%d" % k for k in (0, 1, 2)] + ["VER%d" % k for k in (0, 1, 2)] +
           ["LR_ONLY", "AB_ONLY", "FLAT", "T1_NEG_ODD", "V_NEG_ODD", "CLIP_LOW", "CLIP_HIGH", "SATURATED_SIDE"] +
           ["SATURATED_" + s for s in SIDES])


def planes(frame, wmb, hmb):
    """the three planes of an I420 frame, as int arrays of their own"""
    W, H = 16 * wmb, 16 * hmb
    f = np.asarray(frame)
    return [f[:W * H].reshape(H, W).astype(np.int64), f[W * H:W * H + W * H // 4].reshape(H // 2, W // 2).astype(np.int64),
            f[W * H + W * H // 4:W * H + W * H // 2].reshape(H // 2, W // 2).astype(np.int64)]


def i420(picture):
    return np.concatenate([np.asarray(p).astype(np.uint8).reshape(-1) for p in picture])


def walk(wmb, hmb, decoded):
    """[(mb, avail)] in the reference's order: the row of the first decoded macroblock leftwards from it, then rightwards; the rows
    above it column by column, upwards; the rows below in raster order.  A concealed macroblock counts as decoded for those after
    it.  decoded: one truth value per macroblock, at least one of them true (a wholly lost picture is not concealed this way)."""
    dec = [bool(d) for d in decoded]
    assert len(dec) == wmb * hmb and any(dec)
    first = dec.index(True)
    row, col = divmod(first, wmb)
    order = []

    def one(y, x):
        a = y * wmb + x
        avail = 0
        if y and dec[a - wmb]: avail |= ABOVE
        if y != hmb - 1 and dec[a + wmb]: avail |= BELOW
        if x and dec[a - 1]: avail |= LEFT
        if x != wmb - 1 and dec[a + 1]: avail |= RIGHT
        order.append((a, avail))
        dec[a] = True

    for x in range(col - 1, -1, -1): one(row, x)
    for x in range(col + 1, wmb):
        if not dec[row * wmb + x]: one(row, x)
    for x in range(wmb):
        for y in range(row - 1, -1, -1): one(y, x)
    for y in range(row + 1, hmb):
        for x in range(wmb):
            if not dec[y * wmb + x]: one(y, x)
    return order


def position(wmb, hmb, mb, avail):
    """(avail, first column, last column, first row, last row): what decides which neighbours a concealed macroblock can have"""
    x, y = mb % wmb, mb // wmb
    return (avail, x == 0, x == wmb - 1, y == 0, y == hmb - 1)


def _transform(t0, t1, v):
    """Transform() of the reference on data[0] = t0, data[1] = t1, data[4] = v and zeros elsewhere: 16 values, raster"""
    if not t1 and not v:
        return [t0] * 16
    d = [0] * 16
    d[0], d[1], d[2], d[3] = t0 + t1, t0 + (t1 >> 1), t0 - (t1 >> 1), t0 - t1
    d[4] = d[5] = d[6] = d[7] = v
    for c in range(4):
        a, b = d[c], d[4 + c]
        d[c], d[4 + c], d[8 + c], d[12 + c] = a + b, a + (b >> 1), a - (b >> 1), a - b
    return d


def conceal_plane(P, size, x, y, avail, seen=None):
    """conceal macroblock (x, y) of plane P (size 16: luma, 8: chroma) in place from the sides in avail; seen: a set that receives
    the census classes the plane takes"""
    q, x0, y0 = size // 4, size * x, size * y
    sh = 0 if size == 16 else 1                              # every shift of chroma is one less: half as many samples per side
    quarter_sums = {}
    if avail & ABOVE: quarter_sums["ABOVE"] = [int(P[y0 - 1, x0 + q * k:x0 + q * k + q].sum()) for k in range(4)]
    if avail & BELOW: quarter_sums["BELOW"] = [int(P[y0 + size, x0 + q * k:x0 + q * k + q].sum()) for k in range(4)]
    if avail & LEFT: quarter_sums["LEFT"] = [int(P[y0 + q * k:y0 + q * k + q, x0 - 1].sum()) for k in range(4)]
    if avail & RIGHT: quarter_sums["RIGHT"] = [int(P[y0 + q * k:y0 + q * k + q, x0 + size].sum()) for k in range(4)]
    total = {s: sum(v) for s, v in quarter_sums.items()}
    half = {s: v[0] + v[1] - v[2] - v[3] for s, v in quarter_sums.items()}
    A, B, L, R = ("ABOVE" in total), ("BELOW" in total), ("LEFT" in total), ("RIGHT" in total)
    hor, ver = A + B, L + R
    j = hor + ver
    assert j
    t0 = sum(total.values())
    t1 = sum(half[s] for s in ("ABOVE", "BELOW") if s in half)
    v = sum(half[s] for s in ("LEFT", "RIGHT") if s in half)
    if not hor and L and R: t1 = (total["LEFT"] - total["RIGHT"]) >> (5 - sh)
    elif hor: t1 >>= 3 - sh + hor
    if not ver and A and B: v = (total["ABOVE"] - total["BELOW"]) >> (5 - sh)
    elif ver: v >>= 3 - sh + ver
    if j == 1: t0 >>= 4 - sh
    elif j == 2: t0 >>= 5 - sh
    elif j == 3: t0 = (21 * t0) >> (10 - sh)
    else: t0 >>= 6 - sh
    values = _transform(t0, t1, v)
    for by in range(4):
        for bx in range(4):
            P[y0 + q * by:y0 + q * by + q, x0 + q * bx:x0 + q * bx + q] = min(255, max(0, values[4 * by + bx]))
    if seen is not None:
        seen |= {"J%d" % j, "HOR%d" % hor, "VER%d" % ver}
        if not hor and L and R: seen.add("LR_ONLY")
        if not ver and A and B: seen.add("AB_ONLY")
        if not t1 and not v: seen.add("FLAT")
        if t1 < 0 and t1 & 1: seen.add("T1_NEG_ODD")
        if v < 0 and v & 1: seen.add("V_NEG_ODD")
        if min(values) < 0: seen.add("CLIP_LOW")
        if max(values) > 255: seen.add("CLIP_HIGH")
        for s, d in half.items():
            if abs(d) == 255 * size // 2: seen |= {"SATURATED_SIDE", "SATURATED_" + s}


def conceal(picture, wmb, hmb, order, counts=None):
    """conceal the macroblocks of order = [(mb, avail)] (walk()) in `picture` = [Y, Cb, Cr], in place.  counts: {"luma": {class:
    planes}, "chroma": {...}} to add this picture's census to."""
    for mb, avail in order:
        x, y = mb % wmb, mb // wmb
        for k, P in enumerate(picture):
            seen = set() if counts is not None else None
            conceal_plane(P, 8 if k else 16, x, y, avail, seen)
            if counts is not None:
                c = counts["chroma" if k else "luma"]
                for name in seen: c[name] = c.get(name, 0) + 1
    return picture


def copy_lost(picture, reference, wmb, order):
    """the concealment of a P picture: every lost macroblock is the co-located one of the reference picture"""
    for mb, _avail in order:
        x, y = mb % wmb, mb // wmb
        for k, (P, Q) in enumerate(zip(picture, reference)):
            s = 8 if k else 16
            P[s * y:s * y + s, s * x:s * x + s] = Q[s * y:s * y + s, s * x:s * x + s]
    return picture


def census(picture, wmb, hmb, order):
    """{"luma": {class: planes}, "chroma": {class: planes}} of concealing `order` in a COPY of `picture`, every class of CLASSES present"""
    counts = {"luma": dict.fromkeys(CLASSES, 0), "chroma": dict.fromkeys(CLASSES, 0)}
    conceal([np.array(p, dtype=np.int64) for p in picture], wmb, hmb, order, counts)
    return counts
