"""numpy model of h264bsdmiOutputPointMatches (include/h264bsd_mi355x.h): the record of one region, byte for byte, in two forms.

kept, cur: [H, W] uint8 luma planes of two coded frames; window (x0, y0, w, h) in the coded frame; box (x, y, w, h) relative to the
window; kpts, cpts: the bytes of two point records of h264bsdmiOutputCornerPoints at max_points == K (whatever they hold).
record() IS the definition, written straight from it: per point and per test two sums of 25 samples of the clamped luma, and best,
second and mutual by brute force over the pairs.  record_fast() is the same quantity computed the other way round — one box-sum image
of the window padded by 14 in edge mode, every descriptor from two gathers, a vectorised xor-popcount matrix and argmins; it is compared
only against record() (tests/test_point_matches_cpu.py) and exists so that the larger GPU cases stay in seconds."""
import struct

import numpy as np

VALID, MUTUAL, ACCEPTED = 1, 2, 4
NONE = 257
REACH, HALO = 12, 14


def generate_pattern():
    """the 256 tests (px, py, qx, qy) from the generator of the header, and how many draws were dropped on the way"""
    s = 0x9E3779B9

    def draw():
        nonlocal s
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        return s

    def coordinate():
        a = (draw() >> 8) % 13 - 6
        return a + (draw() >> 8) % 13 - 6

    tests, seen, dropped = [], set(), 0
    while len(tests) < 256:
        t = (coordinate(), coordinate(), coordinate(), coordinate())
        if t[:2] == t[2:] or t in seen or t[2:] + t[:2] in seen:
            dropped += 1
            continue
        seen.add(t)
        tests.append(t)
    return tests, dropped


PATTERN = np.array(generate_pattern()[0], np.int64)


def record_bytes(max_points):
    return 32 + 80 * max_points


def points_record(points, K, written=None, count=0, found=0):
    """a point record by hand: the slots hold `points` ((x, y) or (x, y, score)), zeros behind them; written as given (default: their number)"""
    pts = [tuple(p) + (0,) * (3 - len(p)) for p in points]
    assert len(pts) <= K
    out = struct.pack("<IIIIQQ", count, found, len(pts) if written is None else written, 0, 0, 0)
    out += b"".join(struct.pack("<iiq", *p) for p in pts)
    return out + bytes(16 * (K - len(pts)))


def slots(rec, K, window, box):
    """[(x, y, valid)] of the K slots of a point record: valid iff i < min(written, K) and (x, y) in T"""
    _, _, ww, wh = window
    x, y, w, h = box
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, ww), min(y + h, wh)
    written = min(struct.unpack_from("<I", rec, 8)[0], K)
    out = []
    for i in range(K):
        px, py = struct.unpack_from("<ii", rec, 32 + 16 * i)
        out.append((px, py, i < written and x0 <= px < x1 and y0 <= py < y1))
    return out


def _window(frame, window):
    x0, y0, w, h = window
    return np.asarray(frame)[y0:y0 + h, x0:x0 + w].astype(np.int64)


def smoothed(win, u, v):
    """B(u, v): the sum of the 25 samples of the replicated luma around (u, v)"""
    H, W = win.shape
    return int(sum(win[min(max(v + dv, 0), H - 1), min(max(u + du, 0), W - 1)] for dv in range(-2, 3) for du in range(-2, 3)))


def descriptor(win, x, y):
    """the 32 bytes of the descriptor of (x, y), test by test"""
    out = bytearray(32)
    for t, (px, py, qx, qy) in enumerate(PATTERN.tolist()):
        if smoothed(win, x + px, y + py) < smoothed(win, x + qx, y + qy):
            out[t // 8] |= 1 << (t % 8)
    return bytes(out)


def _pack(K, ks, cs, dk, dc, slots4):
    """the record from its parts: the header is counted from the slots"""
    acc = [i for i in range(K) if slots4[i][3] & ACCEPTED]
    head = (sum(1 for s in ks if s[2]), sum(1 for s in cs if s[2]), len(acc), sum(1 for s in slots4 if s[3] & MUTUAL),
            sum(cs[slots4[i][0]][0] - ks[i][0] for i in acc), sum(cs[slots4[i][0]][1] - ks[i][1] for i in acc))
    out = struct.pack("<IIIIiiII", *head, 0, 0)
    out += b"".join(struct.pack("<iIII", *s) for s in slots4)
    return out + b"".join(dk) + b"".join(dc)


def _accept(best, second, mutual, max_distance, ratio, mutual_only):
    return best <= max_distance and (ratio == 256 or best * 256 < ratio * second) and (not mutual_only or mutual)


def record(kept, cur, window, box, kpts, cpts, K, max_distance=64, ratio=205, max_move=0, mutual_only=1):
    wk, wc = _window(kept, window), _window(cur, window)
    ks, cs = slots(kpts, K, window, box), slots(cpts, K, window, box)
    dk = [descriptor(wk, x, y) if ok else bytes(32) for x, y, ok in ks]
    dc = [descriptor(wc, x, y) if ok else bytes(32) for x, y, ok in cs]
    ik, ic = [int.from_bytes(d, "little") for d in dk], [int.from_bytes(d, "little") for d in dc]

    def candidate(i, j):
        return ks[i][2] and cs[j][2] and (max_move == 0 or max(abs(ks[i][0] - cs[j][0]), abs(ks[i][1] - cs[j][1])) <= max_move)

    def d(i, j):
        return bin(ik[i] ^ ic[j]).count("1")

    out = []
    for i in range(K):
        cand = sorted((d(i, j), j) for j in range(K) if candidate(i, j))
        if not ks[i][2] or not cand:
            out.append((-1, NONE, NONE, VALID if ks[i][2] else 0))
            continue
        best, j = cand[0]
        second = cand[1][0] if len(cand) > 1 else NONE
        mutual = min((d(i2, j), i2) for i2 in range(K) if candidate(i2, j))[1] == i
        flags = VALID | (MUTUAL if mutual else 0) | (ACCEPTED if _accept(best, second, mutual, max_distance, ratio, mutual_only) else 0)
        out.append((j, best, second, flags))
    return _pack(K, ks, cs, dk, dc, out)


POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def box_sums(win):
    """B(u, v) for u in -12 .. W + 11, v in -12 .. H + 11 at [v + 12, u + 12]: one image of the window padded by 14 in edge mode"""
    p = np.pad(win, HALO, mode="edge")
    c = np.pad(p.cumsum(axis=0).cumsum(axis=1), ((1, 0), (1, 0)))
    return c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]


def descriptors_fast(B, sl):
    """[K, 32] uint8: the descriptors of the valid slots, zeros for the others"""
    out = np.zeros((len(sl), 32), np.uint8)
    ok = np.array([s[2] for s in sl], bool)
    if ok.any():
        x = np.array([s[0] for s in sl], np.int64)[ok, None] + REACH
        y = np.array([s[1] for s in sl], np.int64)[ok, None] + REACH
        bits = B[y + PATTERN[None, :, 1], x + PATTERN[None, :, 0]] < B[y + PATTERN[None, :, 3], x + PATTERN[None, :, 2]]
        out[ok] = np.packbits(bits, axis=1, bitorder="little")
    return out


def record_fast(kept, cur, window, box, kpts, cpts, K, max_distance=64, ratio=205, max_move=0, mutual_only=1):
    ks, cs = slots(kpts, K, window, box), slots(cpts, K, window, box)
    dk, dc = descriptors_fast(box_sums(_window(kept, window)), ks), descriptors_fast(box_sums(_window(cur, window)), cs)
    BIG = 1 << 20
    D = POPCOUNT[dk[:, None, :] ^ dc[None, :, :]].sum(axis=2)
    vk, vc = np.array([s[2] for s in ks], bool), np.array([s[2] for s in cs], bool)
    cand = vk[:, None] & vc[None, :]
    if max_move:
        # invalid slots may hold anything: their coordinates are not looked at
        xk, yk = (np.array([s[a] if s[2] else 0 for s in ks], np.int64) for a in (0, 1))
        xc, yc = (np.array([s[a] if s[2] else 0 for s in cs], np.int64) for a in (0, 1))
        cand &= np.maximum(np.abs(xk[:, None] - xc[None, :]), np.abs(yk[:, None] - yc[None, :])) <= max_move
    D = np.where(cand, D, BIG)
    bj = D.argmin(axis=1)                                  # the first of the smallest: the smallest j
    best = D[np.arange(K), bj]
    rest = D.copy()
    rest[np.arange(K), bj] = BIG
    second = rest.min(axis=1)
    col = D.argmin(axis=0)                                 # per current slot the smallest (d, i)
    out = []
    for i in range(K):
        if best[i] >= BIG:
            out.append((-1, NONE, NONE, VALID if ks[i][2] else 0))
            continue
        j, b, s = int(bj[i]), int(best[i]), int(second[i]) if second[i] < BIG else NONE
        mutual = int(col[j]) == i
        out.append((j, b, s, VALID | (MUTUAL if mutual else 0) | (ACCEPTED if _accept(b, s, mutual, max_distance, ratio, mutual_only) else 0)))
    return _pack(K, ks, cs, [bytes(r) for r in dk], [bytes(r) for r in dc], out)


class Record:
    """the fields of a record's bytes"""

    def __init__(self, rec, K):
        assert len(rec) == record_bytes(K)
        self.kept_valid, self.current_valid, self.accepted, self.mutual, self.sum_dx, self.sum_dy, z0, z1 = struct.unpack_from("<IIIIiiII", rec, 0)
        assert z0 == 0 and z1 == 0
        self.slots = [struct.unpack_from("<iIII", rec, 32 + 16 * i) for i in range(K)]
        self.kept_descriptors = np.frombuffer(rec, np.uint8, 32 * K, 32 + 16 * K).reshape(K, 32)
        self.current_descriptors = np.frombuffer(rec, np.uint8, 32 * K, 32 + 48 * K).reshape(K, 32)
