"""Model of h264bsdmiOutputPointModel (include/h264bsd_mi355x.h): the record of one region, byte for byte, in two forms.

mrec, krec, crec: the bytes of one record of h264bsdmiOutputPointMatches and of two of h264bsdmiOutputCornerPoints at max_points == K,
whatever they hold.  record() IS the definition, written straight from it in Python integers, which are unbounded: a 64-bit overflow in
the kernel shows.  record_fast() is the same quantity in numpy int64 (every magnitude stays below 2^61, the header's bound), vectorised
over hypotheses in chunks; it is compared only against record() (tests/test_point_model_cpu.py) and exists so that the K = 256 cases
stay in seconds.  inputs() builds the three records by hand from a list of pairs."""
import struct

import numpy as np

import matches_model as mm

TRANSLATION, SIMILARITY = 0, 1
USABLE, INLIER = 1, 2
COORD_MAX = 16383
SUMS = 12


def record_bytes(max_points):
    return 128 + 4 * max_points


def usable_pairs(mrec, krec, crec, K):
    """[(slot i, xk, yk, xc, yc)] of the usable pairs, in slot order"""
    nk, nc = min(struct.unpack_from("<I", krec, 8)[0], K), min(struct.unpack_from("<I", crec, 8)[0], K)
    out = []
    for i in range(K):
        j, _, _, flags = struct.unpack_from("<iIII", mrec, 32 + 16 * i)
        if not flags & mm.ACCEPTED or not 0 <= j < K or i >= nk or j >= nc:
            continue
        p = struct.unpack_from("<ii", krec, 32 + 16 * i) + struct.unpack_from("<ii", crec, 32 + 16 * j)
        if all(0 <= v <= COORD_MAX for v in p):
            out.append((i,) + p)
    return out


def _inlier_similarity(A, B, V, tolerance):
    Px, Py, Qx, Qy = B[1] - A[1], B[2] - A[2], B[3] - A[3], B[4] - A[4]
    dpx, dpy, dqx, dqy = V[1] - A[1], V[2] - A[2], V[3] - A[3], V[4] - A[4]
    re = (dqx * Px - dqy * Py) - (Qx * dpx - Qy * dpy)
    im = (dqx * Py + dqy * Px) - (Qx * dpy + Qy * dpx)
    return re * re + im * im <= tolerance * tolerance * (Px * Px + Py * Py)


def _inlier_translation(A, V, tolerance):
    dx, dy = (V[3] - V[1]) - (A[3] - A[1]), (V[4] - V[2]) - (A[4] - A[2])
    return dx * dx + dy * dy <= tolerance * tolerance


def _gated(A, B, max_scale):
    """the pair a < b is a hypothesis"""
    PP, QQ = (B[1] - A[1]) ** 2 + (B[2] - A[2]) ** 2, (B[3] - A[3]) ** 2 + (B[4] - A[4]) ** 2
    if PP == 0 or QQ == 0:
        return False
    return not max_scale or (65536 * QQ <= max_scale ** 2 * PP and 65536 * PP <= max_scale ** 2 * QQ)


def best(pairs, model, tolerance, max_scale):
    """(hypotheses, count, a, b) with a, b indices into pairs (b None for a translation); count 0 and a None without a hypothesis"""
    n, hyp, top = len(pairs), 0, (0, None, None)
    if model == TRANSLATION:
        for a in range(n):
            hyp += 1
            c = sum(_inlier_translation(pairs[a], v, tolerance) for v in pairs)
            if c > top[0]:
                top = (c, a, None)
    else:
        for a in range(n):
            for b in range(a + 1, n):
                if not _gated(pairs[a], pairs[b], max_scale):
                    continue
                hyp += 1
                c = sum(_inlier_similarity(pairs[a], pairs[b], v, tolerance) for v in pairs)
                if c > top[0]:
                    top = (c, a, b)
    return (hyp,) + top


def best_fast(pairs, model, tolerance, max_scale, chunk=2048):
    """best() in numpy int64"""
    n = len(pairs)
    if n == 0:
        return 0, 0, None, None
    P = np.array([p[1:] for p in pairs], np.int64)                          # [n, 4]: xk, yk, xc, yc
    if model == TRANSLATION:
        d = P[:, 2:] - P[:, :2]
        e = d[None, :, :] - d[:, None, :]
        counts = ((e * e).sum(axis=2) <= tolerance * tolerance).sum(axis=1)
        a = int(np.argmax(counts))                                          # the first maximum: the smallest a
        return n, int(counts[a]), a, None
    ia, ib = np.triu_indices(n, 1)                                          # a ascending, then b: the first maximum is the smallest (a, b)
    if len(ia) == 0:
        return 0, 0, None, None
    A, B = P[ia], P[ib]
    Pv, Qv = B[:, :2] - A[:, :2], B[:, 2:] - A[:, 2:]
    PP, QQ = (Pv * Pv).sum(axis=1), (Qv * Qv).sum(axis=1)
    ok = (PP > 0) & (QQ > 0)
    if max_scale:
        ok &= (65536 * QQ <= max_scale * max_scale * PP) & (65536 * PP <= max_scale * max_scale * QQ)
    counts = np.full(len(ia), -1, np.int64)
    for h0 in range(0, len(ia), chunk):
        s = slice(h0, h0 + chunk)
        dp = P[None, :, :2] - A[s, None, :2]                                # [h, n, 2]
        dq = P[None, :, 2:] - A[s, None, 2:]
        px, py, qx, qy = Pv[s, None, 0], Pv[s, None, 1], Qv[s, None, 0], Qv[s, None, 1]
        re = (dq[..., 0] * px - dq[..., 1] * py) - (qx * dp[..., 0] - qy * dp[..., 1])
        im = (dq[..., 0] * py + dq[..., 1] * px) - (qx * dp[..., 1] + qy * dp[..., 0])
        c = (re * re + im * im <= tolerance * tolerance * PP[s, None]).sum(axis=1)
        counts[s] = np.where(ok[s], c, -1)
    hyp = int(ok.sum())
    if hyp == 0:
        return 0, 0, None, None
    h = int(np.argmax(counts))
    return hyp, int(counts[h]), int(ia[h]), int(ib[h])


def _record(mrec, krec, crec, K, model, tolerance, max_scale, min_inliers, best_of):
    pairs = usable_pairs(mrec, krec, crec, K)
    hyp, count, a, b = best_of(pairs, model, tolerance, max_scale)
    found = a is not None and count >= min_inliers
    flags, sums = [0] * K, [0] * SUMS
    for p in pairs:
        flags[p[0]] = USABLE
    if found:
        for v in pairs:
            if _inlier_translation(pairs[a], v, tolerance) if model == TRANSLATION else _inlier_similarity(pairs[a], pairs[b], v, tolerance):
                flags[v[0]] |= INLIER
                _, x, y, u, w = v
                for k, t in enumerate((x, y, u, w, x * x, x * y, y * y, x * u, y * u, x * w, y * w, u * u + w * w)):
                    sums[k] += t
        assert sum(1 for f in flags if f & INLIER) == count
    head = struct.pack("<IIIIiiII", len(pairs), hyp, count if found else 0, 1 if found else 0, pairs[a][0] if found else -1,
                       pairs[b][0] if found and model == SIMILARITY else -1, 0, 0)
    return head + struct.pack("<12q", *sums) + struct.pack(f"<{K}I", *flags)


def record(mrec, krec, crec, K, model=SIMILARITY, tolerance=2, max_scale=0, min_inliers=None):
    """the definition, in Python integers"""
    return _record(mrec, krec, crec, K, model, tolerance, max_scale, 1 + model if min_inliers is None else min_inliers, best)


def record_fast(mrec, krec, crec, K, model=SIMILARITY, tolerance=2, max_scale=0, min_inliers=None):
    return _record(mrec, krec, crec, K, model, tolerance, max_scale, 1 + model if min_inliers is None else min_inliers, best_fast)


class Record:
    """the fields of one record"""

    def __init__(self, rec, K):
        assert len(rec) == record_bytes(K)
        self.usable, self.hypotheses, self.inliers, self.found, self.a, self.b, z0, z1 = struct.unpack_from("<IIIIiiII", rec, 0)
        self.zero = (z0, z1)
        self.sums = list(struct.unpack_from("<12q", rec, 32))
        self.flags = list(struct.unpack_from(f"<{K}I", rec, 128))

    def head(self):
        return self.usable, self.hypotheses, self.inliers, self.found, self.a, self.b, self.zero


def inputs(K, pairs, j=None, flags=None, kept_written=None, current_written=None):
    """the three records by hand: pairs[i] = ((xk, yk), (xc, yc)) is kept slot i matched to current slot j[i] (default: a fixed
    permutation of the slots in use, so that a kernel that read current slot i would show); flags[i]: the matches slot's flags (default
    VALID | MUTUAL | ACCEPTED); the slots behind the pairs are unmatched (-1, 257, 257, 0) and their points zero.  Returns (mrec, krec,
    crec)"""
    n = len(pairs)
    assert n <= K
    if j is None:
        step = next(s for s in (7, 5, 3, 1) if n % s or s == 1)
        j = [(i * step + 3) % n for i in range(n)]                          # a permutation: step and n are coprime
        assert sorted(j) == list(range(n))
    if flags is None:
        flags = [mm.VALID | mm.MUTUAL | mm.ACCEPTED] * n
    current = [(0, 0)] * K
    for i in range(n):
        if 0 <= j[i] < K:
            current[j[i]] = pairs[i][1]
    mrec = struct.pack("<IIIIiiII", n, n, n, n, 0, 0, 0, 0)
    mrec += b"".join(struct.pack("<iIII", j[i] if -2 ** 31 <= j[i] < 2 ** 31 else j[i] - 2 ** 32, 0, 257, flags[i]) for i in range(n))
    mrec += struct.pack("<iIII", -1, 257, 257, 0) * (K - n) + bytes(64 * K)
    krec = mm.points_record([p[0] for p in pairs], K, written=n if kept_written is None else kept_written)
    used = max([jj + 1 for jj in j if 0 <= jj < K], default=0)
    crec = mm.points_record(current[:used], K, written=used if current_written is None else current_written)
    return mrec, krec, crec
