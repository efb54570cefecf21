"""The hand-built cases of h264bsdmiOutputPointModel, shared by tests/test_point_model_cpu.py (the two forms of the model equal on each)
and tests/test_gpu_point_model.py (the device equal to the model on each): cases() gives a list of Case(name, K, kw, mrec, krec, crec),
kw the model's keywords (model, tolerance, max_scale, min_inliers).  All motions are exact in integers."""
import collections
import struct

import numpy as np

import matches_model as mm
import model_fit_model as fm

Case = collections.namedtuple("Case", "name K kw mrec krec crec")
T, S = fm.TRANSLATION, fm.SIMILARITY
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = [1, 2, 3, 63, 64, 65, 255, 256]

MOTIONS = {                                                     # kept (x, y) -> current, exact; the points are even and in 200 .. 3000
    "translation": lambda x, y: (x + 40, y + 25),
    "rot90": lambda x, y: (5000 - y, x + 100),
    "rot180": lambda x, y: (6000 - x, 7000 - y),
    "scale2": lambda x, y: (2 * x + 10, 2 * y + 20),
    "half": lambda x, y: (x // 2 + 30, y // 2 + 40),
    "other": lambda x, y: (x + 300, y - 150),
}


def scatter(rng, n, lo=200, hi=3000):
    """n distinct even points"""
    pts = set()
    while len(pts) < n:
        pts.add((2 * int(rng.integers(lo // 2, hi // 2)), 2 * int(rng.integers(lo // 2, hi // 2))))
    return sorted(pts, key=lambda p: (p[0] * 7919 + p[1] * 104729) % 10007)


def moved(points, motion):
    return [(p, MOTIONS[motion](*p)) for p in points]


def noise(rng, points):
    return [(p, (int(rng.integers(0, 6000)), int(rng.integers(0, 6000)))) for p in points]


def interleave(a, b):
    out = []
    for i in range(max(len(a), len(b))):
        out += a[i:i + 1] + b[i:i + 1]
    return out


def cases():
    rng = np.random.default_rng(20)
    out = []

    def add(name, K, pairs, kw, **inputs_kw):
        out.append(Case(name, K, kw, *fm.inputs(K, pairs, **inputs_kw)))

    # every size at which the kernel takes another path: one thread, a wavefront and its neighbours, all four and one short of it
    for K in SIZES:
        pts = scatter(rng, K)
        m = (3 * K + 4) // 5
        add(f"full_translation_K{K}", K, interleave(moved(pts[:m], "translation"), noise(rng, pts[m:])), dict(model=T, tolerance=2))
        add(f"full_similarity_K{K}", K, interleave(moved(pts[:m], "rot90"), noise(rng, pts[m:])), dict(model=S, tolerance=2))
    # 0, 1 and 2 usable pairs
    pts = scatter(rng, 12)
    for n in (0, 1, 2):
        for model in (T, S):
            add(f"usable_{n}_model{model}", 8, moved(pts[:n], "scale2"), dict(model=model, tolerance=1))
    # no hypothesis: all kept points equal, all current points equal
    add("kept_equal_similarity", 8, [((500, 600), q) for q in pts[:5]], dict(model=S, tolerance=3))
    add("kept_equal_translation", 8, [((500, 600), q) for q in pts[:5]], dict(model=T, tolerance=3))
    add("current_equal_similarity", 8, [(p, (500, 600)) for p in pts[:5]], dict(model=S, tolerance=3))
    add("current_equal_translation", 8, [(p, (500, 600)) for p in pts[:5]], dict(model=T, tolerance=3))
    # an exact motion and a second, consistent one beside it: smaller, equal (the tie goes to the smaller (a, b)), larger; either order
    for motion in ("rot90", "rot180", "scale2", "half", "translation"):
        for n1, n2 in ((6, 4), (5, 5), (4, 6)):
            pts = scatter(rng, n1 + n2)
            first, second = moved(pts[:n1], motion), moved(pts[n1:], "other")
            model = T if motion == "translation" else S
            for tol in (0, 2):
                add(f"two_motions_{motion}_{n1}_{n2}_tol{tol}", 16, interleave(first, second), dict(model=model, tolerance=tol))
            add(f"two_motions_{motion}_{n1}_{n2}_swapped", 16, interleave(second, first), dict(model=model, tolerance=1))
    # residuals exactly on the inlier boundary and one step beyond, on a basis pair that is not axis-aligned (|P| = 5 and 13)
    for (dx, dy), (ox, oy), tol in (((3, 4), (4, 4), 5), ((5, 12), (6, 12), 13), ((4, 3), (3, 5), 5), ((12, 5), (12, 6), 13)):
        base = [(100, 100), (103, 104), (105, 112), (220, 330), (400, 180)]
        for motion in ("rot90", "rot180", "scale2", "translation"):
            exact = moved(base, motion)
            on = [((300 + 10 * k, 500 + 7 * k), (q[0] + sx * dx, q[1] + sy * dy))
                  for k, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))) for q in [MOTIONS[motion](300 + 10 * k, 500 + 7 * k)]]
            beyond = [((700 + 10 * k, 200 + 7 * k), (q[0] + sx * ox, q[1] + sy * oy))
                      for k, (sx, sy) in enumerate(((1, 1), (-1, -1))) for q in [MOTIONS[motion](700 + 10 * k, 200 + 7 * k)]]
            model = T if motion == "translation" else S
            # the definition measures the residual in current samples, whatever the scale: the offsets hold for every motion
            add(f"boundary_{motion}_{dx}_{dy}_tol{tol}", 16, exact + on + beyond, dict(model=model, tolerance=tol))
    # the scale gate exactly at S and one step beyond, both directions
    for Sc, P, Q, name in ((512, (10, 0), (20, 0), "at"), (512, (10, 0), (21, 0), "beyond"), (512, (20, 0), (10, 0), "inverse_at"),
                           (512, (21, 0), (10, 0), "inverse_beyond"), (300, (256, 0), (300, 0), "at"), (300, (256, 0), (301, 0), "beyond"),
                           (300, (0, 300), (256, 0), "inverse_at"), (300, (0, 301), (256, 0), "inverse_beyond"),
                           (256, (3, 4), (5, 0), "at"), (256, (3, 4), (5, 1), "beyond"), (4096, (1, 0), (16, 0), "at"), (4096, (1, 0), (0, 17), "beyond"),
                           (4096, (16383, 16383), (1024, 1024), "inverse_near"),
                           (4096, (16383, 16383), (1023, 1023), "inverse_beyond")):
        (px, py), (qx, qy) = ((0, 0), (0, 0)) if max(P) == fm.COORD_MAX else ((50, 60), (700, 800))
        pairs = [((px, py), (qx, qy)), ((px + P[0], py + P[1]), (qx + Q[0], qy + Q[1]))]
        add(f"scale_gate_{Sc}_{name}_{P}_{Q}", 4, pairs, dict(model=S, tolerance=0, max_scale=Sc))
    pts = scatter(rng, 20)
    add("scale_gate_among_many", 32, interleave(moved(pts[:12], "scale2"), moved(pts[12:], "other")), dict(model=S, tolerance=1, max_scale=400))
    # the largest 64-bit magnitudes: coordinates at 0 and 16383 with tolerance 255
    M = fm.COORD_MAX
    corners = [(0, 0), (M, M), (0, M), (M, 0)]
    flipped = [(c, (M - c[0], M - c[1])) for c in corners]
    far = [((0, 0), (0, 0)), ((M, M), (M, M)), ((0, M), (M, M)), ((M, 0), (0, 0)), ((1, 0), (M, M - 255)), ((M - 1, M), (0, 255)), ((8000, 8000), (8383, 8000))]
    for model in (T, S):
        add(f"extremes_model{model}", 16, flipped + far, dict(model=model, tolerance=255))
        add(f"extremes_identity_model{model}", 16, [(c, c) for c in corners] + far, dict(model=model, tolerance=255))
    add("sums_256_at_16383_translation", 256, [((M, M), (M, M))] * 256, dict(model=T, tolerance=0))
    near = [(M - i % 16, M - i // 16) for i in range(256)]
    add("sums_256_near_16383_similarity", 256, [(p, p) for p in near], dict(model=S, tolerance=0))
    # unusable inputs among good ones: coordinates, j, flags, written
    pts = scatter(rng, 16)
    good = moved(pts, "rot90")
    for bad in (-1, 16384, INT_MIN, INT_MAX):
        pairs = list(good)
        for k in range(4):                                                  # each of the four coordinates in a slot of its own
            p = list(pairs[2 + 3 * k][0] + pairs[2 + 3 * k][1])
            p[k] = bad
            pairs[2 + 3 * k] = ((p[0], p[1]), (p[2], p[3]))
        for model in (T, S):
            add(f"coordinate_{bad}_model{model}", 16, pairs, dict(model=model, tolerance=2))
    for K in (16, 20):
        n = 16
        j = [(5 * i + 3) % n for i in range(n)]
        for slot, bad in ((1, -1), (4, K), (9, INT_MAX), (12, INT_MIN), (14, K + 1), (6, 18)):      # 18: a slot at K = 20, behind `written`
            j[slot] = bad
        add(f"bad_j_K{K}", K, good, dict(model=S, tolerance=2), j=j, current_written=16)
    flags = [mm.VALID | mm.MUTUAL | mm.ACCEPTED] * 16
    for slot, f in ((0, 0), (3, mm.VALID | mm.MUTUAL), (7, 0xFFFFFFFB), (8, 0xFFFFFFFF), (11, mm.ACCEPTED)):
        flags[slot] = f
    add("flags", 16, good, dict(model=S, tolerance=2), flags=flags)
    for kw_, cw in ((0, None), (None, 0), (0xFFFFFFFF, 0xFFFFFFFF), (9, None), (None, 9), (17, 2 ** 31)):
        for K in (16, 24):
            add(f"written_{kw_}_{cw}_K{K}", K, good, dict(model=S, tolerance=2), kept_written=kw_, current_written=cw)
    # random bytes as all three inputs; and random records whose j and flags are in range, so that the coordinates are reached
    for K in (7, 64, 256):
        mrec, krec, crec = rng.bytes(mm.record_bytes(K)), rng.bytes(32 + 16 * K), rng.bytes(32 + 16 * K)
        for model in (T, S):
            out.append(Case(f"random_bytes_K{K}_model{model}", K, dict(model=model, tolerance=255), mrec, krec, crec))
        m2 = bytearray(mrec)
        for i in range(K):
            struct.pack_into("<iIII", m2, 32 + 16 * i, int(rng.integers(0, K)), 0, 0, int(rng.integers(0, 8)))
        k2, c2 = bytearray(krec), bytearray(crec)
        for rec in (k2, c2):
            for i in range(K):
                if rng.integers(0, 4):                                      # three of four points in range, the rest random words
                    struct.pack_into("<ii", rec, 32 + 16 * i, int(rng.integers(0, 40)), int(rng.integers(0, 40)))
        out.append(Case(f"random_records_K{K}", K, dict(model=S, tolerance=3, max_scale=1024), bytes(m2), bytes(k2), bytes(c2)))
        out.append(Case(f"random_records_translation_K{K}", K, dict(model=T, tolerance=3), bytes(m2), bytes(k2), bytes(c2)))
    # min_inliers one above the best count: the zeroed form
    for c in [c for c in out if c.name in ("two_motions_rot90_6_4_tol0", "two_motions_translation_5_5_tol2", "full_similarity_K64", "usable_1_model0")]:
        top = fm.Record(fm.record_fast(c.mrec, c.krec, c.crec, c.K, **c.kw), c.K).inliers
        assert top >= 1
        out.append(Case(c.name + "_min_inliers_above", c.K, dict(c.kw, min_inliers=top + 1), c.mrec, c.krec, c.crec))
        out.append(Case(c.name + "_min_inliers_at", c.K, dict(c.kw, min_inliers=max(top, 1 + c.kw["model"])), c.mrec, c.krec, c.crec))
    assert len({c.name for c in out}) == len(out)
    return out


def many_records(R=300, K=64, full=7):
    """R records with a different number of pairs each, record `full` with all K: a record that finishes early sits beside one that runs
    long.  Returns (kw, [(mrec, krec, crec)])"""
    rng = np.random.default_rng(21)
    recs = []
    for r in range(R):
        n = K if r == full else (r * 37 + 11) % (K + 1)
        pts = scatter(rng, n)
        m = (2 * n + 2) // 3
        recs.append(fm.inputs(K, interleave(moved(pts[:m], ("rot90", "scale2", "rot180", "half")[r % 4]), noise(rng, pts[m:]))))
    return dict(model=S, tolerance=2), recs
