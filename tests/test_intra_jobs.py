"""Intra macroblocks on hand-built frame jobs (tests/jobgen.py: build_job(chosen=...), border_samples, intra_to_range), on the CPU:
that the set REACHES every Intra4x4 / Intra16x16 / chroma cell the rules allow and every named case of the prediction and residual
arithmetic, counted by a plain integer model (tests/intra_model.py) alone; that the oracle the kernels are compared with on the GPU
(tests/test_gpu_intra_jobs.py) equals that model byte for byte; that one-line mutants of the model differ from the oracle on the set;
and which Intra4x4 path of k_frame_intra (one macroblock per wavefront / up to four in 16-lane groups) the scheduling recipes take.

The set is INTRA_SET below: (family, name, arguments of the family's builder).  sequence() builds the pictures of a recipe.
  cells4     3 x 3 and 3 x 2 pictures, I_PCM but for the centre macroblock, which is Intra4x4 under one availability mask; nine
             pictures, picture m gives every block mode m where the block's neighbours allow it (else DC)
  cells16    11 x 6 lattices: Intra16x16 macroblocks at odd (x, y), I_PCM around them; every (availability, luma mode) and
             (availability, chroma mode); border content per recipe
  planes     the same lattice, plane prediction for luma and chroma over flat / stepped borders: b and c negative, zero, positive
             and at their extremes, values below 0 and above 255 before the clip
  edges      1 x 4, 4 x 1, 2 x 2 and 5 x 4 pictures of Intra4x4 macroblocks, modes 3 and 7 on blocks 1, 4, 5 wherever allowed:
             natural availability (last column: B without C), slices that start inside the picture, and C alone masked
  residual   every qp_y and qp_c; levels scaled against the model's own residual to both ends of [-512, 511]; luma / chroma DC whose
             scaled sums are negative and odd below QP 12 / 6; the RAW luma DC; Intra16x16 with DC only, AC only, both, neither
             (and AC blocks whose position 0 is not 0 although no DC block is coded)
  sched      availability 0 everywhere (everything ready at once): 2 x 2 and 3 x 3 Intra4x4, and 11 x 6 pictures whose groups of four
             run through the orders of Intra4x4 / Intra16x16 / I_PCM; full availability (the ready set is a diagonal); P pictures
             with a few chosen intra macroblocks among inter ones
  wide       33 x 2 and 65 x 2, for the band hand-over's poll (x += 64, seen bits in (wmb + 31) >> 5 words)"""
import contextlib
import functools

import numpy as np
import pytest

import h264bsd_amd
from oracle import pyoracle
import intra_model
import jobgen
from jobgen import build_job

FAMILIES = ["cells4", "cells16", "planes", "edges", "residual", "sched", "wide"]
LATTICE = (11, 6)
PLANE_BORDERS = [("flat0", "step_up", "step_up"), ("flat255", "step_down", "step_down"), ("flat0", "step_up", "flat0"),
                 ("flat255", "flat255", "step_down"), ("flat0", "flat0", "step_up"), ("flat255", "step_down", "flat255")]      # (D, B, A)


def _set():
    out = []
    for size in ((3, 3), (3, 2)):
        for avail in range(16):
            out.append(("cells4", f"{size[0]}x{size[1]}-avail{avail}", (size, avail)))
    for k, content in enumerate(["noise", "noise", "ramp", "flat0", "flat255", "step_up", "step_down"]):
        out.append(("cells16", f"{content}-{'residual' if k % 2 else 'bare'}", (content, k % 2)))
    out.append(("planes", "stepped-borders", ()))
    for size in ((1, 4), (4, 1), (2, 2), (5, 4)):
        n = size[0] * size[1]
        for how in ["natural", "no_c"] + [f"slice{s}" for s in sorted({1, n // 2, n - 1}) if s]:
            out.append(("edges", f"{size[0]}x{size[1]}-{how}", (size, how)))
    out += [("residual", "every-qp", ("qp",)), ("residual", "dc-parity", ("dc",)), ("residual", "raw-dc", ("raw",)), ("residual", "to-range", ("range",))]
    out += [("sched", "2x2-avail0", ("flat", (2, 2))), ("sched", "3x3-avail0", ("flat", (3, 3))), ("sched", "orders-avail0", ("orders",)),
            ("sched", "5x4-full", ("full", (5, 4))), ("sched", "11x6-full", ("full", (11, 6))), ("sched", "5x4-p", ("p", (5, 4))), ("sched", "11x6-p", ("p", (11, 6)))]
    out += [("wide", "33x2", ((33, 2),)), ("wide", "65x2", ((65, 2),))]
    return out


INTRA_SET = _set()
SCHEDULING = [r for r in INTRA_SET if r[0] == "sched"]
ENUMERATED = [r for r in INTRA_SET if r[0] in ("cells4", "cells16", "planes")]
BANDED = [r for r in INTRA_SET if r[1] in ("5x4-full", "11x6-full", "33x2", "65x2")]


def recipe_id(r):
    return f"{r[0]}-{r[1]}"


def _seed(r):
    return 31000 + INTRA_SET.index(r)


# ------------------------------------------------------------------ descriptions of chosen macroblocks (jobgen.put_chosen)
def _levels(rng, qp, ac_only=False, density=0.35):
    """a block of levels whose size follows the QP: about 100 / (scale << qp / 6) levels of residual each"""
    amp = max(1, min(12, (12 * 64) // (jobgen.LS2[qp % 6] << (qp // 6))))
    c = [int(v) for v in jobgen._coef_block(rng, ac_only, density, amp)]
    if not any(c): c[5] = 1
    return c


def _fits(d):
    r, coefs = np.zeros(32, np.uint8), np.zeros(27 * 16, np.int16)
    coded, _n = jobgen.put_chosen(r, d, coefs, 0, 1, 1, 3)
    try:
        intra_model.mb_residual(coefs.tobytes(), 0, dict(kind=d["kind"], qp_y=int(r[1]), qp_c=int(r[2]), coded=coded, coef_idx=0))
        return True
    except ValueError:
        return False


def fit(d):
    """halve the levels of a drawn macroblock until the model accepts its residual"""
    half = lambda lv: [int(v / 2) for v in lv]
    while not _fits(d):
        for key in ("luma", "chroma_ac"): d[key] = {z: half(lv) for z, lv in d.get(key, {}).items()}
        for key in ("luma_dc", "chroma_dc"):
            if d.get(key) is not None: d[key] = half(d[key])
    return d


def i4(rng, avail, modes=None, qp=None, p_coded=0.0, chroma=None, cqp_off=0):
    qp = int(rng.integers(0, 52)) if qp is None else qp
    left, top, corner = bool(avail & 1), bool(avail & 2), bool(avail & 8)
    if modes is None: modes = jobgen._i4_modes(rng, avail)
    cm = [0] + ([1] if left else []) + ([2] if top else []) + ([3] if left and top and corner else [])
    d = dict(kind=1, avail=avail, modes=modes, qp_y=qp, cqp_off=cqp_off, chroma=int(rng.choice(cm)) if chroma is None else chroma,
             luma={z: _levels(rng, qp) for z in range(16) if rng.random() < p_coded}, chroma_ac={})
    qc = jobgen.QPC[min(51, max(0, qp + cqp_off))]
    if rng.random() < p_coded:
        d["chroma_dc"] = [int(v) for v in rng.integers(-6, 7, 8)]
        d["chroma_ac"] = {k: _levels(rng, qc, True) for k in range(8) if rng.random() < 0.4}
    return fit(d)


def i16(rng, avail, l16=None, chroma=None, qp=None, shape=0, cqp_off=0, chroma_coded=None):
    """shape: bit 0 a DC block, bit 1 AC blocks"""
    qp = int(rng.integers(0, 52)) if qp is None else qp
    left, top, corner = bool(avail & 1), bool(avail & 2), bool(avail & 8)
    lm = [2] + ([0] if top else []) + ([1] if left else []) + ([3] if left and top and corner else [])
    cm = [0] + ([1] if left else []) + ([2] if top else []) + ([3] if left and top and corner else [])
    d = dict(kind=2, avail=avail, qp_y=qp, cqp_off=cqp_off, l16=int(rng.choice(lm)) if l16 is None else l16,
             chroma=int(rng.choice(cm)) if chroma is None else chroma, luma={}, chroma_ac={})
    if shape & 1: d["luma_dc"] = [int(v) for v in rng.integers(-10, 11, 16)]
    if shape & 2: d["luma"] = {z: _levels(rng, qp, True) for z in range(16) if rng.random() < 0.5} or {6: _levels(rng, qp, True)}
    qc = jobgen.QPC[min(51, max(0, qp + cqp_off))]
    if rng.random() < 0.5 if chroma_coded is None else chroma_coded:
        d["chroma_dc"] = [int(v) for v in rng.integers(-6, 7, 8)]
        d["chroma_ac"] = {k: _levels(rng, qc, True) for k in range(8) if rng.random() < 0.4}
    return fit(d)


def _picture(rng, size, chosen, contents=None, default="noise", cur_slot=0):
    """all macroblocks that are not chosen are I_PCM: contents[address] or the default"""
    w, h = size
    pcm = {a: jobgen.border_samples((contents or {}).get(a, default), rng) for a in range(w * h) if a not in chosen}
    return build_job(h264bsd_amd.lib(), rng, w, h, cur_slot, 4, [], pcm=pcm, chosen=chosen)


def _lattice(rng, tests, borders, cur_slot=0):
    """tests at odd (x, y) of an 11 x 6 picture, in raster order; borders[i] = (D, B, A) contents of test i's neighbours"""
    w, h = LATTICE
    spots = [(x, y) for y in range(1, h, 2) for x in range(1, w, 2)]
    chosen, contents = {}, {}
    for (x, y), d, (cd, cb, ca) in zip(spots, tests, borders):
        chosen[y * w + x] = d
        contents[(y - 1) * w + x - 1], contents[(y - 1) * w + x], contents[y * w + x - 1] = cd, cb, ca
    return _picture(rng, LATTICE, chosen, contents, cur_slot=cur_slot)


def slice_avail(a, w, start):
    """the availability of macroblock a when a slice starts at macroblock `start` (6.4.5: a neighbour in another slice is not available)"""
    x, y = a % w, a // w
    first = start if a >= start else 0
    nat = jobgen.natural_avail(x, y, w)
    return nat & ((1 if a - 1 >= first else 0) | (2 if a - w >= first else 0) | (4 if a - w + 1 >= first else 0) | (8 if a - w - 1 >= first else 0))


def _modes_37(rng, avail, k):
    """random valid modes, but diagonal down left / vertical left (3 / 7, which of them alternates with k) on blocks 1, 4, 5 where allowed"""
    modes = jobgen._i4_modes(rng, avail)
    for j, z in enumerate((1, 4, 5)):
        if 3 in jobgen._i4_ok(avail, z): modes[z] = (3, 7)[(j + k) % 2]
    return modes


# ------------------------------------------------------------------ the builders of the families
def _build_cells4(rng, size, avail):
    jobs = []
    bare = size == (3, 3)
    for m in range(9):
        modes = [m if m in jobgen._i4_ok(avail, z) else 2 for z in range(16)]
        content = jobgen.BORDERS[(avail + m) % len(jobgen.BORDERS)] if m not in (3, 7) else "noise"
        d = i4(rng, avail, modes, qp=int(rng.integers(16, 40)), p_coded=0.0 if bare else 0.5)
        jobs.append(_picture(rng, size, {size[0] + 1: d}, default=content))
    return jobs


def i16_cells():
    """(avail, luma mode, chroma mode): every (avail, luma mode) and every (avail, chroma mode) that is allowed"""
    out = []
    for avail in range(16):
        left, top, corner = bool(avail & 1), bool(avail & 2), bool(avail & 8)
        lm = [2] + ([0] if top else []) + ([1] if left else []) + ([3] if left and top and corner else [])
        cm = [0] + ([1] if left else []) + ([2] if top else []) + ([3] if left and top and corner else [])
        out += [(avail, lm[k % len(lm)], cm[k % len(cm)]) for k in range(max(len(lm), len(cm)))]
    return out


def _build_cells16(rng, content, residual):
    cells, jobs = i16_cells(), []
    for at in range(0, len(cells), 15):
        tests = [i16(rng, av, l, c, qp=int(rng.integers(10, 40)), shape=int(rng.integers(0, 4)) if residual else 0, chroma_coded=bool(residual)) for av, l, c in cells[at:at + 15]]
        d_content = {"step_up": "flat0", "step_down": "flat255"}.get(content, content)
        jobs.append(_lattice(rng, tests, [(d_content, content, content)] * len(tests)))
    return jobs


def _build_planes(rng):
    jobs = []
    for p in range(3):
        tests = [i16(rng, (15, 11)[(p + k) % 2], 3, 3, qp=28, shape=0, chroma_coded=False) for k in range(15)]
        jobs.append(_lattice(rng, tests, [PLANE_BORDERS[(k + p) % len(PLANE_BORDERS)] for k in range(15)]))
    return jobs


def _build_edges(rng, size, how):
    w, h = size
    jobs = []
    for k in range(2):
        chosen = {}
        for a in range(w * h):
            x, y = a % w, a // w
            avail = jobgen.natural_avail(x, y, w)
            if how == "no_c": avail &= ~4
            elif how.startswith("slice"): avail = slice_avail(a, w, int(how[5:]))
            chosen[a] = i4(rng, avail, _modes_37(rng, avail, k + a), qp=int(rng.integers(20, 36)), p_coded=0.3)
        jobs.append(_picture(rng, size, chosen))
    return jobs


def _scale_one(d, rng, towards):
    """one block of the macroblock to the end `towards` of the residual range (jobgen.intra_to_range), the others left alone"""
    if d["kind"] == 1 or not d.get("luma"):
        z = int(rng.integers(0, 16))
        lv = [0] * 16
        for i in rng.choice(16, 3, replace=False): lv[int(i)] = int(rng.choice([-3, -2, 2, 3]))
        if d["kind"] == 2: lv[0] = 0
        d.setdefault("luma", {})[z] = jobgen.intra_to_range(lv, d["qp_y"], towards, dc=0 if d["kind"] == 2 and d.get("luma_dc") is None else None)
    return d


def _build_residual(rng, what):
    size, jobs = (11, 6), []
    w, h = size
    n = w * h
    if what == "qp":
        for p in range(3):
            chosen = {}
            for a in range(n):
                qp, avail = (a + 17 * p) % 52, jobgen.natural_avail(a % w, a // w, w)
                chosen[a] = i4(rng, avail, qp=qp, p_coded=0.5) if (a + p) % 2 else i16(rng, avail, qp=qp, shape=(a // 2) % 4, chroma_coded=True)
                if not chosen[a].get("luma") and chosen[a].get("luma_dc") is None: chosen[a]["luma"] = {3: _levels(rng, qp, chosen[a]["kind"] == 2)}
                if chosen[a].get("chroma_dc") is None: chosen[a]["chroma_dc"] = [int(v) for v in rng.integers(-3, 4, 8)]
                fit(chosen[a])
            jobs.append(_picture(rng, size, chosen))
    elif what == "dc":
        for p in range(2):
            chosen = {}
            for a in range(n):
                qp = [1, 2, 7, 8, 13, 14, 26, 0, 6, 12, 39][(a + p) % 11]
                d = i16(rng, jobgen.natural_avail(a % w, a // w, w), qp=qp, shape=1 | (2 if a % 3 == 0 else 0), chroma_coded=True)
                if a % 4:                                              # an odd sum of levels: every element of the Hadamard sum is odd
                    d["luma_dc"][0] += 1 - sum(d["luma_dc"]) % 2
                    d["chroma_dc"][0] += 1 - sum(d["chroma_dc"][0:4]) % 2
                    d["chroma_dc"][4] += 1 - sum(d["chroma_dc"][4:8]) % 2
                chosen[a] = fit(d) if _fits(d) else i16(rng, 0, qp=qp, shape=0)
            jobs.append(_picture(rng, size, chosen))
    elif what == "raw":
        size = (5, 4)
        for p in range(2):
            chosen = {}
            for a in range(20):
                avail, qp = jobgen.natural_avail(a % 5, a // 5, 5), int(rng.integers(0, 52))
                if (a + p) % 2:                                        # the RAW form: the block holds the sixteen finished DC values
                    d = i16(rng, avail, qp=qp, shape=2 * (a % 4 < 2))
                    d["luma_dc"], d["raw"] = [int(v) for v in rng.integers(-6000, 6001, 16)], True
                else:                                                  # no DC block, and AC blocks whose position 0 is not 0: it counts as 0
                    d = i16(rng, avail, qp=qp, shape=2)
                    for z in d["luma"]: d["luma"][z][0] = int(rng.choice([-4, -1, 1, 3]))
                chosen[a] = fit(d)
            jobs.append(_picture(rng, size, chosen))
    else:
        for p in range(2):
            chosen = {}
            for a in range(n):
                qp = int(rng.integers(0, 34))
                d = i4(rng, 0, qp=qp, p_coded=0.0) if a % 2 else i16(rng, 0, qp=qp, shape=0, chroma_coded=False)
                chosen[a] = _scale_one(d, rng, -1 if (a // 2 + p) % 2 else 1)
                assert _fits(chosen[a])
            jobs.append(_picture(rng, size, chosen))
    return jobs


def no_inter_residual(recs, _mvs):
    """patch= of build_job: the inter macroblocks lose their coefficients.  build_job draws them without regard to the residual
    range, and no picture of this set may trip the kernels' range wire."""
    for a in range(recs.shape[0]):
        if recs[a, 0] == 0: jobgen._uncode(recs, a)


def order_kinds(group):
    """the kinds (1 Intra4x4, 2 Intra16x16, 3 I_PCM) of the four macroblocks of group g of the orders pictures: its digits in base 3"""
    return [1 + (group // 3 ** j) % 3 for j in range(4)]


def _build_sched(rng, what, size=None):
    lib = h264bsd_amd.lib()
    if what == "flat":
        return [_picture(rng, size, {a: i4(rng, 0, p_coded=0.4) for a in range(size[0] * size[1])}) for _ in range(2)]
    if what == "orders":                                               # 80 groups of four: every order of the three kinds but four I_PCM
        jobs = []
        for p in range(5):
            kinds = [k for g in range(16 * p, 16 * p + 16) for k in order_kinds(g)] + [1, 2]
            jobs.append(_picture(rng, (11, 6), {a: (i4(rng, 0, p_coded=0.4) if k == 1 else i16(rng, 0, shape=int(rng.integers(0, 4)))) for a, k in enumerate(kinds) if k != 3}))
        return jobs
    w, h = size
    if what == "full":
        jobs = []
        for p in range(2):
            chosen = {}
            for a in range(w * h):
                avail = jobgen.natural_avail(a % w, a // w, w)
                k = int(rng.integers(0, 10))
                if k < 6: chosen[a] = i4(rng, avail, p_coded=0.4)
                elif k < 9: chosen[a] = i16(rng, avail, shape=int(rng.integers(0, 4)))
            jobs.append(_picture(rng, size, chosen))
        return jobs
    jobs = _build_sched(rng, "full", size)[:1]
    for p in range(2):                                                 # P pictures: a few chosen intra macroblocks among inter ones
        chosen = {}
        for a in rng.choice(w * h, max(2, w * h // 8), replace=False):
            a = int(a)
            avail = jobgen.natural_avail(a % w, a // w, w)
            chosen[a] = i4(rng, avail, p_coded=0.4) if rng.random() < 0.7 else i16(rng, avail, shape=int(rng.integers(0, 4)))
        jobs.append(build_job(lib, rng, w, h, 1 + p, 4, list(range(1 + p)), p_inter=1.0, p_pcm=0.0, chosen=chosen, patch=no_inter_residual))
    return jobs


def _build_wide(rng, size, cur_slot=0):
    w, h = size
    chosen = {}
    for a in range(w * h):
        avail = jobgen.natural_avail(a % w, a // w, w)
        if a % 7 != 3: chosen[a] = i4(rng, avail, p_coded=0.3) if a % 3 else i16(rng, avail, shape=int(rng.integers(0, 4)))
    return [_picture(rng, size, chosen, cur_slot=cur_slot)]


BUILDERS = dict(cells4=_build_cells4, cells16=_build_cells16, planes=_build_planes, edges=_build_edges, residual=_build_residual,
                sched=_build_sched, wide=_build_wide)


@functools.lru_cache(maxsize=None)
def sequence(recipe):
    """the jobs of a recipe (the library must be built: the `built` fixture)"""
    return BUILDERS[recipe[0]](np.random.default_rng(_seed(recipe)), *recipe[2])


@functools.lru_cache(maxsize=None)
def oracle_frames(recipe):
    jobs = sequence(recipe)
    dpb = pyoracle.OracleDpb(jobs[0])
    return [dpb.decode(job, deblock=False).copy() for job in jobs]


@functools.lru_cache(maxsize=None)
def rendered(recipe):
    """[(the oracle's un-deblocked picture, the model's)] of every picture of the recipe and the census of all of them.  The model is
    given the oracle's picture for the macroblocks that are not intra, and fills every intra one with 77 before it starts."""
    pairs, census = [], intra_model.Counter()
    for job, frame in zip(sequence(recipe), oracle_frames(recipe)):
        mine, counts = intra_model.reconstruct(job, frame)
        pairs.append((frame, np.frombuffer(mine, dtype=np.uint8)))
        census.update(counts)
    return pairs, census


# ------------------------------------------------------------------ reach
def enumerate_cells():
    """The enumeration redone here, from the clauses and not from the model's helper: per availability mask (A 1, B 2, C 4, D 8) what
    each of the 16 blocks (block order of 6.4.3) sees and which modes that allows; the (mode, A, B) cells of Intra16x16 and chroma;
    the 16 chroma DC cells."""
    want = set()
    xy = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0), (2, 1), (3, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 2), (3, 2), (2, 3), (3, 3)]
    for avail in range(16):
        A, B, C, D = (bool(avail & b) for b in (1, 2, 4, 8))
        for z, (bx, by) in enumerate(xy):
            left, top = A or bx > 0, B or by > 0
            corner = D if (bx, by) == (0, 0) else B if by == 0 else A if bx == 0 else True
            if by == 0: tr = C if bx == 3 else B
            else: tr = bx < 3 and xy.index((bx + 1, by - 1)) < z
            modes = {2} | ({0, 3, 7} if top else set()) | ({1, 8} if left else set()) | ({4, 5, 6} if left and top and corner else set())
            want |= {("i4", z, m, left, top, corner, tr) for m in modes}
        plane = A and B and D
        want |= {("i16", m, A, B) for m, ok in ((0, B), (1, A), (2, True), (3, plane)) if ok}
        want |= {("chroma", m, A, B) for m, ok in ((0, True), (1, A), (2, B), (3, plane)) if ok}
        want |= {("chroma_dc", kk, A, B) for kk in range(4)}
    return want


QP_C_VALUES = sorted(set(jobgen.QPC))


def reach(recipes):
    census = intra_model.Counter()
    for r in recipes: census.update(rendered(r)[1])
    return census


def shortfalls(recipes):
    census = reach(recipes)
    cells = enumerate_cells()
    assert cells == intra_model.cells() and len(cells) > 200, "the enumeration here and the model's differ"
    out = [f"cell {c} occurs {census[c]} times" for c in sorted(cells) if census[c] < 2]
    out += [f"class {name}: {census[name]} times" for name in intra_model.CLASSES if census[name] < 10]
    out += [f"qp_y {q}: {census[('qp_y', q)]} macroblocks" for q in range(52) if census[("qp_y", q)] < 3]
    out += [f"qp_c {q}: {census[('qp_c', q)]} macroblocks" for q in QP_C_VALUES if census[("qp_c", q)] < 3]
    return out, census


def reach_table(census):
    cells = enumerate_cells()
    groups = {}
    for c in cells: groups.setdefault(c[0], []).append(census[c])
    lines = [f"{name} cells: {len(v)}, the rarest {min(v)} times" for name, v in sorted(groups.items())]
    lines += [f"{name:32s} {census[name]:6d}" for name in intra_model.CLASSES]
    lines += ["qp_y: the rarest value %d macroblocks; qp_c: %d" % (min(census[("qp_y", q)] for q in range(52)), min(census[("qp_c", q)] for q in QP_C_VALUES))]
    return "\n".join(lines)


def test_the_intra_set_reaches_what_it_is_for(built):
    missing, census = shortfalls(INTRA_SET)
    print(reach_table(census))
    assert not missing, "\n".join(missing) + "\n" + reach_table(census)


# what the scheduling and wide families are for is not arithmetic: their pictures are held to their shape instead
def shape_shortfalls(recipes):
    out = []
    names = {r[1] for r in recipes}
    for r in recipes:
        for job in sequence(r):
            h = pyoracle.blob_header(job)
            wmb, _hmb, recs, _ = intra_model.job_view(job)
            need = [job[h["rec_off"] + 32 * a + 16] for a in range(h["n_mbs"])]
            if r[0] == "sched" and r[2][0] in ("flat", "orders") and (any(need) or h["n_intra_levels"] != 1): out.append(f"{recipe_id(r)}: not everything is ready at once")
            if r[0] == "sched" and r[2][0] == "full" and h["n_intra_levels"] < wmb: out.append(f"{recipe_id(r)}: {h['n_intra_levels']} dependency levels")
    for name in ("2x2-avail0", "3x3-avail0", "orders-avail0", "5x4-full", "11x6-full", "5x4-p", "11x6-p", "33x2", "65x2"):
        if name not in names: out.append(f"no recipe {name}")
    if "orders-avail0" in names:
        r = next(r for r in recipes if r[1] == "orders-avail0")
        seen = set()
        for job in sequence(r):
            kinds = [rec["kind"] for rec in intra_model.job_view(job)[2]]
            seen |= {tuple(kinds[4 * g:4 * g + 4]) for g in range(16)}
        if len(seen) != 80: out.append(f"{len(seen)} orders of kinds in a group of four")
    for name in ("5x4-p", "11x6-p"):
        for r in (r for r in recipes if r[1] == name):
            for job in sequence(r)[1:]:
                recs = intra_model.job_view(job)[2]
                n_intra = sum(rec["kind"] in (1, 2) for rec in recs)
                if not 0 < 4 * n_intra <= len(recs): out.append(f"{name}: {n_intra} intra macroblocks of {len(recs)}")
    return out


def test_the_scheduling_and_wide_recipes_have_their_shape(built):
    assert not shape_shortfalls(INTRA_SET)


@pytest.mark.parametrize("family", FAMILIES)
def test_no_family_of_the_set_is_spare(built, family):
    rest = [r for r in INTRA_SET if r[0] != family]
    missing, _census = shortfalls(rest)
    assert missing or shape_shortfalls(rest), f"the set reaches everything without the family {family}"


def test_residuals_stay_in_range_and_modes_are_valid(built):
    """the model raises on a residual outside [-512, 511] and on a mode that reads a sample that is not there: rendering is the test"""
    for r in INTRA_SET: rendered(r)


# ------------------------------------------------------------------ the oracle against the model
@pytest.mark.parametrize("recipe", INTRA_SET, ids=recipe_id)
def test_oracle_equals_the_model(built, recipe):
    for k, (oracle, model) in enumerate(rendered(recipe)[0]):
        diff = np.nonzero(oracle != model)[0]
        assert diff.size == 0, f"picture {k}: {diff.size} bytes differ, first at {int(diff[0])}: oracle {oracle[diff[0]]} model {model[diff[0]]}"


# ------------------------------------------------------------------ mutants of the model
MUTANTS = {
    "block 5 takes has_tr from B": ("tr_of_block5", lambda avail: bool(avail & 2)),
    "above-right replicated from above[7]": ("tr_replica", lambda row: row[7] if row[7] is not None else row[3]),
    "luma DC below QP 12 without the rounding term": ("luma_dc_round", lambda q6: 0),
    "chroma DC >> 1 as a truncating division": ("chroma_dc_halve", lambda v: int(v / 2)),
    "chroma DC block 1 prefers left": ("chroma_dc_block1_first", "left"),
    "plane b with + 31": ("plane_b_round", 31),
    "Intra16x16 DC from position 0 when no DC block": ("i16_dc_absent", lambda level0: level0),
    "no clip at 0": ("clip_lo", lambda v: v & 255),
    "no clip at 255": ("clip_hi", lambda v: v & 255),
}


@contextlib.contextmanager
def mutated(name):
    key, rule = MUTANTS[name]
    old = intra_model.RULES[key]
    intra_model.RULES[key] = rule
    try:
        yield
    finally:
        intra_model.RULES[key] = old


def mutant_differences(name, recipes):
    """the recipes on which the mutated model and the unchanged oracle differ"""
    out = []
    with mutated(name):
        for r in recipes:
            try:
                if any(not np.array_equal(frame, np.frombuffer(intra_model.reconstruct(job, frame, census=False)[0], dtype=np.uint8))
                       for job, frame in zip(sequence(r), oracle_frames(r))):
                    out.append(r)
            except ValueError:                                         # (a mutated rule may leave the residual range or the picture: that is a difference too)
                out.append(r)
    return out


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_model_mutant_differs_from_the_oracle(built, name):
    differing = mutant_differences(name, INTRA_SET)
    print(f"{name}: {len(differing)} of {len(INTRA_SET)} recipes")
    assert differing, f"the mutant '{name}' equals the oracle on every recipe: the set has a hole"


# ------------------------------------------------------------------ which Intra4x4 path a picture takes
def claim_groups(ready, waves):
    """The claim rule of k_frame_intra for a picture whose `ready` macroblocks are all ready at once: a free wavefront takes
    share = (ready - claimed) / wavefronts of them, at least 1 and at most 4; Intra4x4 macroblocks of a group of more than one are
    predicted jointly (intra4_joint), a lone macroblock takes the ten-step loop of intra_mb.  (Every claim sees the cursor that
    the claim before it left, so the sizes do not depend on which wavefront wins.)"""
    groups, claimed = [], 0
    while claimed < ready:
        k = min(4, max(1, (ready - claimed) // waves))
        groups.append(k)
        claimed += k
    return groups


def test_which_path_the_scheduling_recipes_take(built):
    """From the code: the queue of a picture whose macroblocks all have availability 0 holds every macroblock before the first claim
    (they are queued while the dependency counts are set up).  At intra_waves = 1 the 2 x 2 picture is one joint group of four and
    the 3 x 3 one is 4 + 4 + 1; at 12 both are single-path throughout.  The 11 x 6 orders pictures are 16 groups of four and one of
    two at one wavefront (the share is whatever is left: 66 = 16 x 4 + 2), so group g holds the kinds order_kinds(g); at 4
    wavefronts they start with groups of four (66 / 4 > 4) and end in singles; at 12 the first claims take 4 (66 / 12 = 5) and
    the sizes fall to 1 once fewer than 24 are left.  Full-availability pictures start from the first macroblock and their I_PCM ones and then have
    about one ready macroblock per row (an Intra4x4 macroblock waits for its above-right neighbour); P pictures have few intra
    macroblocks.  Never 24 ready at once: single path at 12 wavefronts; at 4 a group of two can form when 8 are ready; at
    intra_waves = 1 every claim of more than one ready macroblock is a joint group."""
    assert claim_groups(4, 1) == [4] and claim_groups(9, 1) == [4, 4, 1]
    assert claim_groups(4, 12) == [1] * 4 and claim_groups(9, 12) == [1] * 9
    assert claim_groups(4, 4) == [1] * 4 and claim_groups(9, 4) == [2, 1, 1, 1, 1, 1, 1, 1]
    assert claim_groups(66, 1) == [4] * 16 + [2]
    g4, g12 = claim_groups(66, 4), claim_groups(66, 12)
    assert g4[:12] == [4] * 12 and g4[-1] == 1 and sum(g4) == 66
    assert g12[:5] == [4] * 5 and g12[-12:] == [1] * 12 and sum(g12) == 66
    for r in SCHEDULING:
        if r[2][0] in ("flat", "orders"):
            for job in sequence(r):
                h = pyoracle.blob_header(job)
                assert h["n_intra"] == h["n_mbs"], "I_PCM macroblocks are claimed like the others"
