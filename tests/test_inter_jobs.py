"""Inter macroblocks on hand-built frame jobs (tests/jobgen.py: picture_samples, pcm_of, build_job(inter=...)), on the CPU: reference pictures
whose samples are chosen and level blocks that sit on the 16-bit bound of the packed residual (hd_resid.c: hd_residual_bound_ok, 32735).

  * A plain integer model (tests/inter_model.py) counts what the set INTER_SET reaches, per inter list and per letter of Table 8-12, and
    the set is held to it; no family of the set is spare.
  * The oracle the kernels are compared with on the GPU (tests/test_gpu_inter_jobs.py) equals that model byte for byte, on the set and on
    the 35 random pipeline pictures; a P picture over a flat picture is that flat picture, whatever the vectors.
  * The register arithmetic of the lane kernels (kernels/inter_lane_block.hip.h) runs on the CPU as a stand-alone program
    (tests/lane_arith/lane_arith_host.cpp, plain and with sanitizers) and equals the model on every window and block of the set and on a sweep
    of the bound: wherever the library clears FJ_CODED_WIDE, lb_residual_pk = lb_residual_32 = the model.

The set: (family, name, arguments).  Every recipe is its reference pictures (all I_PCM, unfiltered) and then P pictures that all go to the
slot behind them; `which` names the inter list that every macroblock of its P pictures is in (uni: one vector, k_recon_inter_lb; quad: one per
quadrant, k_recon_inter_lq; gen: sixteen, k_recon_inter), asserted from the header of each.
  flat       3 x 2 over flat 0 / flat 255: every fraction, windows inside and across the borders; the closed form.  (This family and `ramps`
             add no arithmetic class that the others do not reach: the reach test holds them by the pictures it requires as references,
             told from the decoded samples — content_of)
  periodic   3 x 2 over the period-3 columns, rows and lattice in both polarities: the exact ends of the six-tap and of the second-stage
             sums for every letter, both clips of every stage
  ramps      3 x 2 over the one-sample checkerboard and a ramp that saturates at both ends, and over the dark / bright noise pair
  fractions  11 x 6 over the checkerboard and the columns: each of the 64 chroma fractions, exact ties
  bound      2 x 2: every qp_y and qp_c, a lone level at an (odd, odd) position in every block, the largest inside the bound, both signs, luma
             against chroma in half of the macroblocks
  cdc        2 x 2: chroma DC levels (+-n, 0, 0, 0) at the bound at every qp_c, with and without AC; negative odd sums at qp_c < 6, among them
             sums whose halving decides a sample
  wide       2 x 2: two levels in row 0 that fail the bound while every sample stays in range (and reach -512, which nothing inside the bound does)
  over       2 x 2: the lone level one step past the bound where that is still inside 16 bits without the rounding term: bound in (32735, 32767],
             one sample at 512.  The only recipes whose residual leaves its range (the kernels' range wire fires): 16-bit arithmetic wraps here"""
import contextlib
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import h264bsd_amd
from oracle import pyoracle
import inter_model
import intra_model
import jobgen
from jobgen import build_job
from inter_model import LIMIT, LISTS, NORM_ADJUST
from replay_compare import RANDOM_PIPELINE, random_pipeline_jobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["flat", "periodic", "ramps", "fractions", "bound", "cdc", "wide", "over"]
WINDOW_PAIRS = {"flat": [("flat0", "flat255")], "periodic": [("cols+", "cols-"), ("rows+", "rows-"), ("lattice+", "lattice-")],
                "ramps": [("checker", "ramp"), ("dark", "bright")]}
P_PICTURES = {"uni": 6, "quad": 4, "gen": 2}                   # of a window recipe: every fraction over both references in every list
ODD = [(1, 1), (1, 3), (3, 1), (3, 3)]                         # (row, column): the positions of the largest scale
FJ_CODED_WIDE = 1 << 27
QP_C_VALUES = list(range(40))


def _set():
    out = []
    for family, pairs in WINDOW_PAIRS.items():
        out += [(family, f"{a}-{b}-{which}", (a, b, which)) for a, b in pairs for which in LISTS]
    out += [(family, which, (which,)) for family in ("fractions", "bound", "cdc", "wide", "over") for which in LISTS]
    return out


INTER_SET = _set()


def recipe_id(r):
    return f"{r[0]}-{r[1]}"


def _seed(r):
    return 41000 + INTER_SET.index(r)


def step(qp, cls=1):
    """the scale of a level at QP qp: cls 1 the (odd, odd) positions — the largest —, 0 the (even, even) ones, 2 the others (8.5.9)"""
    return NORM_ADJUST[qp % 6][cls] << (qp // 6)


def dc_step(qp_c):
    return NORM_ADJUST[qp_c % 6][0] << max(qp_c // 6 - 1, 0)


def lone(pos, level):
    lv = [0] * 16
    lv[4 * pos[0] + pos[1]] = level
    return lv


# ------------------------------------------------------------------ pictures
def references(rng, size, contents):
    w, h = size
    return [build_job(h264bsd_amd.lib(), rng, w, h, slot, len(contents) + 1, [], any_deblock=False, pcm=jobgen.pcm_of(jobgen.picture_samples(c, w, h, rng)))
            for slot, c in enumerate(contents)]


def spread(which, vec, k):
    """the vectors of macroblock k in the list `which` from a function vec(i) of a running index: one, four or sixteen"""
    n = {"uni": 1, "quad": 4, "gen": 16}[which]
    return [vec(n * k + i) for i in range(n)]


def p_picture(rng, size, n_refs, which, descs):
    """the P picture (slot n_refs) whose macroblocks are all described (jobgen.put_inter); its header must say that the intended kernel
    takes every one of them"""
    w, h = size
    job = build_job(h264bsd_amd.lib(), rng, w, h, n_refs, n_refs + 1, list(range(n_refs)), inter=descs)
    hd = pyoracle.blob_header(job)
    n = w * h
    want = {"uni": (n, n, 0), "quad": (n, 0, n), "gen": (n, 0, 0)}[which]
    assert len(descs) == n and (hd["n_gen"], hd["n_gen_uniform"], hd["n_gen_quad"]) == want, (which, hd["n_gen"], hd["n_gen_uniform"], hd["n_gen_quad"])
    return job


def _build_windows(rng, a, b, which):
    """vector g of the recipe (in the order of its pictures, macroblocks and blocks) has fraction g mod 16 and the reference (g div 16)
    mod 2: every letter over both pictures; whole parts that put windows inside the picture and across each border"""
    size = (3, 2)
    jobs = references(rng, size, [a, b])

    def vec(g):
        fx, fy = g % 4, (g // 4) % 4
        wx, wy = (7 * g) % 13 - 6, (5 * g) % 9 - 4
        if (fx, fy) == (0, 0): wx |= 1                                     # (half a chroma sample: never a copy macroblock)
        return 4 * wx + fx, 4 * wy + fy
    n = {"uni": 1, "quad": 4, "gen": 16}[which]
    for p in range(P_PICTURES[which]):
        descs = {}
        for mb in range(6):
            k = 6 * p + mb
            descs[mb] = dict(mv=spread(which, vec, k), slots=[((n * k) // 16) % 2])
        jobs.append(p_picture(rng, size, 2, which, descs))
    return jobs


def _build_fractions(rng, which):
    size = (11, 6)
    jobs = references(rng, size, ["checker", "cols+"])
    descs = {}
    for mb in range(66):
        def vec(i):
            f = (i * 37) % 64                                              # 37 is coprime with 64: every fraction, neighbours far apart
            return 8 * ((i % 5) - 2) + f % 8, 8 * ((i // 5) % 3 - 1) + f // 8
        descs[mb] = dict(mv=spread(which, vec, mb), slots=[(mb + q) % 2 for q in range(4)] if which != "uni" else [mb % 2])
        if which == "uni" and descs[mb]["mv"][0][0] % 8 == 0 and descs[mb]["mv"][0][1] % 8 == 0:
            descs[mb].update(qp_y=20, luma={0: lone((0, 0), 1)})            # whole chroma samples: one small level, or it is a copy macroblock
    return jobs + [p_picture(rng, size, 2, which, descs)]


def _vectors(which, k):
    """fractional vectors of a residual macroblock: what they predict does not matter, which list they put it in does"""
    return spread(which, lambda i: (4 * (i % 3) + 1 + (i % 2), 4 * ((i // 2) % 3) - 3 + (i % 4)), k)


def _residual_pictures(rng, which, mbs):
    """2 x 2 pictures (one group of four) over the dark / bright pair, macroblock k = mbs[k]: a dict of put_inter's residual keys"""
    jobs = references(rng, (2, 2), ["dark", "bright"])
    while len(mbs) % 4: mbs = mbs + [mbs[len(mbs) % 3]]
    for at in range(0, len(mbs), 4):
        descs = {a: dict(mbs[at + a], mv=_vectors(which, at + a), slots=[(at + a) % 2] if which == "uni" else [(a + q) % 2 for q in range(4)]) for a in range(4)}
        jobs.append(p_picture(rng, (2, 2), 2, which, descs))
    return jobs


def _build_bound(rng, which):
    mbs = []
    for k in range(52):
        qp_y, qp_c, pos = k, k % 40, ODD[k % 4]
        sl = 1 if k % 2 == 0 else -1
        sc = -sl if (k // 2) % 2 == 0 else sl                              # chroma against luma in every other pair of macroblocks
        mbs.append(dict(qp_y=qp_y, qp_c=qp_c, luma={z: lone(pos, sl * (LIMIT // step(qp_y))) for z in range(16)},
                        chroma_ac={c: lone(pos, sc * (LIMIT // step(qp_c))) for c in range(8)}))
    return _residual_pictures(rng, which, mbs)


def _build_cdc(rng, which):
    mbs = []
    for k in range(48):
        qp_c = k if k < 40 else (1, 2)[k % 2]
        d = dict(qp_y=30, qp_c=qp_c)
        sign = 1 if k % 4 < 2 else -1
        ac = 0
        if k % 2 and k < 40:                                               # half of the bound to a lone AC level, the rest to the DC
            ac = (LIMIT // 2) // step(qp_c)
            d["chroma_ac"] = {c: lone(ODD[(c + k) % 4], -sign * ac) for c in range(8)}
        n = (LIMIT - ac * step(qp_c)) // dc_step(qp_c)
        if qp_c in (1, 2) and n % 2 == 0: n -= 1                           # an odd level times an odd scale: the sum that >> 1 rounds down
        if k >= 40:
            # ... and rounds down across a step of (dc + 32) >> 6: -scale x n = 63 (mod 128), so dc = 31 (mod 64) where a truncating
            # division gives 32.  Scale 11 (qp_c 1): n = 99 (mod 128); scale 13 (qp_c 2): n = 5 (mod 128)
            n = ((99, 5)[qp_c - 1] + 128 * (k - 40)) % (LIMIT // dc_step(qp_c))
            assert (-n * NORM_ADJUST[qp_c][0]) % 128 == 63 and ((-n * NORM_ADJUST[qp_c][0]) >> 1) % 64 == 31
        d["chroma_dc"] = [sign * n, 0, 0, 0, -n if k >= 40 else -sign * n, 0, 0, 0]
        if k % 3 == 0: d["luma"] = {5: lone((0, 0), 3)}
        mbs.append(d)
    return _residual_pictures(rng, which, mbs)


def _build_wide(rng, which):
    """luma: levels L at (0, 0) and (0, 2), both of the smallest scale s: columns 0 and 3 of the block are 2 L s everywhere, inside the range
    while 2 L s <= 32735 (negative: 32800, which gives -512); the bound, which takes the largest scale for every level, fails by a factor 1.6.
    Chroma, whose (0, 0) is the DC's: levels at (0, 2) and (2, 0), which give +2 L s and -2 L s in one block"""
    mbs = []
    for k in range(52):
        qp_y, qp_c = k, (k * 7) % 40
        sign = -1 if k % 2 else 1
        ly, lc = sign * ((32800 if sign < 0 else LIMIT) // (2 * step(qp_y, 0))), LIMIT // (2 * step(qp_c, 0))
        d = dict(qp_y=qp_y, qp_c=qp_c, luma={z: [ly, 0, ly] + [0] * 13 for z in range(0, 16, 1 + k % 3)})
        if k % 4 >= 2: d["chroma_ac"] = {c: [0, 0, sign * lc, 0, 0, 0, 0, 0, sign * lc] + [0] * 7 for c in range(8)}
        mbs.append(d)
    return _residual_pictures(rng, which, mbs)


def over_qps():
    """the QPs at which the level behind the largest one inside the bound still has level x scale <= 32767"""
    return [qp for qp in range(52) if (LIMIT // step(qp) + 1) * step(qp) <= 32767]


def _build_over(rng, which):
    qps = over_qps()
    mbs = []
    for k in range(8):
        qp_y, qp_c = qps[k % len(qps)], qps[(3 * k + 1) % len(qps)]
        s = 1 if k % 2 == 0 else -1
        d = dict(qp_y=qp_y, qp_c=qp_c)
        if k % 4 < 2: d["luma"] = {z: lone(ODD[(z + k) % 4], s * (LIMIT // step(qp_y) + 1)) for z in range(16)}
        else: d["chroma_ac"] = {c: lone(ODD[(c + k) % 4], s * (LIMIT // step(qp_c) + 1)) for c in range(8)}
        mbs.append(d)
    return _residual_pictures(rng, which, mbs)


BUILDERS = dict(flat=_build_windows, periodic=_build_windows, ramps=_build_windows, fractions=_build_fractions, bound=_build_bound, cdc=_build_cdc,
                wide=_build_wide, over=_build_over)


@functools.lru_cache(maxsize=None)
def sequence(recipe):
    """the jobs of a recipe (the library must be built: the `built` fixture)"""
    return BUILDERS[recipe[0]](np.random.default_rng(_seed(recipe)), *recipe[2])


N_REFS = 2                                                     # every recipe: two reference pictures, then its P pictures


def content_of(frame, wmb, hmb):
    """which of jobgen.PICTURES a decoded reference picture is, from its samples alone: the named pictures sample for sample, the noise pair
    by its range (more than one value, all within 0 .. 5 or 250 .. 255); None for anything else"""
    for c in jobgen.PICTURES:
        if c not in ("dark", "bright") and np.array_equal(frame, np.concatenate([p.ravel() for p in jobgen.picture_samples(c, wmb, hmb)])): return c
    if len(np.unique(frame)) > 1: return "dark" if frame.max() <= 5 else "bright" if frame.min() >= 250 else None
    return None


@contextlib.contextmanager
def out_of_range_allowed(on=True):
    old = intra_model.RULES["reject_out_of_range"]
    intra_model.RULES["reject_out_of_range"] = not on
    try:
        yield
    finally:
        intra_model.RULES["reject_out_of_range"] = old


@functools.lru_cache(maxsize=None)
def rendered(recipe):
    """([(the oracle's un-deblocked P picture, the model's)], the census of all of them).  The model raises on a residual outside
    [-512, 511] in every family but `over`."""
    jobs = sequence(recipe)
    dpb = pyoracle.OracleDpb(jobs[0])
    slots = {}
    pairs, census = [], inter_model.Counter()
    for k, job in enumerate(jobs):
        frame = dpb.decode(job, deblock=False).copy()
        if k < N_REFS:
            slots[k] = frame
            continue
        with out_of_range_allowed(recipe[0] == "over"):
            mine, counts = inter_model.reconstruct(job, slots, frame)
        pairs.append((frame, np.frombuffer(mine, dtype=np.uint8)))
        census.update(counts)
        # what the picture predicts from, by the samples of the reference pictures that its macroblocks name
        wmb, hmb, recs = inter_model.job_view(job)[:3]
        for slot in sorted({s for rec in recs for s in rec["slots"]}):
            census[(recipe[2][-1], "content", content_of(slots[slot], wmb, hmb))] += 1
    return pairs, census


# ------------------------------------------------------------------ reach
def shortfalls(recipes):
    census = inter_model.Counter()
    for r in recipes: census.update(rendered(r)[1])
    out = []
    for which in LISTS:
        out += [f"{which}: class {c} {census[(which, c)]} times" for c in inter_model.CLASSES if census[(which, c)] < 10]
        for letters, classes in ((set(inter_model.H_LETTERS) | set(inter_model.J_LETTERS), ("hsum_min", "hsum_max")), (inter_model.V_LETTERS, ("vsum_min", "vsum_max")),
                                 (inter_model.J_LETTERS, ("jsum_min", "jsum_max"))):
            out += [f"{which}: letter {l} never has {c}" for l in sorted(letters) for c in classes if census[(which, "letter", l, c)] < 1]
        out += [f"{which}: chroma fraction ({xf}, {yf}) {census[(which, 'cfrac', xf, yf)]} times" for yf in range(8) for xf in range(8) if census[(which, "cfrac", xf, yf)] < 10]
        out += [f"{which}: qp_y {q} never inside the bound" for q in range(52) if census[(which, "qp_y", q)] < 1]
        out += [f"{which}: qp_c {q} never inside the bound" for q in QP_C_VALUES if census[(which, "qp_c", q)] < 1]
        out += [f"{which}: no P picture over {c}" for c in jobgen.PICTURES if census[(which, "content", c)] < 1]
    return out, census


def reach_table(census):
    lines = ["%-28s" % "class" + "".join("%10s" % w for w in LISTS)]
    lines += ["%-28s" % c + "".join("%10d" % census[(w, c)] for w in LISTS) for c in ["macroblocks"] + inter_model.CLASSES]
    lines.append("%-28s" % "rarest chroma fraction" + "".join("%10d" % min(census[(w, "cfrac", xf, yf)] for xf in range(8) for yf in range(8)) for w in LISTS))
    return "\n".join(lines)


def test_the_inter_set_reaches_what_it_is_for(built):
    missing, census = shortfalls(INTER_SET)
    print(reach_table(census))
    assert not missing, "\n".join(missing) + "\n" + reach_table(census)


@pytest.mark.parametrize("family", FAMILIES)
def test_no_family_of_the_set_is_spare(built, family):
    missing, _census = shortfalls([r for r in INTER_SET if r[0] != family])
    assert missing, f"the set reaches everything without the family {family}"


def test_residuals_are_in_range_except_where_built_to_be_wide(built):
    """FJ_CODED_WIDE, as the library sets it, is clear on every coded macroblock of the set but those of `wide` and `over`, where it is
    set; the model raises on a residual outside [-512, 511] but in `over`, whose every macroblock holds a sample of 512"""
    for r in INTER_SET:
        rendered(r)
        for job in sequence(r)[N_REFS:]:
            for rec in inter_model.job_view(job)[2]:
                if rec["coded"] & 0x02FFFFFF:
                    assert bool(rec["coded"] & FJ_CODED_WIDE) == (r[0] in ("wide", "over")), recipe_id(r)
    for r in (r for r in INTER_SET if r[0] == "over"):
        job = sequence(r)[N_REFS]
        with pytest.raises(ValueError):
            inter_model.reconstruct(job, {0: bytes(4 * 384), 1: bytes(4 * 384)}, bytes(4 * 384), census=False)


# ------------------------------------------------------------------ the oracle against the model
@pytest.mark.parametrize("recipe", INTER_SET, ids=recipe_id)
def test_oracle_equals_the_model(built, recipe):
    for k, (oracle, model) in enumerate(rendered(recipe)[0]):
        diff = np.nonzero(oracle != model)[0]
        assert diff.size == 0, f"P picture {k}: {diff.size} bytes differ, first at {int(diff[0])}: oracle {oracle[diff[0]]} model {model[diff[0]]}"


@functools.lru_cache(maxsize=None)
def random_census(seed, wmb, hmb):
    """the model over the five pictures of a random pipeline sequence (deblocked references, as the pipeline has them): the number of
    bytes that differ from the oracle's un-deblocked pictures, and the census.  Random levels ignore the residual range."""
    jobs = random_pipeline_jobs(h264bsd_amd.lib(), seed, wmb, hmb)
    dpb = pyoracle.OracleDpb(jobs[0])
    census, differ = inter_model.Counter(), 0
    with out_of_range_allowed():
        for job in jobs:
            slots = {s: dpb.slots[s][:dpb.frame_bytes].copy() for s in range(len(dpb.slots))}
            frame = dpb.decode(job, deblock=False).copy()
            mine, counts = inter_model.reconstruct(job, slots, frame)
            differ += int(np.count_nonzero(frame != np.frombuffer(mine, dtype=np.uint8)))
            census.update(counts)
            dpb.decode(job)
    return differ, census


@pytest.mark.parametrize("seed,wmb,hmb", RANDOM_PIPELINE)
def test_oracle_equals_the_model_on_the_random_pipeline_pictures(built, seed, wmb, hmb):
    assert random_census(seed, wmb, hmb)[0] == 0


def test_print_the_census_of_the_random_pictures(built):
    """(docs/PARITY.md holds this table next to the set's)"""
    census = inter_model.Counter()
    for case in RANDOM_PIPELINE: census.update(random_census(*case)[1])
    print(reach_table(census))
    assert sum(census[(w, "macroblocks")] for w in LISTS) > 1000


@pytest.mark.parametrize("recipe", [r for r in INTER_SET if r[0] == "flat"], ids=recipe_id)
def test_a_p_picture_over_a_flat_picture_is_flat(built, recipe):
    """the closed form: whatever the vector, every quadrant of every macroblock is the value of its reference picture — oracle and model"""
    value = {0: 0, 1: 255}
    jobs = sequence(recipe)
    for job, (oracle, model) in zip(jobs[2:], rendered(recipe)[0]):
        wmb, hmb, recs = inter_model.job_view(job)[:3]
        Y, C = np.zeros((16 * hmb, 16 * wmb), np.uint8), np.zeros((8 * hmb, 8 * wmb), np.uint8)
        for a, rec in enumerate(recs):
            for q in range(4):
                x, y = 2 * (a % wmb) + (q & 1), 2 * (a // wmb) + (q >> 1)
                Y[8 * y:8 * y + 8, 8 * x:8 * x + 8] = C[4 * y:4 * y + 4, 4 * x:4 * x + 4] = value[rec["slots"][q]]
        want = np.concatenate([Y.ravel(), C.ravel(), C.ravel()])
        assert np.array_equal(oracle, want) and np.array_equal(model, want)


# ------------------------------------------------------------------ the lane arithmetic on the CPU (tests/lane_arith/)
def find_clangxx():
    """the ROCm clang++ (what hipcc compiles the kernels with), else any clang++"""
    tried = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), sub, "clang++") for sub in ("llvm/bin", "lib/llvm/bin")]
    for path in tried + [shutil.which("clang++")]:
        if path and os.path.exists(path): return path
    return None


def build_host_program(workdir, sanitize=None):
    """tests/lane_arith/lane_arith_host.cpp as a program of its own, in the manner of tests/host_program.py: never loaded into Python"""
    cxx = find_clangxx()
    assert cxx is not None, "no clang++ found: the lane arithmetic has no CPU check without one"
    exe = os.path.join(workdir, "lane_arith_host" + ("_" + sanitize.replace(",", "_") if sanitize else ""))
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-Wall", os.path.join(ROOT, "tests", "lane_arith", "lane_arith_host.cpp"), "-o", exe]
    if sanitize: cmd += [f"-fsanitize={sanitize}", "-fno-omit-frame-pointer"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run_host_program(exe, workdir, cases):
    """cases: lists of ints behind their letter; returns the result lines as lists of ints"""
    src, dst = os.path.join(workdir, "cases.txt"), os.path.join(workdir, "results.txt")
    with open(src, "w") as f:
        f.write("\n".join(c[0] + " " + " ".join(str(int(v)) for v in c[1:]) for c in cases) + "\n")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    lines = open(dst).read().splitlines()
    assert len(lines) == len(cases), (len(lines), len(cases))
    return [[int(v) for v in ln.split()[1:]] for ln in lines]


@pytest.fixture(scope="module", params=[None, "address,undefined"], ids=["plain", "sanitizers"])
def host_program(request, tmp_path_factory):
    workdir = str(tmp_path_factory.mktemp("lane_arith"))
    return build_host_program(workdir, request.param), workdir


def residual_case(qp_y, qp_c, y, c, cdc, i, packed):
    return ["R", qp_y, qp_c, int(cdc is not None), i, int(packed)] + list(cdc if cdc is not None else [0] * 4) + list(y) + list(c)


def model_residual(qp_y, qp_c, y, c, cdc, i):
    """what the result line of a residual case must hold; None in place of a block that leaves [-512, 511]"""
    dc = intra_model.chroma_dc(list(cdc), qp_c)[i] if cdc is not None else 0
    out = [dc]
    for lv, qp, d in ((y, qp_y, None), (c, qp_c, dc)):
        try:
            out.append([v for row in intra_model.residual_block(list(lv), qp, d) for v in row])
        except ValueError:
            out.append(None)
    return out


def check_residuals(results, cases, wants, packed):
    n_packed = 0
    for got, case, (dc, y, c), pk in zip(results, cases, wants, packed):
        assert got[0] == dc, ("chroma DC", case, got[0], dc)
        assert got[1] == int(y is None) and got[2] == int(c is None), ("range verdicts", case, got[1:3])
        if y is not None: assert got[3:19] == y, ("lb_residual_32, luma", case, got[3:19], y)
        if c is not None: assert got[19:35] == c, ("lb_residual_32, chroma", case, got[19:35], c)
        if pk:
            assert y is not None and c is not None, ("the bound holds and a sample leaves the range", case)
            assert got[35:51] == y and got[51:67] == c, ("lb_residual_pk", case, got[35:67], y, c)
            n_packed += 1
    return n_packed


@functools.lru_cache(maxsize=None)
def set_cases():
    """every 4x4 luma window, every chroma row of the one-vector and quadrant macroblocks, and every pair of a luma block z with the chroma
    block z & 7 (the pairing of k_recon_inter_lb) of the P pictures of the set, with what the model gives for each; and of each case the
    inter list its macroblock is in"""
    cases, wants, where = [], [], []
    for r in INTER_SET:
        jobs = sequence(r)
        dpb = pyoracle.OracleDpb(jobs[0])
        refs = [intra_model.planes_of(dpb.decode(job, deblock=False).copy(), *inter_model.job_view(job)[:2]) for job in jobs[:N_REFS]]
        for job in jobs[N_REFS:]:
            wmb, hmb, recs, coef_off, lists = inter_model.job_view(job)
            W, H = 16 * wmb, 16 * hmb
            for a, rec in enumerate(recs):
                mbx, mby = a % wmb, a // wmb
                for blk in range(16):
                    bx, by = blk & 3, blk >> 2
                    mvx, mvy = rec["mv"][blk]
                    P = refs[rec["slots"][(by >> 1) * 2 + (bx >> 1)]]
                    x0, y0 = 16 * mbx + 4 * bx + (mvx >> 2) - 2, 16 * mby + 4 * by + (mvy >> 2) - 2
                    win = [[P[0][min(max(y0 + rr, 0), H - 1)][min(max(x0 + cc, 0), W - 1)] for cc in range(9)] for rr in range(9)]
                    cases.append(["L", mvx & 3, mvy & 3] + [v for row in win for v in row])
                    wants.append([v for row in inter_model.luma_block(win, mvx & 3, mvy & 3) for v in row])
                if lists.get(a) in ("uni", "quad"):
                    for q in range(4):
                        mvx, mvy = rec["mv"][(q >> 1) * 8 + (q & 1) * 2]
                        xf, yf = mvx & 7, mvy & 7
                        for plane in range(2):
                            P = refs[rec["slots"][q]][1 + plane]
                            x0, y0 = 8 * mbx + 4 * (q & 1) + (mvx >> 3), 8 * mby + 4 * (q >> 1) + (mvy >> 3)
                            rows = [[P[min(max(y0 + rr, 0), H // 2 - 1)][min(max(x0 + cc, 0), W // 2 - 1)] for cc in range(5)] for rr in range(5)]
                            for rr in range(4):
                                cases.append(["C", (8 - xf) * (8 - yf), xf * (8 - yf), (8 - xf) * yf, xf * yf] + rows[rr] + rows[rr + 1])
                                S = lambda x, y: rows[y][x]
                                wants.append([inter_model.chroma_sample(S, cc, rr, xf, yf) for cc in range(4)])
                if rec["coded"] & 0x02FFFFFF:
                    luma, cdc, cac = inter_model.mb_blocks(job, coef_off, rec)
                    for z in range(16):
                        k = z & 7
                        y, c, d = luma.get(z, intra_model.ZERO), cac.get(k, intra_model.ZERO), cdc[4 * (k >> 2):4 * (k >> 2) + 4] if cdc is not None else None
                        cases.append(residual_case(rec["qp_y"], rec["qp_c"], y, c, d, k & 3, not rec["coded"] & FJ_CODED_WIDE))
                        wants.append(model_residual(rec["qp_y"], rec["qp_c"], y, c, d, k & 3))
                where += [lists.get(a)] * (len(cases) - len(where))
    return cases, wants, where


def test_host_program_equals_the_model_on_the_set(built, host_program):
    exe, workdir = host_program
    cases, wants, where = set_cases()
    results = run_host_program(exe, workdir, cases)
    for which in ("uni", "quad"):                                          # all 64 chroma fractions reach lb_chroma_row in both lane lists
        weights = {tuple(c[1:5]) for c, w in zip(cases, where) if c[0] == "C" and w == which}
        assert weights == {((8 - xf) * (8 - yf), xf * (8 - yf), (8 - xf) * yf, xf * yf) for xf in range(8) for yf in range(8)}, (which, len(weights))
    resid = [(g, c, w) for g, c, w in zip(results, cases, wants) if c[0] == "R"]
    for got, case, want in zip(results, cases, wants):
        if case[0] != "R": assert got == want, (case[:5], got, want)
    n_packed = check_residuals([g for g, _, _ in resid], [c for _, c, _ in resid], [w for _, _, w in resid], [c[5] for _, c, _ in resid])
    kinds = [c[0] for c in cases]
    print(f"{kinds.count('L')} luma windows, {kinds.count('C')} chroma rows, {len(resid)} block pairs, {n_packed} of them packed")
    assert kinds.count("L") > 5000 and kinds.count("C") > 5000 and n_packed > 1000 and len(resid) - n_packed > 200


def many_levels(rng, total, ac_only):
    """a block of several levels whose magnitudes add up to `total`, at random positions with random signs"""
    lv = [0] * 16
    places = [int(p) for p in rng.choice(np.arange(1 if ac_only else 0, 16), int(rng.integers(2, 9)), replace=False)]
    cuts = sorted(int(v) for v in rng.integers(0, total + 1, len(places) - 1))
    for p, lo, hi in zip(places, [0] + cuts, cuts + [total]): lv[p] = (hi - lo) * int(rng.choice([-1, 1]))
    return lv


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """[(qp_y, qp_c, luma levels, chroma levels, the plane's DC levels or None, place of the block in the plane)]: the bound from both
    sides.  For every qp_y (and qp_c = qp_y mod 40) and each of the 16 positions, both signs: the lone level that is the largest inside the
    bound and the one behind it, in luma and — positions 1 .. 15 — in chroma; at position 0 of chroma the DC levels (+-n, 0, 0, 0) instead,
    n the largest inside and the one behind it.  Then blocks of several levels whose sum lies in the last scale step below 32735, chroma with
    a DC that takes a random share of the bound."""
    rng = np.random.default_rng(4242)
    out = []
    for qp_y in range(52):
        qp_c = qp_y % 40
        for pos in range(16):
            for sign in (1, -1):
                for more in (0, 1):
                    y = lone((pos >> 2, pos & 3), sign * (LIMIT // step(qp_y) + more))
                    if pos:
                        out.append((qp_y, qp_c, y, lone((pos >> 2, pos & 3), -sign * (LIMIT // step(qp_c) + more)), None, 0))
                    else:
                        out.append((qp_y, qp_c, y, [0] * 16, [-sign * (LIMIT // dc_step(qp_c) + more), 0, 0, 0], (qp_y + more) % 4))
        for k in range(6):
            share = int(rng.integers(0, LIMIT // dc_step(qp_c) + 1)) if k % 2 else 0
            cdc = [int(v) for v in rng.multinomial(share, [0.25] * 4) * rng.choice([-1, 1], 4)] if k % 2 else None
            out.append((qp_y, qp_c, many_levels(rng, LIMIT // step(qp_y), False), many_levels(rng, (LIMIT - share * dc_step(qp_c)) // step(qp_c), True), cdc, k % 4))
    return out


def wide_through_the_library(sweep):
    """FJ_CODED_WIDE of every case as h264bsdmiJobFinalize sets it (hd_residual_bound_ok on the sums of the macroblock's blocks): each case is
    an inter macroblock with one luma block, one chroma AC block and, where it has them, DC levels in one plane"""
    flags = []
    rng = np.random.default_rng(1)
    for at in range(0, len(sweep), 64):
        part = sweep[at:at + 64]
        descs = {}
        for a in range(64):
            qp_y, qp_c, y, c, cdc, i = part[a % len(part)]
            descs[a] = dict(mv=[(1, 2)], slots=[0], qp_y=qp_y, qp_c=qp_c, luma={3: y}, chroma_ac={i: c})
            if cdc is not None: descs[a]["chroma_dc"] = list(cdc) + [0] * 4
        job = build_job(h264bsd_amd.lib(), rng, 8, 8, 1, 2, [0], inter=descs)
        flags += [bool(rec["coded"] & FJ_CODED_WIDE) for rec in inter_model.job_view(job)[2]][:len(part)]
    return flags


def test_host_program_equals_the_model_on_a_sweep_of_the_bound(built, host_program):
    """the library's bound against the model's statement of it; wherever it holds, lb_residual_pk = lb_residual_32 = the model (the exact
    comparison is what shows an overflow of the packed sums: the sanitizers do not instrument vector arithmetic); where it fails,
    lb_residual_32 and its range verdict = the model, and the packed transform is not run: its sums would overflow, which is undefined"""
    exe, workdir = host_program
    sweep = sweep_cases()
    wide = wide_through_the_library(sweep)
    for (qp_y, qp_c, y, c, cdc, i), w in zip(sweep, wide):
        assert w == (not inter_model.bound_ok([y], list(cdc) + [0] * 4 if cdc is not None else None, [c], qp_y, qp_c)), ("the bound", qp_y, qp_c, y, c, cdc)
    cases = [residual_case(qp_y, qp_c, y, c, cdc, i, not w) for (qp_y, qp_c, y, c, cdc, i), w in zip(sweep, wide)]
    wants = [model_residual(*case) for case in sweep]
    n_packed = check_residuals(run_host_program(exe, workdir, cases), cases, wants, [not w for w in wide])
    peaks = [max(abs(v) for v in inter_model.peaks(y, qp_y)[:2]) for (qp_y, _qc, y, _c, _d, _i), w in zip(sweep, wide) if not w]
    print(f"{len(cases)} cases, {n_packed} packed; largest intermediate of a packed luma block {max(peaks)}")
    assert n_packed >= 52 * (16 * 2 + 6) and max(peaks) >= 32752 and sum(w is None for _d, w, _c in wants) >= 52 * 2
