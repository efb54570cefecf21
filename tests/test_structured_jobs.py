"""Structured hand-built frame jobs (tests/jobgen.py: patch_typed, patch_sub8x8, patch_coherent, patch_copy_runs,
patch_window_edges, smooth content) on the CPU: that they REACH what the random jobs never do, that the host's proofs about
them are sound, and that the oracle they are compared with on the GPU (tests/test_gpu_structured_jobs.py) is itself pinned to
the compiled reference where the new cases are.

The structured set is STRUCTURED_SET below: (generator, width, height in macroblocks, seed); sequence() builds the
pictures of a recipe — an intra picture, then two structured P pictures (copy runs and coherent fields: three) that refer to everything before them."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import h264bsd_amd
from oracle import pyoracle
import jobgen
from jobgen import FJ_COPY_RUN, build_job
from replay_compare import RANDOM_PIPELINE, random_pipeline_jobs
from test_oracle_stage_pins import ref, ref_filter_picture  # noqa: F401 (ref is a fixture)

SIZES = [(1, 1), (1, 6), (6, 1), (2, 2), (3, 7), (5, 4), (11, 3), (19, 2)]       # 19 wide holds a stretch of 17, 3 wide makes runs wrap rows
GENERATORS = ["typed", "sub8x8", "coherent", "coherent_whole", "copy", "edges"]
SMOOTH = {"typed", "sub8x8", "coherent", "coherent_whole"}     # content that opens the filter; the reconstruction recipes keep the noise,
                                                                 # on which a window that is off by one sample shows everywhere
STRUCTURED_SET = [(g, w, h, 7000 + 100 * gi + si) for gi, g in enumerate(GENERATORS) for si, (w, h) in enumerate(SIZES)]
RECON_ONLY = [r for r in STRUCTURED_SET if r[0] in ("copy", "edges")]
BANDED = [r for r in STRUCTURED_SET if r[0] in ("coherent", "typed") and r[1:3] in ((5, 4), (3, 7))]


COPY_PLAN = jobgen.plan_copy_pictures([s for s in SIZES for _ in range(3)])       # the three P pictures of every "copy" recipe


def recipe_id(r):
    return f"{r[0]}-{r[1]}x{r[2]}"


@functools.lru_cache(maxsize=None)
def sequence(recipe):
    """the jobs of a recipe (the library must be built: the `built` fixture)"""
    gen, w, h, seed = recipe
    lib = h264bsd_amd.lib()
    rng = np.random.default_rng(seed)
    smooth = jobgen.draw_ramps(rng) if gen in SMOOTH else False     # one ramp for all pictures of the sequence
    n = w * h
    jobs = [build_job(lib, rng, w, h, 0, 4, [], p_pcm=0.6 if smooth else 0.1, smooth=smooth)]
    for pic, refs in ((1, [0]), (2, [0, 1]), (3, [0, 1, 2]))[:3 if gen in ("copy", "coherent", "coherent_whole") else 2]:
        kw = dict(p_inter=1.0, p_pcm=0.0, smooth=smooth)
        if gen == "typed":
            kw.update(p_inter=0.9, p_pcm=0.03, patch=jobgen.patch_typed(rng))
        elif gen == "sub8x8":
            kw.update(p_inter=0.9, p_pcm=0.03, patch=jobgen.patch_sub8x8(rng))
        elif gen in ("coherent", "coherent_whole"):
            kw.update(p_inter=0.95, p_pcm=0.04, patch=jobgen.patch_coherent(rng, w, whole=gen == "coherent_whole", still=pic != 2), extra_blocks=n)
        elif gen == "copy":
            kw.update(patch=jobgen.patch_copy_runs(w, COPY_PLAN[3 * SIZES.index((w, h)) + pic - 1]))
        else:
            kw.update(patch=jobgen.patch_window_edges(rng, w, first=37 * (seed % 100) + 401 * pic))
        jobs.append(build_job(lib, rng, w, h, pic, 4, refs, **kw))
    return jobs


def fixed_layout_sequence():
    """3x7: an intra picture, a picture that is ONE zero-motion copy stretch from slot 0, and the same from slot 1 with one coded
    macroblock in the middle"""
    lib = h264bsd_amd.lib()
    rng = np.random.default_rng(7999)
    jobs = [build_job(lib, rng, 3, 7, 0, 4, [], p_pcm=0.2)]
    jobs.append(build_job(lib, rng, 3, 7, 1, 4, [0], p_inter=1.0, p_pcm=0.0, patch=jobgen.patch_copy_runs(3, whole_picture=0)))
    jobs.append(build_job(lib, rng, 3, 7, 2, 4, [0, 1], p_inter=1.0, p_pcm=0.0, extra_blocks=1,
                          patch=jobgen.patch_copy_runs(3, whole_picture=1, coded_mb=10)))
    return jobs


@functools.lru_cache(maxsize=None)
def rendered(recipe):
    """[(job, un-deblocked reconstruction, final picture, census)] of a recipe, by the oracle; the census walk must leave the
    picture that oracle_deblock leaves"""
    jobs = sequence(recipe)
    dpb = pyoracle.OracleDpb(jobs[0])
    out = []
    for job in jobs:
        frame = dpb.decode(job, deblock=False)
        recon = frame.copy()
        census = pyoracle.deblock_census(job, frame)                  # in place: the slot now holds the deblocked picture
        out.append((job, recon, frame.copy(), census))
    return out


# ------------------------------------------------------------------ views of a finished job
def job_view(job):
    h = h264bsd_amd.job_header(job)
    n = h["n_mbs"]
    recs = np.frombuffer(job, dtype=np.uint8, count=n * 32, offset=h["rec_off"]).reshape(n, 32)
    v = dict(h=h, n=n, w=h["width_mbs"], recs=recs, kind=recs[:, 0], pred=recs[:, 4], dbk=recs[:, 5], trivial=recs[:, 21],
             coded=np.frombuffer(recs[:, 8:12].tobytes(), dtype=np.uint32), refs=recs[:, 16:20], mvs=h264bsd_amd.job_mvs(job).astype(int))
    v["copies"] = [struct.unpack_from("<HBBhh", job, h["copy_off"] + 8 * i) for i in range(h["n_copy"])]          # mb, slot, count, dx, dy
    v["gen"] = [struct.unpack_from("<HB", job, h["gen_off"] + 16 * i) for i in range(h["n_gen"])]                 # mb, uniform
    v["dbk_idx"] = [struct.unpack_from("<H", job, h["dbk_off"] + 2 * i)[0] for i in range(h["n_dbk"])]
    inter = v["kind"] == 0
    one_ref = (v["refs"] == v["refs"][:, :1]).all(axis=1)
    v["one_vector"] = inter & one_ref & (v["mvs"] == v["mvs"][:, :1]).all(axis=(1, 2))
    v["plain"] = v["one_vector"] & ((v["coded"] & 0x03FFFFFF) == 0)       # what fj_finalize_ex calls uniform: one vector, one reference, no coefficients
    return v


def wanted_neighbours(v, a):
    """the macroblocks across the left / upper edge of a that its flags have filtered"""
    return [p for bit, p in ((1, a - 1), (2, a - v["w"])) if v["dbk"][a] & bit]


# ------------------------------------------------------------------ reach
# census classes that no picture can take (oracle/pixel_oracle.c, next to the class list): an intra side gives strength 4 exactly on
# macroblock edges and 3 exactly inside, and the partition type rules inner edges only
UNREACHABLE = {"V_MB_BS3", "H_MB_BS3", "V_INNER_BS4", "H_INNER_BS4", "V_MB_BS0_BY_TYPE_MV_4_OR_MORE", "H_MB_BS0_BY_TYPE_MV_4_OR_MORE"}


def census_table(total):
    return "\n".join(f"{name:36s} {count:8d}" for name, count in total.items())


def window_keys(v):
    """(path, axis, plane, end, position relative to the border) of every reference window end of the picture that lies one sample
    inside, on, or one sample outside a border; and (path, horizontal fraction?, vertical fraction?) of the windows that have one"""
    S = (16 * v["w"], 16 * (v["n"] // v["w"]))
    keys, classes = set(), set()

    def window(path, block, pos, mv):
        hit = False
        for ax in range(2):
            first, last = pos[ax] + (mv[ax] >> 2) - 2, pos[ax] + (mv[ax] >> 2) + block + 2
            cfirst = pos[ax] // 2 + (mv[ax] >> 3)
            for plane, lo, hi, size in (("luma", first, last, S[ax]), ("chroma", cfirst, cfirst + block // 2, S[ax] // 2)):
                if lo in (-1, 0, 1): keys.add((path, ax, plane, "first", lo)); hit = True
                if hi - size in (-2, -1, 0): keys.add((path, ax, plane, "last", hi - size)); hit = True
        if hit: classes.add((path, bool(mv[0] & 3), bool(mv[1] & 3)))

    for a, uniform in v["gen"]:
        x, y = 16 * (a % v["w"]), 16 * (a // v["w"])
        mv = v["mvs"][a]
        if uniform == 1: window("one", 16, (x, y), mv[0])
        elif uniform == 2:
            for q in range(4): window("quad", 8, (x + 8 * (q & 1), y + 8 * (q >> 1)), mv[(q >> 1) * 8 + (q & 1) * 2])
        else:
            for b in range(16):
                pos = (x + 4 * (b & 3), y + 4 * (b >> 2))
                window("4x4", 4, pos, mv[b])
                if not (mv[b][0] & 3 or mv[b][1] & 3):                # whole samples: the block itself decides (k_recon_inter)
                    for ax in range(2):
                        first = pos[ax] + (mv[b][ax] >> 2)
                        if first in (-1, 0, 1): keys.add(("4x4 block", ax, "first", first))
                        if first + 3 - S[ax] in (-2, -1, 0): keys.add(("4x4 block", ax, "last", first + 3 - S[ax]))
    for mb, _slot, count, dx, dy in v["copies"]:
        for a in range(mb, mb + count):
            for ax, first in enumerate((16 * (a % v["w"]) + dx, 16 * (a // v["w"]) + dy)):
                if first in (-2, 0, 2): keys.add(("copy", ax, "first", first))
                if first + 16 - S[ax] in (-2, 0, 2): keys.add(("copy", ax, "last", first + 16 - S[ax]))
    return keys, classes


WINDOW_KEYS = {(p, ax, plane, end, t) for p in ("one", "quad", "4x4") for ax in range(2) for plane in ("luma", "chroma")
               for end, ts in (("first", (-1, 0, 1)), ("last", (-2, -1, 0))) for t in ts}
WINDOW_KEYS |= {("4x4 block", ax, end, t) for ax in range(2) for end, ts in (("first", (-1, 0, 1)), ("last", (-2, -1, 0))) for t in ts}
WINDOW_KEYS |= {("copy", ax, end, t) for ax in range(2) for end in ("first", "last") for t in (-2, 0, 2)}
# (path, fraction in x, fraction in y): whole-sample, horizontal-only, vertical-only, two-dimensional; a whole-sample one-vector
# macroblock without coefficients is a copy, with coefficients it takes the one-vector path
WINDOW_CLASSES = {(p, fx, fy) for p in ("one", "quad", "4x4") for fx in (False, True) for fy in (False, True)}


def test_the_structured_set_reaches_what_it_is_for(built):
    total, parts, quad = {}, set(), 0
    run_lengths = {False: set(), True: set()}                         # by "is displaced"
    wraps, via_uniform, via_other = 0, 0, 0
    keys, classes, displaced = set(), set(), set()
    for recipe in STRUCTURED_SET:
        for job, _recon, _final, census in rendered(recipe):
            for name, c in census.items(): total[name] = total.get(name, 0) + c
            v = job_view(job)
            quad += v["h"]["n_gen_quad"]
            parts |= {int(p >> 4) & 3 for p in v["pred"][v["kind"] == 0]}
            W, H = 16 * v["w"], 16 * (v["n"] // v["w"])
            for mb, _slot, count, dx, dy in v["copies"]:
                run_lengths[bool(dx or dy)].add(count)
                if count > 1 and (dx or dy):
                    x0, x1, y0 = 16 * (mb % v["w"]) + dx, 16 * ((mb + count - 1) % v["w"]) + dx, 16 * (mb // v["w"]) + dy
                    displaced |= {("dx % 4", dx % 4), ("dy / 2 odd", bool(dy // 2 & 1))}
                    if 0 <= x0 and x0 + 16 <= W and x1 + 16 > W: displaced.add("first inside, later ones across the right border")
                    if x0 < 0 and 0 <= x1: displaced.add("first ones across the left border, later ones inside")
                    if y0 < 0: displaced.add("across the upper border")
                    if y0 + 16 > H: displaced.add("across the lower border")
                wraps += (dx, dy) == (0, 0) and count > 1 and mb % v["w"] == v["w"] - 1 and v["w"] > 1
            for a in range(v["n"]):
                nb = wanted_neighbours(v, a)
                if v["kind"][a] == 0 and v["dbk"][a] and v["trivial"][a] and nb:
                    # the two branches of fj_dbk_trivial (hd_core.c): a neighbour that is itself plain, a coded or partitioned one
                    via_uniform += any(v["plain"][p] for p in nb)
                    via_other += any(not v["plain"][p] for p in nb)
            k, c = window_keys(v)
            keys |= k; classes |= c
    table = census_table(total)
    low = {n: c for n, c in total.items() if n not in UNREACHABLE and c < 10}
    assert not low, f"census classes taken fewer than 10 times: {low}\n{table}"
    assert all(total[n] == 0 for n in UNREACHABLE), table
    assert quad > 0, "no macroblock with one vector per quadrant (k_recon_inter_lq)"
    assert parts == {0, 1, 2, 3}, f"FJ_PARTS_* values that occur: {parts}"
    want = set(range(2, FJ_COPY_RUN + 1))
    assert want <= run_lengths[False] and want <= run_lengths[True], f"copy-run lengths: zero motion {run_lengths[False]}, displaced {run_lengths[True]}"
    want = {("dx % 4", 0), ("dx % 4", 2), ("dy / 2 odd", False), ("dy / 2 odd", True), "first inside, later ones across the right border",
            "first ones across the left border, later ones inside", "across the upper border", "across the lower border"}
    assert want <= displaced, f"displaced copy runs of more than one macroblock that never occur: {want - displaced}"
    assert wraps >= 1, "no zero-motion copy run starts in the last column of a row and goes on in the next"
    assert via_uniform >= 10 and via_other >= 10, f"macroblocks proved strength-free next to a plain neighbour: {via_uniform}, next to a coded or partitioned one: {via_other}"
    assert not WINDOW_KEYS - keys, f"window ends that never occur: {sorted(WINDOW_KEYS - keys, key=str)}"
    assert not WINDOW_CLASSES - classes, f"fraction classes that never occur at a border: {sorted(WINDOW_CLASSES - classes)}"


def test_every_stretch_length_is_laid_out(built):
    """every length 1 .. 2 * FJ_COPY_RUN + 1 of a stretch of equal copy macroblocks occurs (fj_copy_runs cuts them), and the picture
    that is one run"""
    lengths = set()
    for recipe in RECON_ONLY:
        for job in sequence(recipe)[1:]:
            v = job_view(job)
            key = [(int(v["refs"][a, 0]), tuple(v["mvs"][a, 0])) if v["plain"][a] and not (v["mvs"][a, 0] & 7).any() else None for a in range(v["n"])]
            a = 0
            while a < v["n"]:
                b = a
                while b + 1 < v["n"] and key[b + 1] == key[a] and (key[a] is None or key[a][1] == (0, 0) or (b + 1) % v["w"]): b += 1
                if key[a] is not None: lengths.add(b - a + 1)
                a = b + 1
    assert set(range(1, 2 * FJ_COPY_RUN + 2)) <= lengths, sorted(lengths)
    whole = job_view(fixed_layout_sequence()[1])
    assert [c[2] for c in whole["copies"]] == [8, 8, 5] and all(c[3:] == (0, 0) for c in whole["copies"])
    coded = job_view(fixed_layout_sequence()[2])
    assert [(c[0], c[2]) for c in coded["copies"]] == [(0, 8), (8, 2), (11, 8), (19, 2)] and coded["gen"] == [(10, 1)]


# ------------------------------------------------------------------ the host's proofs
ALL_JOBS = [("structured", r) for r in STRUCTURED_SET] + [("random", r) for r in RANDOM_PIPELINE]


def _jobs_of(which, r):
    return sequence(r) if which == "structured" else random_pipeline_jobs(h264bsd_amd.lib(), *r)


@pytest.mark.parametrize("which,r", ALL_JOBS, ids=[w + "-" + (recipe_id(r) if w == "structured" else "%d-%d-%d" % r) for w, r in ALL_JOBS])
def test_host_proofs_are_sound(built, which, r):
    for job in _jobs_of(which, r):
        v = job_view(job)
        bs = pyoracle.strengths(job).reshape(v["n"], 32)
        assert set(v["dbk_idx"]) == {a for a in range(v["n"]) if not v["trivial"][a]}, "dbk_idx is not the complement of dbk_trivial"
        for a in range(v["n"]):
            if v["trivial"][a]:
                assert not bs[a].any(), f"macroblock {a} is marked dbk_trivial but has strengths {bs[a].reshape(2, 4, 4).tolist()}"
            # the converse, as far as the host promises it: a filtered plain macroblock whose filtered neighbours are plain, have its
            # reference and vectors within 3
            if v["plain"][a] and v["dbk"][a]:
                nb = wanted_neighbours(v, a)
                if all(v["plain"][p] and v["refs"][p, 0] == v["refs"][a, 0] and np.abs(v["mvs"][p, 0] - v["mvs"][a, 0]).max() <= 3 for p in nb):
                    assert v["trivial"][a], f"macroblock {a} is not marked dbk_trivial"
                    assert not bs[a].any()
        # list classes, recomputed from the dense vectors
        m = v["mvs"].reshape(v["n"], 2, 2, 2, 2, 2)                   # [mb][qy][by][qx][bx][xy]
        in_quadrants = (m == m[:, :, :1, :, :1]).all(axis=(1, 2, 3, 4, 5))
        for a, uniform in v["gen"]:
            want = 1 if v["one_vector"][a] else 2 if in_quadrants[a] else 0
            assert uniform == want, f"macroblock {a}: list class {uniform}, vectors say {want}"
            if uniform == 2 and (v["refs"][a] == v["refs"][a, 0]).all():
                assert not (v["mvs"][a] == v["mvs"][a, 0]).all(), "equal inside each quadrant AND overall, yet in the quadrant list"
        listed = {a for a, _ in v["gen"]} | {a for mb, _s, count, _dx, _dy in v["copies"] for a in range(mb, mb + count)}
        assert listed == {a for a in range(v["n"]) if v["kind"][a] == 0}
        for mb, _s, count, dx, dy in v["copies"]:
            for a in range(mb, mb + count):
                assert v["plain"][a] and tuple(v["mvs"][a, 0]) == (4 * dx, 4 * dy) and not (v["mvs"][a, 0] & 7).any()


# ------------------------------------------------------------------ the oracle, pinned where the new cases are
@pytest.mark.parametrize("recipe", STRUCTURED_SET, ids=recipe_id)
def test_deblocking_of_structured_jobs_matches_h264bsdFilterPicture(ref, built, recipe):
    """from the oracle's own un-deblocked reconstruction, so that the content is the smooth one"""
    for i, (job, recon, final, _census) in enumerate(rendered(recipe)):
        theirs = ref_filter_picture(ref, job, jobgen.mb_types(job), recon)
        diff = np.nonzero(final != theirs)[0]
        assert diff.size == 0, f"picture {i}: {diff.size} samples differ, first at byte {int(diff[0])}"


@pytest.mark.parametrize("recipe", STRUCTURED_SET, ids=recipe_id)
def test_census_walk_leaves_the_picture_of_oracle_deblock(built, recipe):
    orc = pyoracle.oracle_lib()
    for job, recon, final, census in rendered(recipe):
        ours = recon.copy()
        buf = ctypes.create_string_buffer(job, len(job))
        assert orc.oracle_deblock(buf, ctypes.c_void_p(ours.ctypes.data)) == 0
        assert np.array_equal(ours, final)
        assert set(census) == set(pyoracle.census_names()) and len(census) == len(pyoracle.census_names())
