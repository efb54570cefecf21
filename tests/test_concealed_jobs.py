"""Concealed macroblocks on hand-built frame jobs (tests/jobgen.py: patch_lost, chosen_samples), on the CPU: that the set REACHES
every neighbour mask, every position and every case of the concealment arithmetic, counted by a plain integer model
(tests/conceal_model.py) alone; that the oracle the kernels are compared with on the GPU (tests/test_gpu_concealed_jobs.py) equals
that model; and that the oracle and the parser equal the compiled reference on streams that lose exactly the chosen macroblocks
over exactly the chosen samples (tests/pcm_pictures.py: slice groups, a slice left out).

The set is CONCEALED_SET below: (family, width, height in macroblocks, decoded mask, survivors, content, seed).
  decoded mask   an int (bit a = macroblock a was decoded) or the name of a pattern of decoded_of()
  survivors      "pcm": I_PCM with chosen samples; "intra": Intra4x4 / Intra16x16 / a few I_PCM as build_job draws them, in the
                 intra schedule, so that the concealed macroblocks wait for them; "both": half and half; "p_copy0" / "p_copy1":
                 a P picture whose lost macroblocks are copies from that slot (FJ_MB_CONCEAL_P); "p_intra": a P picture whose
                 survivors are mostly inter and whose lost macroblocks are synthesised (FJ_MB_CONCEAL_I), as the reference does
                 when the last slice is I or no reference is usable
  content        of the I_PCM survivors: jobgen.CONTENTS or "mixed"
sequence() builds the pictures of a recipe: the concealed picture alone, or two intact pictures and the concealed P picture."""
import functools
import struct

import numpy as np
import pytest

import h264bsd_amd
from oracle import pyoracle
import conceal_model
import jobgen
from jobgen import build_job

COVER_3x3 = [1, 8, 32, 40, 64, 85, 101, 140, 161, 168, 224, 256, 276, 320]       # every (avail, position) of a 3 x 3 picture occurs
COVER_SMALL = {(1, 4): [1, 4, 5], (4, 1): [1, 4, 5], (2, 2): [1, 4, 6, 8, 10]}
PATTERNS = ["rows0", "rows1", "cols0", "cols1", "checker0", "checker1", "rect", "notches", "only_tl", "only_tr", "only_bl", "only_mid", "only_last"]
SINGLE = [p for p in PATTERNS if p.startswith("only_")]
BIG = [(5, 4), (11, 6)]
_CONTENT_CYCLE = jobgen.CONTENTS + ["mixed"]


def decoded_of(w, h, mask):
    """one truth value per macroblock"""
    n = w * h
    if isinstance(mask, int):
        return [bool((mask >> a) & 1) for a in range(n)]
    xy = [(a % w, a // w) for a in range(n)]
    if mask in ("rows0", "rows1"): return [y % 2 == int(mask[-1]) for x, y in xy]
    if mask in ("cols0", "cols1"): return [x % 2 == int(mask[-1]) for x, y in xy]
    if mask in ("checker0", "checker1"): return [(x + y) % 2 == int(mask[-1]) for x, y in xy]
    if mask == "rect": return [not (1 <= x < w - 1 and 1 <= y < h - 1) for x, y in xy]
    if mask == "notches":                                               # every other macroblock of each border but the corners: masks 7, 11, 13, 14
        return [not ((x in (0, w - 1) and y % 2 and y < h - 1) or (y in (0, h - 1) and x % 2 and x < w - 1)) for x, y in xy]
    only = {"only_tl": 0, "only_tr": w - 1, "only_bl": n - w, "only_mid": (h // 2) * w + w // 2, "only_last": n - 1}[mask]
    return [a == only for a in range(n)]


def _set():
    out, seed = [], 9000
    for use, survivors in enumerate(("pcm", "both")):
        for k, m in enumerate(COVER_3x3):
            out.append(("cover", 3, 3, m, survivors, _CONTENT_CYCLE[(k + 3 * use) % len(_CONTENT_CYCLE)], seed)); seed += 1
    for (w, h), masks in COVER_SMALL.items():
        for use, survivors in enumerate(("pcm", "both")):
            for k, m in enumerate(masks):
                out.append(("small", w, h, m, survivors, ("split", "noise", "mixed", "ramp", "flat255")[(k + 2 * use) % 5], seed)); seed += 1
    for w, h in ((1, 9), (9, 1)):                                       # masks 10 resp. 5 in a row
        for k, m in enumerate((0b101010101, 0b010101010)):
            for content in ("split", "noise", "ramp"):
                out.append(("alternating", w, h, m, "pcm", content, seed)); seed += 1
    for w, h in BIG:
        for k, p in enumerate(PATTERNS):
            out.append(("pattern", w, h, p, ("pcm", "intra", "both")[k % 3], ("mixed", "split", "noise")[(k // 3) % 3], seed)); seed += 1
    for w, h, p, slot in ((5, 4, "checker0", 0), (5, 4, "rect", 1), (11, 6, "rows1", 1), (11, 6, "only_mid", 0), (3, 3, 85, 0), (3, 3, 40, 1)):
        out.append(("p_copy", w, h, p, "p_copy%d" % slot, "noise", seed)); seed += 1
    for w, h, p in ((5, 4, "checker1"), (5, 4, "cols0"), (11, 6, "rect"), (11, 6, "rows0"), (3, 3, 161), (3, 3, 276)):
        out.append(("p_intra", w, h, p, "p_intra", "noise", seed)); seed += 1
    return out


CONCEALED_SET = _set()
FAMILIES = ["cover", "small", "alternating", "pattern", "p_copy", "p_intra"]
BIG_SET = [r for r in CONCEALED_SET if r[1:3] in BIG]
# the recipes whose macroblocks the compiled reference conceals from a stream (test_oracle_and_parser_equal_the_reference_...):
# all-I_PCM survivors, masks 10 and 13, both opposite-sides branches, both clips
STREAMED = [r for r in CONCEALED_SET if r[4] == "pcm" and r[0] in ("cover", "alternating", "small")] + \
           [r for r in CONCEALED_SET if r[4] == "pcm" and r[0] == "pattern" and r[1:3] == (5, 4)]


def recipe_id(r):
    return f"{r[0]}-{r[1]}x{r[2]}-{r[3]}-{r[4]}-{r[5]}"


def survivor_samples(recipe):
    """{macroblock: 384 samples} of the I_PCM survivors with chosen content, from the recipe's seed alone (the stream test gives
    the same ones to pcm_stream)"""
    _fam, w, h, mask, survivors, content, seed = recipe
    rng = np.random.default_rng(seed + 50000)
    dec = decoded_of(w, h, mask)
    out = {}
    for a in range(w * h):
        if dec[a] and (survivors == "pcm" or (survivors == "both" and rng.random() < 0.5)):
            out[a] = jobgen.chosen_samples(content, rng, a % w, a // w)
    return out


@functools.lru_cache(maxsize=None)
def sequence(recipe):
    """the jobs of a recipe; the concealed picture is the last (the library must be built: the `built` fixture)"""
    _fam, w, h, mask, survivors, _content, seed = recipe
    lib = h264bsd_amd.lib()
    rng = np.random.default_rng(seed)
    dec = decoded_of(w, h, mask)
    if not survivors.startswith("p_"):
        jobs = [build_job(lib, rng, w, h, 0, 4, [], p_pcm=0.1, pcm=survivor_samples(recipe), patch=jobgen.patch_lost(w, h, dec))]
    else:
        jobs = [build_job(lib, rng, w, h, 0, 4, [], p_pcm=0.1), build_job(lib, rng, w, h, 1, 4, [0])]
        slot = int(survivors[-1]) if survivors.startswith("p_copy") else None
        jobs.append(build_job(lib, rng, w, h, 2, 4, [0, 1], p_inter=0.85, patch=jobgen.patch_lost(w, h, dec, ref_slot=slot)))
    assert schedule_completes(jobs[-1]), "the intra schedule of the concealed picture never completes: a device would wait for ever"
    return jobs


# ------------------------------------------------------------------ views of a finished job
def job_view(job):
    h = h264bsd_amd.job_header(job)
    n = h["n_mbs"]
    recs = np.frombuffer(job, dtype=np.uint8, count=n * 32, offset=h["rec_off"]).reshape(n, 32)
    return dict(h=h, n=n, w=h["width_mbs"], hmb=h["height_mbs"], recs=recs, kind=recs[:, 0], down=struct.unpack_from("<I", job, 96)[0],
                coef_idx=np.frombuffer(recs[:, 12:16].tobytes(), dtype=np.uint32))


def lost_order(job):
    """[(mb, avail)] of the concealed macroblocks of a finished job, in concealment order (coef_idx)"""
    v = job_view(job)
    lost = [a for a in range(v["n"]) if v["kind"][a] in (jobgen.FJ_MB_CONCEAL_I, jobgen.FJ_MB_CONCEAL_P)]
    return [(a, int(v["recs"][a, 3])) for a in sorted(lost, key=lambda a: int(v["coef_idx"][a]))]


NEED_OFFSETS = [(-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1)]       # FJ_NEED_L, UL, U, UR, R, DR, D, DL (framejob.h)


def schedule_completes(job):
    """Run the device's dataflow rule on the CPU: a macroblock of the intra schedule starts when the neighbours named in its FJ_NEED_*
    mask (ref_slot[0]) that are themselves in the intra schedule are done.  False: some macroblocks wait for one another."""
    v = job_view(job)
    w, hmb = v["w"], v["hmb"]
    sched = {a for a in range(v["n"]) if v["kind"][a] in (1, 2, 3, jobgen.FJ_MB_CONCEAL_I)}
    pending, waiters = {}, {}
    for a in sched:
        x, y = a % w, a // w
        need = int(v["recs"][a, 16])
        for_ = [(y + dy) * w + x + dx for bit, (dx, dy) in enumerate(NEED_OFFSETS) if (need >> bit) & 1 and 0 <= x + dx < w and 0 <= y + dy < hmb]
        for_ = [b for b in for_ if b in sched]
        pending[a] = len(for_)
        for b in for_: waiters.setdefault(b, []).append(a)
    ready, done = [a for a in sched if not pending[a]], 0
    while ready:
        b = ready.pop()
        done += 1
        for a in waiters.get(b, ()):
            pending[a] -= 1
            if not pending[a]: ready.append(a)
    return done == len(sched)


@functools.lru_cache(maxsize=None)
def rendered(recipe):
    """(un-deblocked reconstruction of the concealed picture by the oracle, the same picture with its lost macroblocks concealed by
    the model instead, the model's census)"""
    _fam, w, h, _mask, survivors, _content, _seed = recipe
    jobs = sequence(recipe)
    dpb = pyoracle.OracleDpb(jobs[0])
    frames = [dpb.decode(job, deblock=False).copy() for job in jobs]
    order = lost_order(jobs[-1])
    pic = conceal_model.planes(frames[-1], w, h)
    for mb, _ in order:                                                # nothing of the oracle's lost macroblocks reaches the model
        for k, P in enumerate(pic):
            s = 8 if k else 16
            P[s * (mb // w):s * (mb // w) + s, s * (mb % w):s * (mb % w) + s] = 77
    counts = {"luma": dict.fromkeys(conceal_model.CLASSES, 0), "chroma": dict.fromkeys(conceal_model.CLASSES, 0)}
    if survivors.startswith("p_copy"):
        conceal_model.copy_lost(pic, conceal_model.planes(frames[int(survivors[-1])], w, h), w, order)
    else:
        conceal_model.conceal(pic, w, h, order, counts)
    return frames[-1], conceal_model.i420(pic), counts


# ------------------------------------------------------------------ reach
def enumerate_positions(w, h):
    """every (avail, first column, last column, first row, last row) that some decoded mask of a w x h picture produces"""
    found = set()
    for m in range(1, 1 << (w * h)):
        found |= {conceal_model.position(w, h, mb, av) for mb, av in conceal_model.walk(w, h, decoded_of(w, h, m))}
    return found


def reach(recipes):
    """what a set of recipes reaches, counted by the model: occurrences of every avail and of every position of the four small sizes,
    the census (planes per class, luma and chroma), and the recipes that break a condition of their own"""
    avail, positions = dict.fromkeys(range(1, 16), 0), {}
    in_a_row = {"mask 10 in a picture one macroblock wide": 0, "mask 5 in a picture one macroblock high": 0}
    census = {"luma": dict.fromkeys(conceal_model.CLASSES, 0), "chroma": dict.fromkeys(conceal_model.CLASSES, 0)}
    broken = []
    for r in recipes:
        fam, w, h, mask, survivors, _content, _seed = r
        dec = decoded_of(w, h, mask)
        order = conceal_model.walk(w, h, dec)
        job = sequence(r)[-1]
        v = job_view(job)
        if not survivors.startswith("p_copy"):
            for mb, av in order:
                avail[av] += 1
                if (w, h) in ((3, 3), (1, 4), (4, 1), (2, 2)):
                    key = ((w, h),) + conceal_model.position(w, h, mb, av)
                    positions[key] = positions.get(key, 0) + 1
            for plane in census:
                for name, c in rendered(r)[2][plane].items(): census[plane][name] += c
            for key, size, m in (("mask 10 in a picture one macroblock wide", w, 10), ("mask 5 in a picture one macroblock high", h, 5)):
                if size == 1: in_a_row[key] = max(in_a_row[key], sum(av == m for _mb, av in order))
        if not survivors.startswith("p_") and any(not dec[a] and dec[a + w] for a in range(w * h - w)) and not v["down"]:
            broken.append((recipe_id(r), "a macroblock is lost above a survivor, yet intra_down_deps is clear"))
        if not survivors.startswith("p_") and isinstance(mask, str) and mask in SINGLE and v["h"]["n_intra_levels"] < h:
            broken.append((recipe_id(r), f"one survivor, yet only {v['h']['n_intra_levels']} dependency levels for {h} rows"))
    broken += [(key, f"at most {c} times in one picture") for key, c in in_a_row.items() if c < 4]
    return avail, positions, census, broken


def reach_table(avail, positions, census):
    lines = ["avail  occurrences"] + [f"{a:5d}  {c:6d}" for a, c in avail.items()]
    lines += ["class                  luma planes  chroma planes"]
    lines += [f"{n:22s} {census['luma'][n]:11d} {census['chroma'][n]:14d}" for n in conceal_model.CLASSES]
    lines += [f"positions of the small sizes that occur: {len(positions)}, the rarest {min(positions.values()) if positions else 0} times"]
    return "\n".join(lines)


def shortfalls(recipes):
    """the conditions on the set that `recipes` miss"""
    avail, positions, census, broken = reach(recipes)
    out = [f"avail {a} occurs {c} times" for a, c in avail.items() if c < 10]
    n_positions = {(3, 3): 42, (1, 4): 5, (4, 1): 5, (2, 2): 10}
    for size, n in n_positions.items():
        want = enumerate_positions(*size)
        assert len(want) == n, (size, len(want))
        out += [f"position {(size,) + p} occurs {positions.get((size,) + p, 0)} times" for p in sorted(want) if positions.get((size,) + p, 0) < 2]
    for plane in ("luma", "chroma"):
        for name, c in census[plane].items():
            if c < (1 if name.startswith("SATURATED_") and name != "SATURATED_SIDE" else 10):
                out.append(f"{plane} class {name}: {c} planes")
    return out + [f"{rid}: {what}" for rid, what in broken], reach_table(avail, positions, census)


def test_the_concealed_set_reaches_what_it_is_for(built):
    missing, table = shortfalls(CONCEALED_SET)
    print(table)
    assert not missing, "\n".join(missing) + "\n" + table


@pytest.mark.parametrize("family", FAMILIES)
def test_no_family_of_the_set_is_spare(built, family):
    """without any one family some condition of the reach test fails, or (the P pictures) a kind of record no longer occurs"""
    rest = [r for r in CONCEALED_SET if r[0] != family]
    kinds = {(int(k), r[4].startswith("p_")) for r in rest for k in set(job_view(sequence(r)[-1])["kind"]) if int(k) in (4, 5)}
    missing, _table = shortfalls(rest)
    assert missing or kinds != {(4, False), (4, True), (5, True)}, f"the set reaches everything without the family {family}"


def test_every_recipe_loses_and_keeps_what_it_says(built):
    for r in CONCEALED_SET:
        _fam, w, h, mask, survivors, _content, _seed = r
        dec = decoded_of(w, h, mask)
        jobs = sequence(r)
        v = job_view(jobs[-1])
        want_kind = jobgen.FJ_MB_CONCEAL_P if survivors.startswith("p_copy") else jobgen.FJ_MB_CONCEAL_I
        assert [v["kind"][a] == want_kind for a in range(w * h)] == [not d for d in dec], recipe_id(r)
        assert lost_order(jobs[-1]) == [(mb, av if want_kind == 4 else 0) for mb, av in conceal_model.walk(w, h, dec)], recipe_id(r)
        kinds = {int(v["kind"][a]) for a in range(w * h) if dec[a]}
        if survivors == "pcm": assert kinds == {3}, recipe_id(r)
        if survivors == "p_intra" and w * h > 9: assert 0 in kinds, recipe_id(r)
        if survivors.startswith("p_copy"):
            assert all((v["recs"][a, 16:20] == int(survivors[-1])).all() for a in range(w * h) if not dec[a]), recipe_id(r)
    assert any({1, 2} & {int(k) for k in job_view(sequence(r)[-1])["kind"]} for r in CONCEALED_SET if r[4] in ("intra", "both"))


# ------------------------------------------------------------------ the oracle and the parser against the compiled reference
@functools.lru_cache(maxsize=None)
def stream_of(recipe):
    """Two all-I_PCM IDR pictures with two slice groups, the survivors (group 0) and the lost macroblocks (group 1).  The first
    picture holds the recipe's samples (survivor_samples) and its group-1 slice is missing; the second is intact.  The reference
    notices that the first picture is incomplete when the first slice of the second arrives (another idr_pic_id), conceals
    exactly the macroblocks of group 1 and delivers the picture with numErrMbs set; no call returns an error, the stream itself is
    well formed."""
    import pcm_pictures
    _fam, w, h, mask, _survivors, _content, seed = recipe
    dec = decoded_of(w, h, mask)
    samples = survivor_samples(recipe)
    rng = np.random.default_rng(seed + 70000)
    pictures = []
    for _ in range(2):
        pic = [np.zeros((16 * h, 16 * w), np.uint8), np.zeros((8 * h, 8 * w), np.uint8), np.zeros((8 * h, 8 * w), np.uint8)]
        for a in range(w * h):
            mb = samples[a] if dec[a] else rng.integers(0, 256, 384, dtype=np.uint8)
            x, y = a % w, a // w
            pic[0][16 * y:16 * y + 16, 16 * x:16 * x + 16] = mb[:256].reshape(16, 16)
            pic[1][8 * y:8 * y + 8, 8 * x:8 * x + 8] = mb[256:320].reshape(8, 8)
            pic[2][8 * y:8 * y + 8, 8 * x:8 * x + 8] = mb[320:].reshape(8, 8)
        pictures.append(tuple(pic))
    return pcm_pictures.pcm_stream(pictures, level=40, groups=[0 if d else 1 for d in dec], omit={0: (1,)})


def test_the_streamed_recipes_reach_every_mask_both_branches_and_both_clips(built):
    avail, census = set(), {"luma": dict.fromkeys(conceal_model.CLASSES, 0), "chroma": dict.fromkeys(conceal_model.CLASSES, 0)}
    for r in STREAMED:
        assert r[4] == "pcm"
        avail |= {av for _mb, av in conceal_model.walk(r[1], r[2], decoded_of(r[1], r[2], r[3]))}
        for plane in census:
            for name, c in rendered(r)[2][plane].items(): census[plane][name] += c
    assert avail == set(range(1, 16)), sorted(avail)
    for plane in census:
        assert all(census[plane][n] > 0 for n in ("LR_ONLY", "AB_ONLY", "CLIP_LOW", "CLIP_HIGH", "T1_NEG_ODD", "V_NEG_ODD", "FLAT")), census[plane]


@pytest.mark.parametrize("recipe", STREAMED, ids=recipe_id)
def test_oracle_and_parser_equal_the_reference_on_a_stream_that_loses_the_same_macroblocks(built, recipe):
    import synth
    _fam, w, h, mask, _survivors, _content, _seed = recipe
    dec = decoded_of(w, h, mask)
    stream = stream_of(recipe)
    ref_trace, ref_pics = synth.decode_reference(stream)
    trace, pics = synth.decode_ours(stream, "oracle")
    assert [tuple(t) for t in trace] == [tuple(t) for t in ref_trace], "h264bsdDecode call trace differs from the reference"
    assert [p[3] for p in ref_pics] == [dec.count(False), 0], "the reference did not conceal exactly the lost group"
    assert [p[1:] for p in pics] == [p[1:] for p in ref_pics], "output order / picId / isIdr / numErrMbs differ"
    assert [p[0] for p in pics] == [p[0] for p in ref_pics], "output pictures are not bit-exact"
    # the parser's records of the lost macroblocks are what patch_lost writes for the same mask, and the hand-built job's picture
    # (survivors of the same samples) is the stream's
    jobs, _trace, _info = h264bsd_amd.capture_stream(stream)
    v = job_view(jobs[0])
    recs = np.zeros((w * h, 32), np.uint8)
    recs[:, 0] = 3
    jobgen.patch_lost(w, h, dec)(recs, np.zeros((w * h, 16, 2), np.int16))
    for a in range(w * h):
        if not dec[a]:
            for what, lo, hi in (("kind", 0, 1), ("qp_y", 1, 2), ("qp_c", 2, 3), ("avail", 3, 4), ("pred", 4, 5), ("dbk", 5, 6), ("coef_idx", 12, 16)):
                assert bytes(v["recs"][a, lo:hi]) == bytes(recs[a, lo:hi]), f"macroblock {a}: {what} is {list(v['recs'][a, lo:hi])}, patch_lost writes {list(recs[a, lo:hi])}"
    ours = pyoracle.OracleDpb(jobs[0]).decode(jobs[0], deblock=False)
    assert np.array_equal(ours, rendered(recipe)[0]), "the stream's reconstruction is not the hand-built job's"


# ------------------------------------------------------------------ the largest legal frame
HUGE = (256, 144)


def huge_decoded(w=HUGE[0], h=HUGE[1]):
    """the top eight rows lost, and one macroblock in every 64 below them (never two of them next to one another)"""
    return [y >= 8 and (x + 9 * y) % 64 != 37 for y in range(h) for x in range(w)]


@functools.lru_cache(maxsize=None)
def huge_job():
    w, h = HUGE
    return build_job(h264bsd_amd.lib(), np.random.default_rng(43), w, h, 0, 2, [], patch=jobgen.patch_lost(w, h, huge_decoded()))


def test_the_huge_concealed_picture(built):
    """256 x 144 macroblocks: it has the downward dependencies that keep it in one band (tests/test_tick_plan.py: next to at most two
    wavefronts), its schedule completes, and the oracle equals the model on it"""
    w, h = HUGE
    job = huge_job()
    v = job_view(job)
    order = lost_order(job)
    assert v["down"] == 1 and v["h"]["n_intra_levels"] > 8 and len(order) == 8 * w + sum(1 for d in huge_decoded()[8 * w:] if not d)
    assert order == conceal_model.walk(w, h, huge_decoded())
    assert schedule_completes(job)
    frame = pyoracle.OracleDpb(job).decode(job, deblock=False).copy()
    pic = conceal_model.planes(frame, w, h)
    for mb, _ in order:
        pic[0][16 * (mb // w):16 * (mb // w) + 16, 16 * (mb % w):16 * (mb % w) + 16] = 77
    assert np.array_equal(conceal_model.i420(conceal_model.conceal(pic, w, h, order)), frame)


# ------------------------------------------------------------------ the oracle against the model
@pytest.mark.parametrize("recipe", CONCEALED_SET, ids=recipe_id)
def test_oracle_equals_the_model(built, recipe):
    """byte for byte on the whole picture: the survivors are the oracle's own, every concealed macroblock is the model's"""
    oracle, model, _counts = rendered(recipe)
    diff = np.nonzero(oracle != model)[0]
    assert diff.size == 0, f"{diff.size} bytes differ, first at {int(diff[0])}: oracle {oracle[diff[0]]} model {model[diff[0]]}"
