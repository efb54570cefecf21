"""k_dbk's own output — the 48-byte deblocking records and the flag bytes (DBKF_*) — against tests/dbk_record_model.py, byte for byte.
The pictures k_frame_dbk makes from the records do not pin them: a wrong scheduling flag need not change a sample, it can turn into
a race instead.  h264bsdmiReplayDbkRecords (Replay.dbk_records) launches k_dbk alone for one tick and copies the scratch out.

k_dbk works one macroblock per lane, 64 list entries per wavefront, on a grid sized by the tick's longest list.  The sizes are the
smallest at which that can go wrong: no neighbours (1x1), no left / no upper neighbour (1x9, 9x1), a list exactly one wavefront long
(8x8 with every macroblock listed: 64), one lane into the second wavefront (13x5: 65), one lane short of a full one (9x7: 63), several
wavefronts (20x12: up to 240), a second workgroup (33x16 with every macroblock listed: 528, a workgroup takes 512).  The kernel has no stride loop, so no picture longer than one pass of the grid
exists; instead the two-stream ticks at the end mix lists whose lengths differ by more than 64, where the workgroups of the shorter
picture leave early."""
import functools
import os
import re

import numpy as np
import pytest

import h264bsd_amd
import jobgen
from jobgen import build_job
from conftest import ROOT
import dbk_record_model as model

SIZES = [(1, 1), (1, 9), (9, 1), (8, 8), (13, 5), (9, 7), (20, 12), (33, 16)]
BIG = (33, 16)                         # more than one workgroup: three kinds are enough
KINDS = ["intra", "intra-all", "p06-random", "p06-typed", "p06-sub8x8", "p097-random", "p097-typed", "p097-coherent", "empty-list", "p06-typed-unfiltered", "p06-typed-all"]
HALF = ("intra-half", 20, 12)          # an intra picture whose lower half is not filtered: a list half as long (two-stream ticks)
CASES = [(k, w, h) for (w, h) in SIZES for k in KINDS if (w, h) != BIG or k in ("intra-all", "p06-typed-all", "p097-random")]


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}"


def _all_filtered(w):
    """every macroblock filtered on every edge it has: an intra picture then lists all of its macroblocks"""
    def patch(recs, mvs16):
        for a in range(recs.shape[0]):
            recs[a, 5] = 4 | (1 if a % w else 0) | (2 if a >= w else 0)
    return patch


@functools.lru_cache(maxsize=None)
def job_of(kind, w, h):
    """one picture; k_dbk reads the job alone, so the P pictures need no decoded references behind them"""
    lib = h264bsd_amd.lib()
    n = w * h
    if kind == "p06-typed-unfiltered":
        # listed but not filtered (k_dbk then zeroes bytes 46..47 and the flag byte): the host lists no such macroblock, so the dbk byte of
        # every third listed macroblock of a finished job is cleared
        job = bytearray(job_of("p06-typed", w, h))
        head = h264bsd_amd.job_header(bytes(job))
        for i in range(0, head["n_dbk"], 3):
            job[head["rec_off"] + 32 * int.from_bytes(job[head["dbk_off"] + 2 * i:head["dbk_off"] + 2 * i + 2], "little") + 5] = 0
        return bytes(job)
    rng = np.random.default_rng(9100 + 17 * (KINDS + [HALF[0]]).index(kind) + 1000 * SIZES.index((w, h)))
    if kind == "intra":
        return build_job(lib, rng, w, h, 0, 4, [], p_pcm=0.2)
    if kind == "intra-half":
        return build_job(lib, rng, w, h, 0, 4, [], p_pcm=0.2, patch=lambda recs, mvs16: recs[n // 2:, 5].fill(0))
    if kind == "intra-all":
        return build_job(lib, rng, w, h, 0, 4, [], p_pcm=0.2, patch=_all_filtered(w))
    if kind == "empty-list":       # any_deblock on, every macroblock proved strength-free: one zero-motion copy stretch from one slot
        return build_job(lib, rng, w, h, 3, 4, [0, 1, 2], p_inter=1.0, p_pcm=0.0, patch=jobgen.patch_copy_runs(w, whole_picture=0))
    kw = dict(p_inter=0.6) if kind.startswith("p06") else dict(p_inter=0.97, mv_range=64)
    if kind.endswith("typed"):
        kw.update(patch=jobgen.patch_typed(rng))
    elif kind.endswith("typed-all"):                               # typed partitions, every macroblock filtered on every edge it has
        typed, every = jobgen.patch_typed(rng), _all_filtered(w)
        kw.update(patch=lambda recs, mvs16: (typed(recs, mvs16), every(recs, mvs16)))
    elif kind.endswith("sub8x8"):
        kw.update(patch=jobgen.patch_sub8x8(rng))
    elif kind.endswith("coherent"):
        kw.update(patch=jobgen.patch_coherent(rng, w), extra_blocks=n)
    return build_job(lib, rng, w, h, 3, 4, [0, 1, 2], **kw)


# the two pictures of a two-stream tick (20x12): list lengths that differ by more than one wavefront
MIXED = [(("intra-all", 20, 12), ("empty-list", 20, 12)), (("intra-all", 20, 12), HALF), (("p06-typed", 20, 12), HALF)]


# ------------------------------------------------------------------ without a GPU: the model's tables and the reach of the cases
def test_model_tables_are_the_kernels_tables():
    text = open(os.path.join(ROOT, "h264bsd_amd", "csrc", "kernels", "common.hip.h")).read()

    def table(name):
        body = re.search(r"__constant__ uint8_t " + name + r"\[52\](?:\[4\])? = \{(.*?)\};", text, flags=re.S).group(1)
        return [int(v) for v in re.findall(r"\d+", body)]

    assert table("c_alpha") == model.ALPHA.tolist()
    assert table("c_beta") == model.BETA.tolist()
    assert np.array(table("c_tc0")).reshape(52, 4)[:, :3].tolist() == model.TC0.tolist()
    assert table("c_qpc") == model.QPC.tolist()


def test_cases_reach_the_list_lengths_they_are_for(built):
    lengths = {(w, h): built.job_header(job_of("intra-all", w, h))["n_dbk"] for (w, h) in SIZES}
    assert lengths == {(1, 1): 1, (1, 9): 9, (9, 1): 9, (8, 8): 64, (13, 5): 65, (9, 7): 63, (20, 12): 240, (33, 16): 528}
    assert built.job_header(job_of("p06-typed-all", *BIG))["n_dbk"] > 512          # partitioned macroblocks in the second workgroup too
    for (w, h) in SIZES[:-1]:
        head = built.job_header(job_of("empty-list", w, h))
        assert head["n_dbk"] == 0 and head["any_deblock"] == 1, (w, h, head["n_dbk"], head["any_deblock"])
    for a, b in MIXED:
        na, nb = built.job_header(job_of(*a))["n_dbk"], built.job_header(job_of(*b))["n_dbk"]
        assert abs(na - nb) > 64, (a, na, b, nb)
    # the P pictures list partitioned macroblocks next to one-vector ones, and macroblocks that are not filtered
    job = job_of("p06-typed", 20, 12)
    exp = model.expected(job)
    recs = np.frombuffer(job, dtype=np.uint8, count=240 * 32, offset=built.job_header(job)["rec_off"]).reshape(240, 32)
    inter = exp["listed"] & (recs[:, 0] == 0)
    assert (recs[inter, 4] & 0x40).any() and not (recs[inter, 4] & 0x40).all()
    assert (~exp["listed"]).any() and not (exp["listed"] & ~exp["filtered"]).any()
    cleared = model.expected(job_of("p06-typed-unfiltered", 20, 12))
    assert (cleared["listed"] & ~cleared["filtered"]).sum() >= 60 and (cleared["listed"] & cleared["filtered"]).sum() >= 120
    assert {int(v) for v in np.unique(exp["rec"][exp["listed"], :16] & 15)} == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_records_and_flags(built, case):
    job = job_of(*case)
    exp = model.expected(job)
    rep = built.Replay([job], n_streams=2)
    try:
        for s in range(2):
            rec, flag = rep.dbk_records(0, s)
            what = model.compare(exp, rec, flag)
            assert what is None, f"stream {s}: {what}"
    finally:
        rep.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", MIXED, ids=lambda p: case_id(p[0]) + "+" + case_id(p[1]))
def test_two_stream_tick_with_lists_of_different_lengths(built, pair):
    """stream 1 runs the other picture of the pair (a staggered set): the grid is sized by the longer list, the surplus workgroups and
    wavefronts of the shorter picture leave without touching its scratch"""
    jobs = [job_of(*pair[0]), job_of(*pair[1])]
    exps = [model.expected(j) for j in jobs]
    rep = built.Replay(jobs, n_streams=2, odd_offset=1)
    try:
        for tick in range(2):
            for s in range(2):
                rec, flag = rep.dbk_records(tick, s)
                what = model.compare(exps[(tick + s) % 2], rec, flag)
                assert what is None, f"tick {tick} stream {s}: {what}"
    finally:
        rep.close()


@pytest.mark.gpu
def test_pipeline_after_a_records_call(built):
    """h264bsdmiReplayDbkRecords leaves the scratch as k_frame_dbk does (flag bytes zero): the full pipeline behind it still
    produces the oracle's pictures"""
    from oracle import pyoracle
    from replay_compare import random_pipeline_jobs
    jobs = random_pipeline_jobs(built.lib(), 5, 9, 1)
    rep = built.Replay(jobs, n_streams=2)
    dpb = pyoracle.OracleDpb(jobs[0])
    try:
        for i, job in enumerate(jobs):
            exp = model.expected(job)
            rec, flag = rep.dbk_records(i, 1)
            assert model.compare(exp, rec, flag) is None
            rep.run(i, 1)
            want = dpb.decode(job)
            assert np.array_equal(rep.fetch(1, pyoracle.blob_header(job)["cur_slot"]), want), f"picture {i}"
    finally:
        rep.close()
