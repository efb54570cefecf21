"""GPU parity on hand-built frame jobs with concealed macroblocks (tests/test_concealed_jobs.py: CONCEALED_SET — every neighbour
mask, every position, every case of the concealment arithmetic, held to its reach on the CPU): conceal_mb and the dataflow schedule
of k_frame_intra, the copies of k_copy and the filtering of concealed macroblocks against the CPU oracle, bit-exact.  The oracle
itself is pinned there to a plain integer model and, through streams that lose the same macroblocks, to the compiled reference."""
import struct

import numpy as np
import pytest

from oracle import pyoracle
from jobgen import build_job
from replay_compare import run_and_compare as _run, tail  # noqa: F401 (tail is a fixture)
from test_concealed_jobs import BIG_SET, CONCEALED_SET, STREAMED, huge_job, recipe_id, sequence, stream_of

pytestmark = pytest.mark.gpu

BAND_PER_ROW = [(1, 1, 4, 1, 1, 4, 1 << 20), (2, 2, 2, 2, 2, 2, 1 << 20)]
INTRA_BIG = [r for r in BIG_SET if not r[4].startswith("p_")]


@pytest.mark.parametrize("stages", [3, 7], ids=["recon", "filtered"])
@pytest.mark.parametrize("recipe", CONCEALED_SET, ids=recipe_id)
def test_concealed_pictures(built, recipe, stages):
    """stages 3: reconstruction only, a wrong sample stays where it was made; 7: concealed macroblocks are filtered as intra at
    QP 40 on every edge"""
    _run(built, sequence(recipe), n_streams=2, stages=stages)


@pytest.mark.parametrize("cfg", BAND_PER_ROW, ids=["1row-4waves", "2rows-2waves"])
@pytest.mark.parametrize("recipe", BIG_SET, ids=recipe_id)
def test_concealed_pictures_when_a_band_per_row_is_asked_for(built, tail, recipe, cfg):
    """FjHeader.intra_down_deps keeps the picture in one band of k_frame_intra whatever the configuration wants"""
    tail(*cfg)
    _run(built, sequence(recipe), n_streams=2)


@pytest.mark.parametrize("cfg", BAND_PER_ROW, ids=["1row-4waves", "2rows-2waves"])
@pytest.mark.parametrize("recipe", INTRA_BIG, ids=recipe_id)
def test_concealed_picture_in_one_tick_with_a_banded_intact_picture(built, tail, recipe, cfg):
    """the regression of test_concealed_picture_next_to_a_banded_heavy_picture (tests/test_gpu_random_jobs.py) on chosen masks: the
    tick's rows-per-band cap must cover the concealed picture although the intact one next to it is split"""
    _fam, w, h = recipe[:3]
    conc = sequence(recipe)[-1]
    assert struct.unpack_from("<I", conc, 96)[0] == 1 and pyoracle.blob_header(conc)["n_intra_levels"] > 0
    intact = build_job(built.lib(), np.random.default_rng(recipe[6] + 1), w, h, 1, 4, [])
    want = {pyoracle.blob_header(job)["cur_slot"]: pyoracle.OracleDpb(job).decode(job).copy() for job in (conc, intact)}
    tail(*cfg)
    rep = built.Replay([intact, conc], n_streams=2, offsets=[0, 1])
    try:
        rep.run(0, 2)                                    # tick 0: stream 0 intact + stream 1 concealed; tick 1: the other way round
        for s in range(2):
            for slot, wanted in want.items():
                got = rep.fetch(s, slot)
                assert np.array_equal(got, wanted), f"stream {s} slot {slot}: {np.count_nonzero(got != wanted)} bytes differ"
    finally:
        rep.close()


@pytest.mark.parametrize("waves", [1, 12])
@pytest.mark.parametrize("recipe", BIG_SET, ids=recipe_id)
def test_concealed_pictures_with_one_and_twelve_wavefronts(built, tail, recipe, waves):
    """one workgroup per picture.  A wavefront claims up to four ready macroblocks: with one wavefront a group mixes concealed and
    intra macroblocks, with twelve the concealed macroblocks of one chain land in different wavefronts"""
    tail(0, 0, waves, 0, 0, waves, 1 << 20)
    _run(built, sequence(recipe), n_streams=2)


def test_huge_concealed_picture_in_one_band(built, tail):
    """256 x 144 macroblocks, the largest level-5.1 frame, the top eight rows and one macroblock in every 64 lost: the picture stays in
    one band, whose scheduling state fills the LDS next to two wavefronts (tests/test_tick_plan.py holds the plan to that on the
    CPU), although bands of 18 rows are asked for"""
    tail(36, 18, 4, 36, 18, 4, 1 << 20)
    job = huge_job()
    assert struct.unpack_from("<I", job, 96)[0] == 1 and pyoracle.blob_header(job)["n_intra_levels"] > 8, "no downward dependencies: the picture would be split"
    _run(built, [job], n_streams=1)


@pytest.mark.parametrize("recipe", STREAMED, ids=recipe_id)
def test_streams_that_lose_a_slice_group_through_the_product(built, recipe):
    import synth
    stream = stream_of(recipe)
    assert synth.decode_ours(stream, "gpu") == synth.decode_ours(stream, "oracle")
