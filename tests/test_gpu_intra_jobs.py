"""GPU parity on hand-built frame jobs of chosen intra macroblocks (tests/test_intra_jobs.py: INTRA_SET — every Intra4x4 / Intra16x16 /
chroma cell, the above-right rule of block 5, both roundings of the DC scalings, the RAW luma DC, residuals at both ends of their range,
both clips; held to its reach on the CPU): k_frame_intra against the CPU oracle, bit-exact, on both Intra4x4 paths (one macroblock per
wavefront, up to four in 16-lane groups), in one workgroup and with a band per macroblock row.  The oracle itself is pinned there to a
plain integer model, and in tests/test_oracle_stage_pins.py to the compiled reference's prediction functions.
No case may trip a wire of the kernels: the residuals stay inside [-512, 511] by construction."""
import numpy as np
import pytest

from oracle import pyoracle
from jobgen import build_job
import jobgen
from replay_compare import run_and_compare as _run, tail  # noqa: F401 (tail is a fixture)
import test_intra_jobs as T
from test_intra_jobs import BANDED, ENUMERATED, INTRA_SET, SCHEDULING, _seed, recipe_id, sequence

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    """device_errors() are sticky bits of the process (other files' jobs set some on purpose): none may be added, and the event
    counter must stand still"""
    bits, events = built.device_errors(), built.device_error_events()
    yield
    assert built.device_errors() == bits and built.device_error_events() == events, "a tripwire of the kernels fired"


@pytest.mark.parametrize("stages", [3, 7], ids=["recon", "filtered"])
@pytest.mark.parametrize("recipe", INTRA_SET, ids=recipe_id)
def test_intra_pictures(built, recipe, stages):
    """stages 3: reconstruction only, a wrong sample stays where it was made; 7: through the deblocking filter"""
    _run(built, sequence(recipe), n_streams=2, stages=stages)


@pytest.mark.parametrize("waves", [1, 4, 12])
@pytest.mark.parametrize("recipe", SCHEDULING + ENUMERATED, ids=recipe_id)
def test_intra_pictures_with_one_four_and_twelve_wavefronts(built, tail, recipe, waves):
    """one workgroup per picture.  Which Intra4x4 path the scheduling recipes take at each setting:
    tests/test_intra_jobs.py::test_which_path_the_scheduling_recipes_take"""
    tail(0, 0, waves, 0, 0, waves, 1 << 20)
    _run(built, sequence(recipe), n_streams=2, stages=3)


def _light_p_picture(built, rng, w, h):
    """a P picture (slot 1, from slot 0) with a few Intra4x4 macroblocks: light, so never split when intra_rows_light is 0"""
    chosen = {int(a): T.i4(rng, jobgen.natural_avail(int(a) % w, int(a) // w, w), p_coded=0.4) for a in rng.choice(w * h, max(2, w * h // 10), replace=False)}
    return build_job(built.lib(), rng, w, h, 1, 4, [0], p_inter=1.0, p_pcm=0.0, chosen=chosen, patch=T.no_inter_residual)


def _in_slot(job, slot):
    out = bytearray(job)
    out[16] = slot                                     # FjHeader.cur_slot
    return bytes(out)


def _compare_slots(rep, jobs):
    dpb = pyoracle.OracleDpb(jobs[0])
    want = {pyoracle.blob_header(job)["cur_slot"]: dpb.decode(job).copy() for job in jobs}
    assert len(want) == len(jobs)
    for s in range(2):
        for slot, wanted in want.items():
            got = rep.fetch(s, slot)
            assert np.array_equal(got, wanted), f"stream {s} slot {slot}: {np.count_nonzero(got != wanted)} bytes differ"


@pytest.mark.parametrize("waves", [1, 12])
@pytest.mark.parametrize("recipe", BANDED, ids=recipe_id)
def test_a_band_per_row_in_one_tick_with_a_picture_that_is_not_split(built, tail, recipe, waves):
    """Three pictures: an intra picture (slot 0), a light P picture that refers to it (slot 1: never split), the recipe's picture
    (slot 2).  Stream 1 starts two pictures ahead, so in tick 2 stream 0 runs the recipe's picture, one band per macroblock row (the
    hand-over between bands: done bytes, the poll over x += 64 and its seen words, loads past the L1), next to stream 1's P picture;
    in tick 0 it is stream 1 that runs it, next to the first intra picture."""
    w, h = recipe[2][-1]
    pictures = sequence(recipe)
    jobs = [pictures[0], _light_p_picture(built, np.random.default_rng(_seed(recipe) + 500), w, h), _in_slot(pictures[-1], 2)]
    tail(1, 1, waves, 0, 1, waves, 1 << 20)
    rep = built.Replay(jobs, n_streams=2, offsets=[0, 2])
    try:
        rep.run(0, 3)
        _compare_slots(rep, jobs)
    finally:
        rep.close()


@pytest.mark.parametrize("recipe", [r for r in INTRA_SET if r[1] in ("5x4-p", "11x6-p")], ids=recipe_id)
def test_a_heavy_and_a_light_picture_share_a_tick(built, recipe):
    """odd_offset = 1 on the recipe's intra picture and its first P picture, two laps: in the second lap the odd stream runs the P
    picture (by then from the right reference) in the tick in which the even stream runs the intra picture, and the other way round"""
    jobs = list(sequence(recipe)[:2])
    rep = built.Replay(jobs, n_streams=2, odd_offset=1)
    try:
        rep.run(0, 2)
        rep.run(0, 2)
        _compare_slots(rep, jobs)
    finally:
        rep.close()
