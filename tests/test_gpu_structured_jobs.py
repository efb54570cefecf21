"""GPU parity on the structured hand-built frame jobs (tests/test_structured_jobs.py: STRUCTURED_SET): kernels vs CPU oracle,
bit-exact.  What the random jobs of test_gpu_random_jobs.py never reach, on pictures of at most 19 x 2 macroblocks: macroblocks
with one vector per quadrant (k_recon_inter_lq), every partition type and the no_motion_edge rule of k_dbk, sub-8x8 partitions,
motion fields whose neighbours differ by 0, 3 and 4 quarter samples (the >= 4 of k_dbk and of fj_dbk_trivial), copy runs of every
length with and without displacement (k_copy's run body, its tail, row ends, borders), reference windows one sample inside, on and
one sample outside every picture border (lfast / cfast), and content on which the filter takes every one of its decisions.
tests/test_structured_jobs.py holds the set to that reach and pins the oracle to the compiled reference on the same jobs."""
import pytest

from replay_compare import run_and_compare, tail  # noqa: F401 (tail is a fixture)
from test_structured_jobs import BANDED, RECON_ONLY, STRUCTURED_SET, fixed_layout_sequence, recipe_id, sequence

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("recipe", STRUCTURED_SET, ids=recipe_id)
def test_structured_pictures_full_pipeline(built, recipe):
    run_and_compare(built, sequence(recipe), n_streams=2, stages=7)


@pytest.mark.parametrize("recipe", RECON_ONLY, ids=recipe_id)
def test_structured_pictures_reconstruction_only(built, recipe):
    """copy runs and window edges without the filter on top: a wrong sample stays where it was made"""
    run_and_compare(built, sequence(recipe), n_streams=2, stages=3)


@pytest.mark.parametrize("cfg", [(1, 1, 4, 1, 1, 4, 1 << 20), (2, 2, 2, 2, 2, 2, 1 << 20)], ids=["1row4waves", "2rows2waves"])
@pytest.mark.parametrize("recipe", BANDED, ids=recipe_id)
def test_structured_pictures_in_row_bands(built, tail, recipe, cfg):
    """coherent fields and typed partitions with the per-picture kernels split into bands of one and two macroblock rows"""
    tail(*cfg)
    run_and_compare(built, sequence(recipe), n_streams=2, stages=7)


def test_whole_picture_copy_runs(built):
    """3x7: the second picture is one zero-motion run of the whole picture from slot 0, the third the same from slot 1 with one coded
    macroblock in the middle"""
    run_and_compare(built, fixed_layout_sequence(), n_streams=2, stages=7)
