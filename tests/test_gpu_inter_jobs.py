"""GPU parity on hand-built frame jobs of chosen inter macroblocks (tests/test_inter_jobs.py: INTER_SET — reference pictures of chosen samples
under every fraction, the exact ends of the interpolation sums, every chroma fraction; level blocks on the 16-bit bound of the packed residual
at every qp_y and qp_c, chroma DC at its bound, macroblocks that fail the bound in range; held to its reach on the CPU): the three inter kernels
(k_recon_inter_lb, k_recon_inter_lq, k_recon_inter — every recipe puts all macroblocks of its P pictures into one of their lists) against the CPU
oracle, byte for byte.  The oracle itself is pinned there to a plain integer model, and in tests/test_oracle_vs_ref.py to the compiled reference.
Pictures are 2 x 2 (residual cases: one group of four), 3 x 2 (windows) and 11 x 6 (the 64 chroma fractions).
No recipe may trip a wire of the kernels but those of the family `over`, whose every macroblock holds one residual sample of 512: there the
range wire must fire."""
import pytest

from replay_compare import run_and_compare
from test_inter_jobs import FAMILIES, INTER_SET, recipe_id, sequence

pytestmark = pytest.mark.gpu

ALL_STAGES = [[r for r in INTER_SET if r[0] == family][k % 3] for k, family in enumerate(FAMILIES)]      # one recipe per family, the lists in turn


def _run(built, recipe, stages):
    """device_errors() are sticky bits of the process (other files' jobs set some on purpose): none may be added and the event counter must
    stand still — but in `over`, where it must move"""
    bits, events = built.device_errors(), built.device_error_events()
    run_and_compare(built, sequence(recipe), n_streams=2, stages=stages)
    if recipe[0] == "over":
        assert built.device_error_events() > events, "a residual sample of 512 went unnoticed"
    else:
        assert built.device_errors() == bits and built.device_error_events() == events, "a tripwire of the kernels fired"


@pytest.mark.parametrize("recipe", INTER_SET, ids=recipe_id)
def test_inter_pictures(built, recipe):
    """reconstruction only: a wrong sample stays where it was made"""
    _run(built, recipe, 3)


@pytest.mark.parametrize("recipe", ALL_STAGES, ids=recipe_id)
def test_inter_pictures_through_the_filter(built, recipe):
    _run(built, recipe, 7)
