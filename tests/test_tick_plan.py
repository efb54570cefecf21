"""The band plan of the two per-picture kernels (h264bsd_amd/csrc/tick_plan.h, plan_bands) decides correctness, not only speed: a
picture with concealed macroblocks must stay in one band of k_frame_intra.  The header includes nothing from HIP, so the plan is
held here without a GPU: a small C++ program built with g++ runs it over a grid of tick shapes with a synthetic LDS need, and the
results must equal tests/golden/tick_plan_pins.json — recorded from the plan as launch_tick carried it before it was a function
of its own, by tests/golden/make_tick_plan_pins.py, which also holds the grid and the program."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264bsd_amd", "csrc")
_GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_tick_plan_pins", os.path.join(_GOLDEN, "make_tick_plan_pins.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

NEW_PLAN = """
#include "tick_plan.h"
static int run_plan(const TickShape &s, const TailConfig &tc, int which, uint32_t waves, size_t (*lds_bytes)(uint32_t, uint32_t, uint32_t),
                    bool may_shorten, BandPlan &bp)
{
    return plan_bands(s, tc, which, waves, lds_bytes, may_shorten, bp);
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return gen.run_driver(NEW_PLAN, str(tmp_path_factory.mktemp("tick_plan")), include_dirs=[CSRC])


def test_header_needs_no_hip():
    """tick_plan.h is built by a host compiler: the three standard headers and nothing else"""
    includes = re.findall(r"^\s*#\s*include\s*(\S+)", open(os.path.join(CSRC, "tick_plan.h")).read(), flags=re.M)
    assert sorted(includes) == ["<algorithm>", "<cstddef>", "<cstdint>"]


def test_grid_is_the_one_the_pins_were_taken_on():
    cases = gen.cases()
    pins = json.load(open(gen.PINS))
    assert pins["cases"] == len(pins["plans"]) == len(cases) == len(set(cases)) and pins["waves_asked"] == gen.WAVES
    for col, values in ((0, {0, 1}), (1, {1, 4, 32, 256}), (4, {1, 4, 8}), (5, {1, 4, 8}), (8, {0, 1}), (9, {320, 64})):
        assert {c[col] for c in cases} == values
    assert {(c[6], c[7]) for c in cases} == {(11, 9), (120, 68), (256, 135)}
    for n in (1, 4, 32, 256):
        assert {c[2] for c in cases if c[1] == n} == {0, n, 256} and {c[3] for c in cases if c[1] == n} == {0, 1, n}
    # the grid reaches every outcome: refusals, shed wavefronts, shortened bands
    assert any(p is None for p in pins["plans"]) and any(p and p[2] < gen.WAVES for p in pins["plans"])
    assert any(p and c[0] == 0 and p[0] > max(c[4], c[5]) for c, p in zip(cases, pins["plans"]))


def test_plan_equals_the_pins(plans):
    pins = json.load(open(gen.PINS))["plans"]
    wrong = [(c, got, want) for c, got, want in zip(gen.cases(), plans, pins) if got != want]
    assert not wrong, f"{len(wrong)} of {len(pins)} plans differ, the first: {wrong[0]}"


def test_whole_pictures_stay_in_one_band(plans):
    """intra_whole: k_frame_intra's rows-per-band cap covers the whole picture wherever the plan succeeds — whatever the other
    pictures of the tick want, and however little LDS is left (fewer wavefronts, never shorter bands)"""
    held = 0
    for (which, n, load, heavy, wl, wh, w, h, whole, budget), p in zip(gen.cases(), plans):
        if which == 1 and whole and p is not None:
            assert p[1] == h, ((which, n, load, heavy, wl, wh, w, h, whole, budget), p)
            held += 1
    assert held > 100
