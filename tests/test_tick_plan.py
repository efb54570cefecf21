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


LARGEST = r"""
#include <cstdio>
#include "tick_plan.h"
#define __host__
#define __device__
namespace h264k {
KERNEL_TEXT
}
int main()
{
    /* one tick: the concealed picture of 256 x 144 macroblocks alone, and next to an intact one that wants a band per row */
    for (unsigned n = 1; n <= 2; n++)
        for (unsigned rows_asked = 0; rows_asked <= 18; rows_asked += 1 + 16 * (rows_asked > 0)) {
            TickShape s;
            s.n_frames = n; s.n_heavy = n; s.max_w = 256; s.max_h = 144; s.intra_whole = true;
            s.want_heavy[1] = n == 1 || !rows_asked ? 1 : (144 + rows_asked - 1) / rows_asked;
            TailConfig tc;
            tc.band_budget = 1u << 20;
            BandPlan bp = {};
            if (plan_bands(s, tc, 1, WAVES, h264k::intra_lds_bytes, false, bp)) { printf("refused\n"); continue; }
            printf("%u %u %u %zu %zu %zu\n", bp.bands, bp.rows, bp.waves, bp.lds, h264k::intra_lds_bytes(bp.waves + 1, 256, bp.rows), (size_t)TAIL_LDS_BUDGET);
        }
    return 0;
}
"""


def test_largest_concealed_picture_is_one_band_next_to_two_wavefronts(tmp_path):
    """What tests/test_gpu_concealed_jobs.py::test_huge_concealed_picture_in_one_band runs must be what it says: with the kernel's own
    LDS need (intra_lds_bytes and its constants, taken from k_frame_intra.hip.h as they stand) a picture of 256 x 144 macroblocks
    that must stay whole is planned as bands of 144 rows — one per picture of the tick — with at most two wavefronts, because a third no longer
    fits next to the scheduling state; alone or next to an intact picture, whatever rows per band are asked for."""
    import subprocess
    text = open(os.path.join(CSRC, "kernels", "k_frame_intra.hip.h")).read()
    parts = [re.search(r"^constexpr int %s = [^;]*;" % name, text, flags=re.M).group(0) for name in ("I4TAB_BYTES", "INTRA_SLOT", "INTRA_WAVE_LDS")]
    parts.append(re.search(r"^__host__ __device__ inline size_t intra_lds_bytes\(.*?^}", text, flags=re.M | re.S).group(0))
    src, exe = str(tmp_path / "largest.cpp"), str(tmp_path / "largest")
    open(src, "w").write(LARGEST.replace("KERNEL_TEXT", "\n".join(parts)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-DWAVES={gen.WAVES}", f"-I{CSRC}", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[int(v) for v in line.split()] for line in out if line]
    assert len(rows) == 6
    for bands, rows_per_band, waves, lds, lds_one_more, budget in rows:
        assert rows_per_band == 144 and 1 <= waves <= 2 and lds <= budget < lds_one_more, (bands, rows_per_band, waves, lds, lds_one_more, budget)
    assert rows[0][0] == 1 and {r[0] for r in rows[:3]} == {1}, "alone, the picture is one workgroup"


def test_whole_pictures_stay_in_one_band(plans):
    """intra_whole: k_frame_intra's rows-per-band cap covers the whole picture wherever the plan succeeds — whatever the other
    pictures of the tick want, and however little LDS is left (fewer wavefronts, never shorter bands)"""
    held = 0
    for (which, n, load, heavy, wl, wh, w, h, whole, budget), p in zip(gen.cases(), plans):
        if which == 1 and whole and p is not None:
            assert p[1] == h, ((which, n, load, heavy, wl, wh, w, h, whole, budget), p)
            held += 1
    assert held > 100
