"""Finished frame jobs, byte for byte, without a GPU: what fj_finalize_ex and the ghost / redo / concealment code around it
(h264bsd_amd/csrc/hd_core.c) make of every fixture stream and of a set of hand-built jobs must equal tests/golden/job_pins.json,
recorded by tests/golden/make_job_pins.py from the commit before job finalisation was cut into steps.  The kernels are launched over
the lists of these jobs and nothing else, so equal bytes mean equal work for the device.

The set: the three bundled streams, every synth_configs.CONFIGS stream and every test_damaged_streams.NAMES stream, each captured
without and with copy elision; 33 jobs of tests/jobgen.build_job through h264bsdmiJobFinalize (dense vectors in front of the
coefficients, a layout the parser never produces) at 1x1 .. 11x9 macroblocks, three of them with copy runs on both sides of a row
end; five hand-made jobs that must be refused (no existing test asserts a refusal of h264bsdmiJobFinalize, so all five are here).
No final job of the set holds an FJ_MB_STALE record — test_the_set_reaches_the_paths_it_pins asserts that too, so it shows if a
stream ever does; none is invented here."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_job_pins", os.path.join(ROOT, "tests", "golden", "make_job_pins.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def got(built):
    """everything once: building the synthetic and damaged streams takes most of the time, the captures about 2 s"""
    return gen.collect(built)


@pytest.fixture(scope="module")
def pins():
    return json.load(open(gen.PINS))


def test_jobs_of_every_stream_equal_the_pins(got, pins):
    assert len(pins["streams"]) == len(got["streams"]) == 294 and list(pins["streams"]) == list(got["streams"])
    assert sum(n for n, _ in pins["streams"].values()) == 1512
    wrong = [name for name, pin in pins["streams"].items() if got["streams"][name] != pin]
    assert not wrong, f"the jobs of {len(wrong)} of {len(pins['streams'])} streams differ from the pins ({pins['recorded_from']}): {wrong[:8]}"


def test_hand_built_jobs_equal_the_pins(got, pins):
    assert len(pins["hand_built"]) == len(got["hand_built"]) >= 24
    assert {"1x1_intra", "2x1_mixed", "1x3_inter", "3x2_nodbk", "5x4_pcm", "5x4_runs", "11x9_intra", "11x9_nodbk"} <= set(pins["hand_built"])
    wrong = [name for name, pin in pins["hand_built"].items() if got["hand_built"][name] != pin]
    assert not wrong, f"{len(wrong)} of {len(pins['hand_built'])} hand-built jobs differ from the pins: {wrong}"


def test_malformed_jobs_are_refused(got):
    """each of the five is one edit away from a job that is accepted, so it is the check of its name that refuses it"""
    assert [what for what, _, _ in got["rejections"]] == gen.REJECTIONS and len(gen.REJECTIONS) == 5
    assert all(rc == -1 and ok == 0 for _, rc, ok in got["rejections"]), got["rejections"]


def test_the_set_reaches_the_paths_it_pins(got):
    """lower bounds: the counts of the set when the pins were recorded.  The error paths are counted over the bundled and damaged
    streams alone (229 streams, 558 jobs), whose figures they are: over all streams 153 jobs hold I_PCM and 337545 copies are elided"""
    s, bd = got["stats"], got["stats_bundled_damaged"]
    assert s["jobs"] == 1512 and s["stale"] == 0 and bd["jobs"] == 558
    assert s["ghost"] >= 162 and s["dbk_only"] >= 162                        # reconstruction-only and deblock-only jobs
    assert s["mvx"] >= 1026 and s["quad"] >= 857                             # a sparse-vector section, quadrant entries
    assert bd["conceal_i"] >= 20 and bd["conceal_i_dbk_only"] >= 6 and bd["max_conceal_i"] >= 30
    assert bd["conceal_p"] >= 17 and bd["phase2"] >= 9 and bd["ipcm"] >= 53
    assert bd["elided"] >= 337524                                            # copies that copy elision left out


def test_pins_are_compact(pins):
    assert os.path.getsize(gen.PINS) < 48 * 1024 and len(pins["recorded_from"]) >= 7
