"""What the point model's host path hands to the engine, without a GPU: api.c's h264bsdmiOutputPointModel bound to the recording device
stand-in (tests/fuzz_asan/mock_engine.c) and to the recording table of the program itself, which has all three entries behind the last
member of JobSink (eng_sink_entries, to which api.c refers weakly), by a stand-alone C program (tests/fuzz_asan/point_model.c).  It drives
a fixed sequence of named calls over instances A and B (fed and popped), U (bound to the engine, never fed anything), O (on a sink whose
table has the first two members only), X (on a sink without a table) and G (capture mode) and prints what the entry was given.  The
drivers of the point matches and the cell shift initialise the first two members and the first member of the table: they are built and
run here as they stand, against the table that has grown.  Built with gcc, plain and with Address-, UB- and LeakSanitizer: host programs
on the CPU that are run directly (tests/host_program.py)."""
import shutil

import pytest

import host_program

PLAIN = " spec 0x1000 matches=0x2000 kept=0x3000 current=0x4000 K=64 model=1 tolerance=2 scale=0 inliers=2 zero=0,0,0"
SHIFT = " spec 0x1008 matches=0x2008 kept=0x3008 current=0x3008 K=1 model=0 tolerance=0 scale=0 inliers=1 zero=0,0,0"
GATED = " spec 0x6000 matches=0x2000 kept=0x3000 current=0x4000 K=256 model=1 tolerance=255 scale=4096 inliers=256 zero=0,0,0"
REFUSED = ["refused_spec_null", "refused_data_null", "refused_data_alignment", "refused_matches_null", "refused_matches_alignment",
           "refused_kept_points_null", "refused_kept_points_alignment", "refused_current_points_null", "refused_current_points_alignment",
           "refused_points_zero", "refused_points", "refused_model", "refused_tolerance", "refused_scale_low", "refused_scale_high",
           "refused_scale_for_translation", "refused_inliers_zero", "refused_inliers_one_for_similarity", "refused_inliers", "refused_zero_0",
           "refused_zero_1", "refused_zero_2", "refused_no_instances", "refused_instances_null", "refused_instance_null", "refused_repeated",
           "refused_records", "refused_capture", "refused_capture_first", "refused_capture_no_records", "refused_sink_without_entry",
           "refused_sink_without_entry_second", "refused_sink_without_table", "refused_sink_without_table_second"]

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order"""
    return host_program.records("point_model", str(tmp_path_factory.mktemp("point_model")), request.param)


def test_the_driver_ran_every_call(records):
    assert [p.split()[1] for p in records["pops"]] == ["A", "B"]
    assert set(REFUSED) <= set(records) and len(records) == 1 + 10 + len(REFUSED)
    assert not any(ln.startswith(("flow ", "matches ")) for rec in records.values() for ln in rec)          # the older members are never reached
    assert not any(ln.startswith(("keep ", "regions ", "shift ")) for rec in records.values() for ln in rec)      # nor any entry of the sink itself


def test_an_accepted_call_hands_over_the_first_sink_the_count_the_spec_and_the_stream(records):
    assert records["two_instances"] == ["rc=0", "model sink=0 records=2 stream=0x0", PLAIN]
    assert records["other_order_and_stream"] == ["rc=0", "model sink=0 records=300 stream=0x5000", PLAIN]      # B first: its sink
    assert records["translation_limits"][:2] == ["rc=0", "model sink=0 records=7 stream=0x0"]
    assert records["translation_limits"][2] == GATED.replace("model=1", "model=0").replace("scale=4096", "scale=0")
    assert records["scale_floor"] == ["rc=0", "model sink=0 records=1 stream=0x0", PLAIN.replace("scale=0", "scale=256")]


def test_an_instance_needs_no_picture_and_need_not_have_been_fed(records):
    assert records["never_fed"] == ["rc=0", "model sink=0 records=65535 stream=0x0", SHIFT]
    assert records["never_fed_first_of_three"] == ["rc=0", "model sink=0 records=1 stream=0x5000", GATED]


def test_no_records_calls_nothing(records):
    assert records["no_records"] == ["rc=0", "sink: not called"] and records["no_records_no_instances"] == ["rc=0", "sink: not called"]


def test_a_failing_entry_is_minus_two(records):
    assert records["entry_fails"] == ["rc=-2", "model sink=0 records=2 stream=0x0", PLAIN]
    assert records["entry_fails_with_stream"] == ["rc=-2", "model sink=0 records=2 stream=0x5000", GATED]


@pytest.mark.parametrize("name", REFUSED)
def test_refused_calls_call_no_entry(records, name):
    """every -1 of the header; a sink whose table lacks the third member and a sink without a table, first or second in the call"""
    assert records[name] == ["rc=-1", "sink: not called"]


@pytest.mark.parametrize("sanitize", host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def test_the_point_matches_driver_still_builds_and_passes_untouched(sanitize, tmp_path):
    """its table initialises the first two members: the third is NULL there, the program links as it stands and its calls go through"""
    recs = host_program.records("point_matches", str(tmp_path), sanitize)
    assert recs["a_has_both"][:2] == ["rc=0", "matches m=1 k=1 stream=0x0"] and recs["both_kept"][1] == "matches m=2 k=2 stream=0x0"
    assert recs["refused_sink_without_entry"][:2] == ["rc=-1", "sink: not called"]


@pytest.mark.parametrize("sanitize", host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def test_the_cell_shift_driver_still_builds_and_passes_untouched(sanitize, tmp_path):
    """its table initialises the first member only"""
    recs = host_program.records("cell_shift", str(tmp_path), sanitize)
    assert recs["a_has_both"][:2] == ["rc=0", "flow m=1 k=1 stream=0x0"] and recs["both_kept"][1] == "flow m=2 k=2 stream=0x0"
    assert recs["refused_sink_without_entry"][:2] == ["rc=-1", "sink: not called"]
