"""What an ACCEPTED point matching hands to the engine and writes back, without a GPU: api.c's h264bsdmiOutputPointMatches bound to a
recording device stand-in (tests/fuzz_asan/mock_engine.c, and the recording table of the program itself with both entries behind the last
member of JobSink: eng_sink_entries, to which api.c refers weakly) by a stand-alone C program (tests/fuzz_asan/point_matches.c), which
drives a fixed sequence of named calls over two instances (A: 640x360 cropped out of 640x368 coded; B: 1920x1080 out of 1920x1088; O: as
A, on a sink whose table has the first member only; N: as A, on a sink that cannot keep pictures) and prints what the engine was given
and what the output arrays hold afterwards.  The driver of the cell shift (tests/fuzz_asan/cell_shift.c) initialises only the first
member of the table: it is built and run here as it stands, against the table that has grown.  Built with gcc, plain and with Address-,
UB- and LeakSanitizer: host programs on the CPU that are run directly (tests/host_program.py)."""
import shutil

import pytest

import host_program

PLAIN = " spec 0x1000 kept=0x2000 current=0x3000 K=64 distance=64 ratio=205 move=0 mutual=1 crop=1 keep_after=0 zero=0"
CHAIN = " spec 0x4000 kept=0x2008 current=0x3008 K=256 distance=256 ratio=256 move=65535 mutual=0 crop=1 keep_after=1 zero=0"
BLANK = dict(got="untouched", current="untouched", kept="untouched", picId="untouched", keptPicId="untouched")
REFUSED = ["refused_spec_null", "refused_data_null", "refused_data_alignment", "refused_kept_points_null", "refused_kept_points_alignment",
           "refused_current_points_null", "refused_current_points_alignment", "refused_points_zero", "refused_points", "refused_distance",
           "refused_ratio_zero", "refused_ratio", "refused_move", "refused_mutual", "refused_crop", "refused_keep_after", "refused_zero",
           "refused_repeated", "refused_capture", "refused_got_null", "refused_regions_count", "refused_side",
           "refused_stream_and_bad_region", "refused_sink_without_entry", "refused_sink_without_keep"]

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order"""
    return host_program.records("point_matches", str(tmp_path_factory.mktemp("point_matches")), request.param)


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec if ln and ln[0] != " " and "=" in ln and not ln.startswith(("rc=", "keep ", "matches ", "flow ")))


def _slots(records):
    """slot of the pops in order: A (picId 100), B, O, N, A (101)"""
    return [int(ln.split("slot=")[1].split()[0]) for ln in records["pops"]]


def test_the_driver_ran_every_call(records):
    assert [p.split()[1] for p in records["pops"]] == ["A", "B", "O", "N", "A"]
    assert "picId=100" in records["pops"][0] and "picId=200" in records["pops"][1] and "picId=101" in records["pops"][4]
    assert set(REFUSED) <= set(records) and len(records) == 1 + 12 + len(REFUSED) + 3
    assert not any(ln.startswith("flow ") for rec in records.values() for ln in rec)            # the first member is never reached


def test_only_instances_with_both_pictures_are_named(records):
    slot_a = _slots(records)[0]
    rec = records["nothing_kept"]
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="0,0", current="1,1", kept="0,0", picId="100,200", keptPicId="0,0")
    rec = records["a_has_both"]
    assert rec[:5] == ["rc=0", "matches m=1 k=1 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,640,360", PLAIN]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["coded_frame"]
    assert rec[2:5] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", " reg 0 index=0 0,0,640,368",
                        " spec 0x1008 kept=0x2000 current=0x2000 K=1 distance=0 ratio=1 move=1 mutual=0 crop=0 keep_after=0 zero=0"]
    rec = records["a_not_current"]
    assert rec[:2] == ["rc=0", "sink: not called"] and _arrays(rec) == dict(got="0", current="0", kept="1", picId="0", keptPicId="100")
    rec = records["a_next_picture"]
    assert rec[1] == "matches m=1 k=1 stream=0x0" and rec[2] == f" pic 0 slot={_slots(records)[4]} win=0,0,640,360 mr=0,0"
    assert _arrays(rec) == dict(got="1", current="1", kept="1", picId="101", keptPicId="100")


def test_explicit_regions_the_stream_and_null_arrays(records):
    slot_a = _slots(records)[0]
    rec = records["boxes_mixed_order"]          # B, A: B has nothing kept; the boxes that name A (instance 1) are 0 and 2, one with sides of 4096
    assert rec[:6] == ["rc=0", "matches m=1 k=2 stream=0x5000", f" pic 1 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,64,64",
                       " reg 0 index=2 700,-10,4096,4096", PLAIN]
    assert _arrays(rec) == dict(got="1,0,1,0", current="1,1", kept="0,1", picId="200,100", keptPicId="0,100")
    rec = records["null_arrays"]
    assert rec[0] == "rc=0" and rec[1].startswith("matches m=1 k=1")
    assert _arrays(rec) == dict(got="1,0", current="null", kept="null", picId="null", keptPicId="null")
    rec = records["no_regions"]
    assert rec[:2] == ["rc=0", "sink: not called"] and _arrays(rec)["got"] == "null"


def test_failed_calls_write_nothing_and_mark_nothing(records):
    rec = records["matches_fail"]
    assert rec[0] == "rc=-2" and rec[1].startswith("matches m=1 k=1") and CHAIN in rec and not any(ln.startswith("keep ") for ln in rec)
    assert _arrays(rec) == BLANK
    rec = records["keep_after_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("matches m=1 k=1") and "keep m=2 k=0 stream=0x0" in rec
    assert _arrays(rec) == BLANK
    assert _arrays(records["b_still_not_kept"]) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")


def test_keep_after_reports_what_the_matching_saw_and_keeps_everyone(records):
    slot_a, slot_b = _slots(records)[:2]
    rec = records["keep_after"]
    assert rec[0] == "rc=0" and rec[1] == "matches m=1 k=1 stream=0x0" and CHAIN in rec
    at = rec.index("keep m=2 k=0 stream=0x0")
    assert at > rec.index(CHAIN) and rec[at + 1:at + 3] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", f" pic 1 slot={slot_b} win=0,0,1920,1088 mr=0,0"]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["both_kept"]
    assert rec[1] == "matches m=2 k=2 stream=0x0" and f" pic 1 slot={slot_b} win=0,0,1920,1080 mr=0,0" in rec and PLAIN in rec
    assert _arrays(rec) == dict(got="1,1", current="1,1", kept="1,1", picId="100,200", keptPicId="100,200")


@pytest.mark.parametrize("name", REFUSED)
def test_refused_calls_call_no_sink_and_write_nothing(records, name):
    """every -1 of the header, a sink whose table lacks the entry (which is not called, though it has a kept picture) and one that
    cannot keep"""
    rec = records[name]
    assert rec[:2] == ["rc=-1", "sink: not called"]
    assert all(v in ("untouched", "null") for v in _arrays(rec).values()), rec


def test_the_other_sink_keeps_but_is_never_asked_to_match(records):
    rec = records["keep_other_sink"]
    assert rec[0] == "rc=0" and rec[1].startswith("keep m=1") and _arrays(rec) == dict(kept="1", picId="400")


@pytest.mark.parametrize("sanitize", host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def test_the_cell_shift_driver_still_builds_and_passes_untouched(sanitize, tmp_path):
    """its table initialises the first member only: the second is NULL there, the program links as it stands and its calls go through"""
    recs = host_program.records("cell_shift", str(tmp_path), sanitize)
    assert recs["a_has_both"][:2] == ["rc=0", "flow m=1 k=1 stream=0x0"] and recs["both_kept"][1] == "flow m=2 k=2 stream=0x0"
    assert recs["refused_sink_without_entry"][:2] == ["rc=-1", "sink: not called"]


@pytest.mark.parametrize("sanitize", host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def test_an_engine_without_the_table_is_refused_and_not_called(sanitize, tmp_path):
    """the stand-in as every older driver links it: no eng_sink_entries at all (tests/fuzz_asan/point_matches_absent.c)"""
    recs = host_program.records("point_matches_absent", str(tmp_path), sanitize)
    rec = recs["refused_engine_without_entry"]
    assert rec[:2] == ["rc=-1", "sink: not called"] and _arrays(rec) == BLANK
    rec = recs["sibling_goes_on"]
    assert rec[0] == "rc=0" and rec[1].startswith("shift m=1 k=1") and _arrays(rec)["got"] == "1" and _arrays(rec)["kept"] == "1"
