"""What the host path of the warped kept pictures hands to the engine, without a GPU: api.c's h264bsdmiWarpKeptPictures bound to the
recording device stand-in (tests/fuzz_asan/mock_engine.c, unchanged) and to the recording table of the program itself, which has all four
entries behind the last member of JobSink (eng_sink_entries, to which api.c refers weakly), by a stand-alone C program
(tests/fuzz_asan/warp_kept.c).  It drives a fixed sequence of named calls over instances A (640x360 in a coded 640x368) and B (1920x1080 in
1920x1088), both fed, popped and kept, C (bound to the engine, never fed anything), O (on a sink whose table has the first three members
only), X (on a sink without a table) and G (capture mode) and prints what the entry was given and what the call wrote.  The drivers of the
point model, the point matches and the cell shift initialise the first three, two and one members of the table: they are built and run
here as they stand, against the table that has grown.  Built with gcc, plain and with Address-, UB- and LeakSanitizer: host programs on
the CPU that are run directly (tests/host_program.py)."""
import shutil

import pytest

import host_program

TOP = 16 * 65536
MAP_A = "map=65536,0,327680,0,65536,-196608"
MAP_B = f"map={TOP},{-TOP},2147483647,{-TOP},{TOP},-2147483648"
MAP_C = "map=1,2,3,4,5,6"
PLAIN = " spec the caller's outside=0 crop=0 count=0x0"
CROPPED = " spec the caller's outside=1 crop=1 count=0x3000"
UNTOUCHED = ["warped=untouched", "keptPicId=untouched"]
REFUSED = ["refused_spec_null", "refused_maps_null", "refused_outside", "refused_crop", "refused_a_high", "refused_a_low", "refused_b_high",
           "refused_b_low", "refused_d_high", "refused_d_low", "refused_e_high", "refused_e_low", "refused_instances_null", "refused_instance_null",
           "refused_warped_null", "refused_repeated", "refused_capture", "refused_capture_first", "refused_sink_without_entry",
           "refused_sink_without_entry_second", "refused_sink_without_table", "refused_sink_without_table_second"]

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order"""
    return host_program.records("warp_kept", str(tmp_path_factory.mktemp("warp_kept")), request.param)


def test_the_driver_ran_every_call(records):
    assert [p.split()[1] for p in records["pops"]] == ["A", "B"]
    assert set(REFUSED) <= set(records) and len(records) == 1 + 12 + len(REFUSED)
    assert records["keep_ab"][-2:] == ["kept=1,1", "picId=100,200"]
    assert not any(ln.startswith(("flow ", "matches ", "model ")) for rec in records.values() for ln in rec)        # the older members are never reached
    entries = [ln.split()[0] for name, rec in records.items() if name not in ("pops", "keep_ab") for ln in rec if not ln.startswith((" ", "rc=", "warped=", "keptPicId=", "sink:"))]
    assert set(entries) == {"warp"}                                                                               # nor any entry of the sink itself


def test_nothing_kept_and_nothing_to_do_call_nothing(records):
    assert records["nothing_kept"] == ["rc=0", "sink: not called", "warped=0,0,0", "keptPicId=0,0,0"]
    assert records["nothing_to_do"] == ["rc=0", "sink: not called"] + UNTOUCHED


def test_an_accepted_call_hands_over_pictures_maps_the_spec_and_the_stream(records):
    """one picture per instance that has a kept picture: its place in the call, its window (the coded frame, or the cropping window), its
    map verbatim beside it; count words for every instance of the call"""
    assert records["replicate_coded_frame"] == ["rc=0", "warp m=2 n_count=3 stream=0x0", f" pic 0 slot=3 index=0 win=0,0,640,368 {MAP_A}",
                                                f" pic 1 slot=3 index=1 win=0,0,1920,1088 {MAP_B}", PLAIN, "warped=1,1,0", "keptPicId=100,200,0"]
    assert records["current_cropped_with_stream"] == ["rc=0", "warp m=2 n_count=3 stream=0x5000", f" pic 0 slot=3 index=0 win=0,0,640,360 {MAP_A}",
                                                      f" pic 1 slot=3 index=1 win=0,0,1920,1080 {MAP_B}", CROPPED, "warped=1,1,0", "keptPicId=100,200,0"]
    assert records["other_order"] == ["rc=0", "warp m=2 n_count=3 stream=0x5000", f" pic 1 slot=3 index=1 win=0,0,1920,1088 {MAP_B}",
                                      f" pic 2 slot=3 index=2 win=0,0,640,368 {MAP_C}", PLAIN, "warped=0,1,1", "keptPicId=0,200,100"]
    assert records["optional_kept_pic_id"][-2:] == ["warped=1,1", "keptPicId=null"] and records["optional_kept_pic_id"][1] == "warp m=2 n_count=2 stream=0x0"


def test_a_failing_entry_is_minus_two_and_writes_nothing(records):
    assert records["entry_fails"][:2] == ["rc=-2", "warp m=2 n_count=3 stream=0x0"] and records["entry_fails"][4:] == [CROPPED] + UNTOUCHED
    assert records["entry_fails_with_stream"][:2] == ["rc=-2", "warp m=2 n_count=2 stream=0x5000"] and records["entry_fails_with_stream"][4:] == [PLAIN] + UNTOUCHED


def test_only_the_current_mode_needs_a_current_picture(records):
    """A has decoded on and shown nothing: REPLICATE warps its kept picture all the same (no frame buffer is named: slot 0), CURRENT leaves
    it alone and says so; the kept picId never changes"""
    rec = records["replicate_without_a_current_picture"]
    assert rec[:3] == ["rc=0", "warp m=2 n_count=3 stream=0x0", f" pic 0 slot=0 index=0 win=0,0,640,368 {MAP_A}"] and rec[-2:] == ["warped=1,1,0", "keptPicId=100,200,0"]
    assert records["current_without_a_current_picture"] == ["rc=0", "warp m=1 n_count=3 stream=0x0", f" pic 1 slot=3 index=1 win=0,0,1920,1080 {MAP_B}",
                                                            CROPPED, "warped=0,1,0", "keptPicId=100,200,0"]
    rec = records["current_again"]
    assert rec[1] == "warp m=2 n_count=3 stream=0x0" and rec[2].startswith(" pic 0 slot=") and rec[-2:] == ["warped=1,1,0", "keptPicId=100,200,0"]


@pytest.mark.parametrize("name", REFUSED)
def test_refused_calls_call_no_entry_and_write_nothing(records, name):
    """every -1 of the header — a coefficient out of range even in the map of an instance that would be left alone —, a sink whose table
    lacks the fourth member and a sink without a table, first or second in the call"""
    assert records[name] == ["rc=-1", "sink: not called", "warped=null" if name == "refused_warped_null" else "warped=untouched", "keptPicId=untouched"]


@pytest.mark.parametrize("driver, call, line", [("point_model", "two_instances", "model sink=0 records=2 stream=0x0"),
                                                ("point_matches", "a_has_both", "matches m=1 k=1 stream=0x0"),
                                                ("cell_shift", "a_has_both", "flow m=1 k=1 stream=0x0")])
@pytest.mark.parametrize("sanitize", host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def test_the_older_drivers_still_build_and_pass_untouched(sanitize, driver, call, line, tmp_path):
    """their tables initialise the first three, two and one members: the fourth is NULL there, the programs link as they stand and their
    calls go through"""
    recs = host_program.records(driver, str(tmp_path), sanitize)
    assert recs[call][:2] == ["rc=0", line]
    assert recs["refused_sink_without_entry"][:2] == ["rc=-1", "sink: not called"]
