"""What an ACCEPTED region shift hands to the engine and writes back, without a GPU: api.c's h264bsdmiOutputRegionShift bound to a
recording device stand-in (tests/fuzz_asan/mock_engine.c) by a stand-alone C program (tests/fuzz_asan/region_shift.c), which
drives a fixed sequence of named calls over two instances (A: 640x360 cropped out of 640x368 coded; B: 1920x1080 out of 1920x1088), one
on a sink without the region_shift entry (O) and one in capture mode, and prints what the sink was given and what the output arrays
hold afterwards.  Built with gcc, plain and with Address-, UB- and LeakSanitizer: a host program on the CPU that is run directly."""
import shutil

import pytest

import host_program

BLANK = dict(got="untouched", current="untouched", kept="untouched", picId="untouched", keptPicId="untouched")

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order"""
    return host_program.records("region_shift", str(tmp_path_factory.mktemp("region_shift")), request.param)


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec if ln and ln[0] != " " and "=" in ln and not ln.startswith(("rc=", "keep ", "shift ")))


def _slots(records):
    """slot of the pops in order: A (picId 100), B (200), O (400), A (101)"""
    return [int(ln.split("slot=")[1].split()[0]) for ln in records["pops"]]


def test_the_pops_are_what_the_calls_should_see(records):
    assert [p.split()[1] for p in records["pops"]] == ["A", "B", "O", "A"]
    assert [p.split("picId=")[1] for p in records["pops"]] == ["100", "200", "400", "101"]


def test_nothing_kept_means_no_sink(records):
    rec = records["nothing_kept"]
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="0,0", current="1,1", kept="0,0", picId="100,200", keptPicId="0,0")


def test_the_search_names_only_instances_with_both_pictures_and_hands_window_and_box(records):
    slot_a = _slots(records)[0]
    rec = records["a_has_both"]
    assert rec[:5] == ["rc=0", "shift m=1 k=1 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,640,360",
                       " spec 0x1000 radius=4 surface=1 crop=1 keep_after=0"]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["coded_frame"]
    assert rec[2:5] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", " reg 0 index=0 0,0,640,368",
                        " spec 0x1000 radius=0 surface=0 crop=0 keep_after=0"]
    rec = records["boxes_mixed_order"]                            # B, A: the boxes that name A (instance 1) are records 0 and 2, in order,
    assert rec[:5] == ["rc=0", "shift m=1 k=2 stream=0x5000", f" pic 1 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,64,64",
                       " reg 0 index=2 700,-10,4096,4096"]        # unclipped: the sink cuts them at the window it is handed
    assert _arrays(rec) == dict(got="1,0,1,0", current="1,1", kept="0,1", picId="200,100", keptPicId="0,100")
    rec = records["null_arrays"]
    assert rec[0] == "rc=0" and rec[1].startswith("shift m=1 k=1")
    assert _arrays(rec) == dict(got="1,0", current="null", kept="null", picId="null", keptPicId="null")


def test_a_side_of_4096_passes_and_4097_does_not(records):
    rec = records["side_4096"]
    assert rec[:2] == ["rc=0", "shift m=1 k=1 stream=0x0"] and " reg 0 index=0 0,0,4096,4096" in rec
    assert _arrays(rec) == dict(got="1", current="1", kept="1", picId="100", keptPicId="100")
    for name in ("refused_width", "refused_height"):
        assert records[name][:2] == ["rc=-1", "sink: not called"] and _arrays(records[name]) == {k: BLANK[k] for k in _arrays(records[name])}


def test_failed_calls_write_nothing_and_mark_nothing(records):
    rec = records["shift_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("shift m=1 k=1") and not any(ln.startswith("keep ") for ln in rec)
    assert _arrays(rec) == BLANK
    rec = records["keep_after_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("shift m=1 k=1") and "keep m=2 k=0 stream=0x0" in rec
    assert _arrays(rec) == BLANK
    assert _arrays(records["b_still_not_kept"]) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")


def test_keep_after_calls_the_keep_entry_behind_the_shift_entry_and_keeps_everyone(records):
    slot_a, slot_b = _slots(records)[:2]
    rec = records["keep_after"]
    assert rec[0] == "rc=0" and rec[1] == "shift m=1 k=1 stream=0x0"
    assert " spec 0x2000 radius=16 surface=0 crop=1 keep_after=1" in rec
    at = rec.index("keep m=2 k=0 stream=0x0")
    assert at > rec.index(" spec 0x2000 radius=16 surface=0 crop=1 keep_after=1")
    assert rec[at + 1:at + 3] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", f" pic 1 slot={slot_b} win=0,0,1920,1088 mr=0,0"]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["both_kept"]
    assert rec[1] == "shift m=2 k=2 stream=0x0" and f" pic 1 slot={slot_b} win=0,0,1920,1080 mr=0,0" in rec
    assert rec[4:6] == [" reg 0 index=0 0,0,640,360", " reg 1 index=1 0,0,1920,1080"]
    assert _arrays(rec) == dict(got="1,1", current="1,1", kept="1,1", picId="100,200", keptPicId="100,200")


@pytest.mark.parametrize("name", ["refused_radius", "refused_surface", "refused_crop", "refused_keep_after", "refused_alignment", "refused_width",
                                  "refused_height", "refused_repeated", "refused_capture", "refused_got_null", "refused_sink_without_entry"])
def test_refused_calls_call_no_sink_and_write_nothing(records, name):
    rec = records[name]
    assert rec[:2] == ["rc=-1", "sink: not called"]
    assert all(v in ("untouched", "null") for v in _arrays(rec).values()), rec


def test_a_sink_without_the_entry_still_keeps(records):
    rec = records["keep_other_sink"]
    assert rec[:2] == ["rc=0", "keep m=1 k=0 stream=0x0"] and _arrays(rec) == dict(kept="1", picId="400")


def test_the_kept_picture_outlives_decoding(records):
    slots = _slots(records)
    rec = records["a_not_current"]
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="0", current="0", kept="1", picId="0", keptPicId="100")
    rec = records["a_next_picture"]
    assert rec[1] == "shift m=1 k=1 stream=0x0" and rec[2] == f" pic 0 slot={slots[3]} win=0,0,640,360 mr=0,0"
    assert _arrays(rec) == dict(got="1", current="1", kept="1", picId="101", keptPicId="100")
