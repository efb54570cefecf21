"""What an ACCEPTED keep or comparison hands to the engine and writes back, without a GPU: api.c's h264bsdmiKeepCurrentPictures and
h264bsdmiOutputRegionChange bound to a recording device stand-in (tests/fuzz_asan/mock_engine.c) by a stand-alone C program
(tests/fuzz_asan/keep_change.c), which drives a fixed sequence of named calls over two instances (A: 640x360 cropped out of 640x368
coded; B: 1920x1080 out of 1920x1088) and prints what the sink was given and what the output arrays hold afterwards.  Built with gcc,
plain and with Address-, UB- and LeakSanitizer: a host program on the CPU that is run directly."""
import shutil

import pytest

import host_program

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order; "final": the lines behind #final"""
    return host_program.records("keep_change", str(tmp_path_factory.mktemp("keep_change")), request.param)


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec if ln and ln[0] != " " and "=" in ln and not ln.startswith(("rc=", "keep ", "change ")))


def _slots(records):
    """slot of the pops in order: A (picId 100), B, T, A (101), A (the other stream)"""
    return [int(ln.split("slot=")[1].split()[0]) for ln in records["pops"]]


def test_the_pops_are_what_the_calls_should_see(records):
    pops = records["pops"]
    assert [p.split()[1] for p in pops] == ["A", "B", "T", "A", "A"]
    assert "picId=100 size=40x23 configured=1" in pops[0] and "picId=200 size=120x68" in pops[1] and "picId=101" in pops[3]
    assert "size=120x68 configured=2" in pops[4]                   # A was configured again, for the other size


def test_nothing_kept_means_no_sink_and_a_failed_keep_marks_nothing(records):
    for name in ("nothing_kept", "still_nothing_kept"):
        assert records[name][:2] == ["rc=0", "sink: not called"]
        assert _arrays(records[name]) == dict(got="0,0", current="1,0", kept="0,0", picId="100,0", keptPicId="0,0")
    rec = records["keep_fails"]
    assert rec[0] == "rc=-2" and rec[1] == "keep m=1 k=0 stream=0x0"
    assert _arrays(rec) == dict(kept="untouched", picId="untouched")


def test_keep_hands_whole_coded_frames_of_the_instances_with_a_picture(records):
    slot_a = _slots(records)[0]
    rec = records["keep_a_only"]
    assert rec[:3] == ["rc=0", "keep m=1 k=0 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0"]
    assert _arrays(rec) == dict(kept="1,0", picId="100,0")


def test_the_comparison_names_only_instances_with_both_pictures(records):
    slot_a, slot_b = _slots(records)[:2]
    rec = records["a_has_both"]
    assert rec[:5] == ["rc=0", "change m=1 k=1 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,640,360",
                       " spec 0x1000 source=1 bins=256 crop=1 thr=3,2,1 keep_after=0"]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["coded_frame"]
    assert rec[2:4] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", " reg 0 index=0 0,0,640,368"]
    assert " crop=0 " in rec[4]
    rec = records["boxes_mixed_order"]                            # B, A: the boxes that name A (instance 1) are records 0 and 2
    assert rec[:5] == ["rc=0", "change m=1 k=2 stream=0x5000", f" pic 1 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,64,64",
                       " reg 0 index=2 700,10,8,8"]
    assert _arrays(rec) == dict(got="1,0,1,0", current="1,1", kept="0,1", picId="200,100", keptPicId="0,100")
    rec = records["null_arrays"]
    assert rec[0] == "rc=0" and rec[1].startswith("change m=1 k=1")
    assert _arrays(rec) == dict(got="1,0", current="null", kept="null", picId="null", keptPicId="null")
    assert slot_b >= 0


def test_failed_calls_write_nothing_and_mark_nothing(records):
    blank = dict(got="untouched", current="untouched", kept="untouched", picId="untouched", keptPicId="untouched")
    rec = records["change_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("change m=1 k=1") and not any(ln.startswith("keep ") for ln in rec)
    assert _arrays(rec) == blank
    rec = records["keep_after_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("change m=1 k=1") and "keep m=2 k=0 stream=0x0" in rec
    assert _arrays(rec) == blank
    assert _arrays(records["b_still_not_kept"]) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")


def test_keep_after_reports_what_the_comparison_saw_and_keeps_everyone(records):
    slot_a, slot_b = _slots(records)[:2]
    rec = records["keep_after"]
    assert rec[0] == "rc=0" and rec[1] == "change m=1 k=1 stream=0x0"
    assert " spec 0x2000 source=2 bins=16 crop=1 thr=0,0,255 keep_after=1" in rec
    at = rec.index("keep m=2 k=0 stream=0x0")
    assert at > 1 and rec[at + 1:at + 3] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", f" pic 1 slot={slot_b} win=0,0,1920,1088 mr=0,0"]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["both_kept"]
    assert rec[1] == "change m=2 k=2 stream=0x0" and f" pic 1 slot={slot_b} win=0,0,1920,1080 mr=0,0" in rec
    assert " reg 1 index=1 0,0,1920,1080" in rec
    assert _arrays(rec) == dict(got="1,1", current="1,1", kept="1,1", picId="100,200", keptPicId="100,200")
    assert _arrays(records["keep_null_ids"]) == dict(kept="1,1", picId="null")


@pytest.mark.parametrize("name", ["refused_repeated", "refused_capture", "refused_threshold", "refused_got_null"])
def test_refused_comparisons_call_no_sink_and_write_nothing(records, name):
    rec = records[name]
    assert rec[:2] == ["rc=-1", "sink: not called"]
    assert all(v in ("untouched", "null") for v in _arrays(rec).values()), rec


@pytest.mark.parametrize("name", ["refused_keep_repeated", "refused_keep_capture", "refused_keep_null"])
def test_refused_keeps_call_no_sink_and_write_nothing(records, name):
    rec = records[name]
    assert rec[:2] == ["rc=-1", "sink: not called"]
    assert all(v in ("untouched", "null") for v in _arrays(rec).values()), rec


def test_the_kept_picture_outlives_decoding_and_a_keep_without_a_picture(records):
    slots = _slots(records)
    rec = records["a_not_current"]
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="0", current="0", kept="1", picId="0", keptPicId="100")
    rec = records["keep_without_current"]
    assert rec[:2] == ["rc=0", "sink: not called"] and _arrays(rec) == dict(kept="0", picId="100")
    rec = records["a_next_picture"]
    assert rec[1] == "change m=1 k=1 stream=0x0" and rec[2] == f" pic 0 slot={slots[3]} win=0,0,640,360 mr=0,0"
    assert _arrays(rec) == dict(got="1", current="1", kept="1", picId="101", keptPicId="100")


def test_a_sequence_of_another_size_drops_the_kept_picture(records):
    slots = _slots(records)
    rec = records["other_size"]
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="0", current="1", kept="0", picId="102", keptPicId="0")
    rec = records["keep_other_size"]
    assert rec[1:3] == ["keep m=1 k=0 stream=0x0", f" pic 0 slot={slots[4]} win=0,0,1920,1088 mr=0,0"]
    assert _arrays(rec) == dict(kept="1", picId="102")
    rec = records["other_size_kept"]
    assert rec[1] == "change m=1 k=1 stream=0x0" and _arrays(rec) == dict(got="1", current="1", kept="1", picId="102", keptPicId="102")


def test_the_twins_output_queue_is_untouched(records):
    final = records["final"]
    assert "twin=1" in final and final[0].split("=")[1] == final[1].split("=")[1]
