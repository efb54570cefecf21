"""What the host path of the corner points refuses, and what an ACCEPTED call hands to the engine and writes back, without a GPU:
api.c's h264bsdmiOutputCornerPoints bound to a recording device stand-in (tests/fuzz_asan/mock_engine.c) by a stand-alone C
program (tests/fuzz_asan/corner_points.c), which drives a fixed sequence of named calls over two instances (A: 640x360 cropped out of
640x368 coded; B: 1920x1080 out of 1920x1088), one on a sink without the corner_points entry (O) and one in capture mode, and prints
what the sink was given and what the output arrays hold afterwards.  Built with gcc, plain and with Address-, UB- and LeakSanitizer: a
host program on the CPU that is run directly."""
import shutil

import pytest

import host_program

BLANK = dict(got="untouched", current="untouched", picId="untouched")
PLAIN = " spec 0x1000 score=0 block=3 nms=3 max_points=64 crop=1 zero=0 min_score=0"
REFUSED = ["refused_spec_null", "refused_data_null", "refused_alignment", "refused_score", "refused_block_0", "refused_block_4", "refused_block_7",
           "refused_nms_0", "refused_nms_8", "refused_points_0", "refused_points_257", "refused_crop", "refused_zero", "refused_harris_min_score",
           "refused_repeated", "refused_capture", "refused_got_null", "refused_dec_null", "refused_window_count", "refused_empty_region",
           "refused_far_region", "refused_huge_region", "refused_instance", "refused_sink_without_entry"]

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order"""
    return host_program.records("corner_points", str(tmp_path_factory.mktemp("corner_points")), request.param)


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec if ln and ln[0] != " " and "=" in ln and not ln.startswith(("rc=", "corners ")))


def _slots(records):
    """slot of the pops in order: A (picId 100), B (200), O (400), A (101)"""
    return [int(ln.split("slot=")[1].split()[0]) for ln in records["pops"]]


def test_the_program_made_every_call(records):
    assert [p.split()[1] for p in records["pops"]] == ["A", "B", "O", "A"]
    assert [p.split("picId=")[1] for p in records["pops"]] == ["100", "200", "400", "101"]
    assert set(REFUSED) <= set(records) and sum(k.startswith("refused_") for k in records) == len(REFUSED)


def test_whole_windows_hand_the_window_as_the_box_and_need_no_kept_picture(records):
    slot_a, slot_b = _slots(records)[:2]
    rec = records["whole_windows"]
    assert rec == ["rc=0", "corners m=2 k=2 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,360 mr=0,0", f" pic 1 slot={slot_b} win=0,0,1920,1080 mr=0,0",
                   " reg 0 index=0 0,0,640,360", " reg 1 index=1 0,0,1920,1080", PLAIN, "got=1,1", "current=1,1", "picId=100,200"]
    rec = records["coded_frame"]                                  # crop = 0, and every field of the spec at its largest reaches the sink
    assert rec[2:7] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", f" pic 1 slot={slot_b} win=0,0,1920,1088 mr=0,0", " reg 0 index=0 0,0,640,368",
                        " reg 1 index=1 0,0,1920,1088", " spec 0x1000 score=1 block=5 nms=7 max_points=256 crop=0 zero=0 min_score=9223372036854775807"]
    rec = records["least"]                                        # MIN_EIGEN takes any u64 as min_score
    assert rec[0] == "rc=0" and " spec 0x2008 score=0 block=5 nms=1 max_points=1 crop=1 zero=0 min_score=18446744073709551615" in rec


def test_boxes_keep_their_record_index_and_reach_the_sink_unclipped(records):
    slot_a, slot_b = _slots(records)[:2]
    rec = records["boxes_mixed_order"]                            # B, A in the call: pictures in the order of first use
    assert rec[:8] == ["rc=0", "corners m=2 k=4 stream=0x5000", f" pic 1 slot={slot_a} win=0,0,640,360 mr=0,0",
                       f" pic 0 slot={slot_b} win=0,0,1920,1080 mr=0,0", " reg 0 index=0 0,0,64,64", " reg 1 index=1 -5,7,100,30",
                       " reg 0 index=2 700,-10,16384,16384", " reg 1 index=3 0,0,640,360"]
    assert rec[8] == PLAIN
    assert _arrays(rec) == dict(got="1,1,1,1", current="1,1", picId="200,100")


def test_optional_arrays_and_no_regions(records):
    rec = records["null_arrays"]
    assert rec[0] == "rc=0" and rec[1] == "corners m=2 k=2 stream=0x0"
    assert _arrays(rec) == dict(got="1,1", current="null", picId="null")
    rec = records["no_regions"]                                   # returns 0, calls nothing, reports the instances all the same
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="null", current="1,1", picId="100,200")


def test_a_failed_engine_writes_nothing(records):
    rec = records["engine_fails"]
    assert rec[0] == "rc=-2" and rec[1] == "corners m=2 k=2 stream=0x0" and PLAIN in rec
    assert _arrays(rec) == BLANK


@pytest.mark.parametrize("name", REFUSED)
def test_refused_calls_call_no_sink_and_write_nothing(records, name):
    rec = records[name]
    assert rec[:2] == ["rc=-1", "sink: not called"]
    assert all(v in ("untouched", "null") for v in _arrays(rec).values()) and len(_arrays(rec)) == 3, rec


def test_an_instance_without_a_current_picture_is_left_out(records):
    slots = _slots(records)
    rec = records["a_not_current"]
    assert rec[:4] == ["rc=0", "corners m=1 k=1 stream=0x0", f" pic 1 slot={slots[1]} win=0,0,1920,1080 mr=0,0", " reg 0 index=1 0,0,1920,1080"]
    assert _arrays(rec) == dict(got="0,1", current="0,1", picId="0,200")
    rec = records["a_next_picture"]
    assert rec[1] == "corners m=1 k=1 stream=0x0" and rec[2] == f" pic 0 slot={slots[3]} win=0,0,640,360 mr=0,0"
    assert _arrays(rec) == dict(got="1", current="1", picId="101")
