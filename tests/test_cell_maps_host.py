"""What an ACCEPTED cell-map call hands to the engine and writes back, without a GPU: api.c's h264bsdmiOutputCellMaps bound to a
recording device stand-in (tests/fuzz_asan/mock_engine.c) by a stand-alone C program (tests/fuzz_asan/cell_maps.c), which drives
a fixed sequence of named calls over two instances (A: 640x360 cropped out of 640x368 coded; B: 1920x1080 out of 1920x1088; N: as A, on
a sink that cannot keep pictures) and prints what the sink was given and what the output arrays hold afterwards.  Built with gcc, plain
and with Address-, UB- and LeakSanitizer: a host program on the CPU that is run directly (tests/host_program.py)."""
import shutil

import pytest

import host_program

PICTURE = " spec 0x1000 grid=23x40 cell=16 source=1 crop=1 mode=0 planes=31 thr=0,0,0 keep_after=0"
CHANGE = " spec 0x1004 grid=68x120 cell=8 source=0 crop=1 mode=1 planes=35 thr=3,2,1 keep_after=0"
CHAIN = " spec 0x2000 grid=5x6 cell=4 source=2 crop=1 mode=1 planes=63 thr=0,0,255 keep_after=1"
BLANK = dict(got="untouched", current="untouched", kept="untouched", picId="untouched", keptPicId="untouched")

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order; "final": the lines behind #final"""
    return host_program.records("cell_maps", str(tmp_path_factory.mktemp("cell_maps")), request.param)


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec if ln and ln[0] != " " and "=" in ln and not ln.startswith(("rc=", "keep ", "cells ")))


def _slots(records):
    """slot of the pops in order: A (picId 100), N, B, T, A (101)"""
    return [int(ln.split("slot=")[1].split()[0]) for ln in records["pops"]]


def test_the_pops_are_what_the_calls_should_see(records):
    pops = records["pops"]
    assert [p.split()[1] for p in pops] == ["A", "N", "B", "T", "A"]
    assert "picId=100 size=40x23" in pops[0] and "picId=400" in pops[1] and "picId=200 size=120x68" in pops[2] and "picId=101" in pops[4]


def test_picture_mode_needs_no_kept_picture(records):
    slot_a, _, slot_b = _slots(records)[:3]
    rec = records["picture_a_only"]                                # before anything was kept; B has no current picture yet
    assert rec[:5] == ["rc=0", "cells m=1 k=1 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,640,360", PICTURE]
    assert _arrays(rec) == dict(got="1,0", current="1,0", kept="0,0", picId="100,0", keptPicId="0,0")
    rec = records["picture_both"]                                  # A kept, B not: PICTURE takes both
    assert rec[:2] == ["rc=0", "cells m=2 k=2 stream=0x0"] and f" pic 1 slot={slot_b} win=0,0,1920,1080 mr=0,0" in rec
    assert " reg 1 index=1 0,0,1920,1080" in rec and rec[-6] == PICTURE
    assert _arrays(rec) == dict(got="1,1", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["a_not_current_picture"]
    assert rec[:2] == ["rc=0", "sink: not called"] and _arrays(rec) == dict(got="0", current="0", kept="1", picId="0", keptPicId="100")


def test_change_mode_names_only_instances_with_both_pictures(records):
    slot_a = _slots(records)[0]
    rec = records["nothing_kept"]
    assert rec[:2] == ["rc=0", "sink: not called"]
    assert _arrays(rec) == dict(got="0,0", current="1,0", kept="0,0", picId="100,0", keptPicId="0,0")
    rec = records["a_has_both"]
    assert rec[:5] == ["rc=0", "cells m=1 k=1 stream=0x0", f" pic 0 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,640,360", CHANGE]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["coded_frame"]
    assert rec[2:4] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", " reg 0 index=0 0,0,640,368"]
    assert rec[4] == " spec 0x1000 grid=1x1 cell=64 source=2 crop=0 mode=1 planes=1 thr=0,0,0 keep_after=0"
    rec = records["a_not_current"]
    assert rec[:2] == ["rc=0", "sink: not called"] and _arrays(rec) == dict(got="0", current="0", kept="1", picId="0", keptPicId="100")
    rec = records["a_next_picture"]
    assert rec[1] == "cells m=1 k=1 stream=0x0" and rec[2] == f" pic 0 slot={_slots(records)[4]} win=0,0,640,360 mr=0,0"
    assert _arrays(rec) == dict(got="1", current="1", kept="1", picId="101", keptPicId="100")


def test_explicit_regions_in_both_modes(records):
    slot_a, _, slot_b = _slots(records)[:3]
    rec = records["boxes_mixed_order"]                             # B, A: B has nothing kept, the boxes that name A (instance 1) are 0 and 2
    assert rec[:5] == ["rc=0", "cells m=1 k=2 stream=0x5000", f" pic 1 slot={slot_a} win=0,0,640,360 mr=0,0", " reg 0 index=0 0,0,64,64",
                       " reg 0 index=2 700,10,8,8"]
    assert rec[5] == CHANGE and _arrays(rec) == dict(got="1,0,1,0", current="1,1", kept="0,1", picId="200,100", keptPicId="0,100")
    rec = records["picture_boxes"]                                 # A is named first: picture 0 of the list, though instance 1 of the call
    assert rec[:8] == ["rc=0", "cells m=2 k=4 stream=0x5000", f" pic 1 slot={slot_a} win=0,0,640,360 mr=0,0", f" pic 0 slot={slot_b} win=0,0,1920,1080 mr=0,0",
                       " reg 0 index=0 0,0,64,64", " reg 1 index=1 -5,7,100,30", " reg 0 index=2 700,10,8,8", " reg 1 index=3 0,0,640,360"]
    assert _arrays(rec) == dict(got="1,1,1,1", current="1,1", kept="0,1", picId="200,100", keptPicId="0,100")
    rec = records["null_arrays"]
    assert rec[0] == "rc=0" and rec[1].startswith("cells m=1 k=1")
    assert _arrays(rec) == dict(got="1,0", current="null", kept="null", picId="null", keptPicId="null")
    rec = records["no_regions"]
    assert rec[:2] == ["rc=0", "sink: not called"] and _arrays(rec)["got"] == "null"


def test_failed_calls_write_nothing_and_mark_nothing(records):
    rec = records["cells_fail"]
    assert rec[0] == "rc=-2" and rec[1].startswith("cells m=1 k=1") and not any(ln.startswith("keep ") for ln in rec)
    assert _arrays(rec) == BLANK
    rec = records["picture_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("cells m=2 k=2") and _arrays(rec) == BLANK
    rec = records["keep_after_fails"]
    assert rec[0] == "rc=-2" and rec[1].startswith("cells m=1 k=1") and "keep m=2 k=0 stream=0x0" in rec
    assert _arrays(rec) == BLANK
    assert _arrays(records["b_still_not_kept"]) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")


def test_keep_after_reports_what_the_comparison_saw_and_keeps_everyone(records):
    slot_a, _, slot_b = _slots(records)[:3]
    rec = records["keep_after"]
    assert rec[0] == "rc=0" and rec[1] == "cells m=1 k=1 stream=0x0" and CHAIN in rec
    at = rec.index("keep m=2 k=0 stream=0x0")
    assert at > rec.index(CHAIN) and rec[at + 1:at + 3] == [f" pic 0 slot={slot_a} win=0,0,640,368 mr=0,0", f" pic 1 slot={slot_b} win=0,0,1920,1088 mr=0,0"]
    assert _arrays(rec) == dict(got="1,0", current="1,1", kept="1,0", picId="100,200", keptPicId="100,0")
    rec = records["both_kept"]
    assert rec[1] == "cells m=2 k=2 stream=0x0" and f" pic 1 slot={slot_b} win=0,0,1920,1080 mr=0,0" in rec
    assert _arrays(rec) == dict(got="1,1", current="1,1", kept="1,1", picId="100,200", keptPicId="100,200")


@pytest.mark.parametrize("name", ["refused_repeated", "refused_capture", "refused_got_null", "refused_threshold", "refused_cell", "refused_grid",
                                  "refused_planes", "refused_picture_keeps", "refused_picture_above", "refused_no_keep_change"])
def test_refused_calls_call_no_sink_and_write_nothing(records, name):
    rec = records[name]
    assert rec[:2] == ["rc=-1", "sink: not called"]
    assert all(v in ("untouched", "null") for v in _arrays(rec).values()), rec


def test_a_sink_that_cannot_keep_serves_picture_mode(records):
    rec = records["no_keep_picture"]
    assert rec[:2] == ["rc=0", "cells m=2 k=2 stream=0x0"] and rec[-6] == PICTURE
    assert _arrays(rec) == dict(got="1,1", current="1,1", kept="1,0", picId="100,400", keptPicId="100,0")


def test_the_twins_output_queue_is_untouched(records):
    final = records["final"]
    assert "twin=1" in final and final[0].split("=")[1] == final[1].split("=")[1]
