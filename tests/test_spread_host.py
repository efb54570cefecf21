"""What the host path of the background spread hands to the engine, without a GPU: api.c's h264bsdmiBlendCurrentPicturesSpread and
h264bsdmiOutputKeptSpread, and the SPREAD mode of h264bsdmiOutputCellMaps / h264bsdmiOutputCellBoxes, bound to the recording device
stand-in (tests/fuzz_asan/mock_engine.c, unchanged) and to the recording table of the program itself, which has all six entries behind
the last member of JobSink, by a stand-alone C program (tests/fuzz_asan/spread.c).  Instances: A (640x360 in a coded 640x368, picIds
from 100) and B (1920x1080 in 1920x1088, from 200) fed and popped, C never fed, D as A from 500, O on a sink whose table has the first
four members only, G capture mode.  tests/fuzz_asan/spread_absent.c is the same on an engine without any table.  Built with gcc, plain
and with Address-, UB- and LeakSanitizer: host programs on the CPU that are run directly (tests/host_program.py)."""
import shutil

import pytest

import host_program

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")

GATED = " spec shift=3 hold=12 moving_shift=8 moving=0x3000"
ALL = " spread gain=2 lowest=2 highest=255 update=1"
STILL = " spread gain=8 lowest=0 highest=40 update=2"
MODE2 = " spec 0x1000 grid=23x40 cell=16 source=1 crop=1 mode=2 planes=15 thr=6,3,2 keep_after=0"
BLEND_BLANK = ["kept=untouched", "blended=untouched", "picId=untouched"]
OUT_BLANK = ["got=untouched", "keptPicId=untouched"]
CELLS_BLANK = ["got=untouched", "current=untouched", "kept=untouched", "picId=untouched", "keptPicId=untouched"]
REFUSED_BLENDS = ["spread_null", "gain_0", "gain_9", "gain_max", "lowest_above_highest", "highest_256", "lowest_256", "update_3", "spec_null", "shift_8",
                  "hold_256", "moving_shift_9", "instances_null", "kept_null", "repeated", "capture", "sink_without_entry", "sink_without_entry_second"]


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record; "pops": the pop lines in order"""
    return host_program.records("spread", str(tmp_path_factory.mktemp("spread")), request.param)


def test_the_driver_ran_and_reached_none_of_the_older_entries(records):
    assert [p.split()[1] for p in records["pops"]] == ["A", "B", "D", "O"]
    assert len(records) == 1 + len(REFUSED_BLENDS) + 35
    assert not any(ln.startswith(("flow ", "matches ", "model ", "warp ")) for rec in records.values() for ln in rec)


@pytest.mark.parametrize("what", REFUSED_BLENDS)
def test_a_refused_spread_blend_calls_nothing_and_writes_nothing(records, what):
    """every -1 of the header: the spread spec, everything the blend refuses, a sink whose table lacks the entry, first or second"""
    assert records[f"refused_{what}"] == ["rc=-1", "sink: not called"] + BLEND_BLANK


def test_no_instances_is_nothing_to_do(records):
    assert records["nothing_to_do"] == ["rc=0", "sink: not called"] + BLEND_BLANK


def test_the_first_spread_blend_says_what_is_known_of_kept_picture_and_spread(records):
    """A and B hold a kept picture from a plain keep and no valid spread; D holds nothing: its model starts.  The entry gets the keep
    call's pictures, both specs as given, the stream, and one moving counter per instance of the call"""
    assert records["first"] == ["rc=0", "blend_spread m=2 n_moving=3 stream=0x0", " pic 0 index=0 slot=0 win=0,0,640,368 fresh=0 unset=1",
                                " pic 1 index=1 slot=3 win=0,0,1920,1088 fresh=0 unset=1", GATED, ALL, "kept=1,1,0", "blended=1,1,0", "picId=101,200,0"]
    rec = records["model_starts"]
    assert rec[:3] == ["rc=0", "blend_spread m=1 n_moving=1 stream=0x0", " pic 0 index=0 slot=3 win=0,0,640,368 fresh=1 unset=1"]
    assert rec[3:] == [GATED, STILL, "kept=1", "blended=0", "picId=500"]
    assert records["out_of_a_started_model"] == ["rc=0", "spread_out m=1 stream=0x0", " inst 0 spread=0x10000", "got=1", "keptPicId=500"]


def test_a_later_spread_blend_finds_both_and_carries_stream_and_specs(records):
    assert records["second"] == ["rc=0", "blend_spread m=2 n_moving=3 stream=0x5000", " pic 0 index=0 slot=2 win=0,0,640,368 fresh=0 unset=0",
                                 " pic 1 index=1 slot=3 win=0,0,1920,1088 fresh=0 unset=0", " spec shift=4 hold=255 moving_shift=4 moving=0x0", STILL,
                                 "kept=1,1,0", "blended=1,1,0", "picId=102,200,0"]


def test_a_failing_entry_marks_nothing(records):
    """-2 writes nothing; the spread is still not valid afterwards (nothing to hand out), the next call says unset again"""
    assert records["first_fails"] == ["rc=-2"] + records["first"][1:6] + BLEND_BLANK
    assert records["out_after_a_failed_blend"] == ["rc=0", "sink: not called", "got=0,0,0", "keptPicId=100,200,0"]
    assert records["out_fails"] == ["rc=-2", "spread_out m=2 stream=0x0", " inst 0 spread=0x10000", " inst 1 spread=0x20000"] + OUT_BLANK


def test_the_readback_names_the_instances_with_a_valid_spread(records):
    assert records["out_nothing_yet"] == ["rc=0", "sink: not called", "got=0,0,0", "keptPicId=0,0,0"]
    assert records["out"] == ["rc=0", "spread_out m=2 stream=0x5000", " inst 0 spread=0x10000", " inst 1 spread=0x20000", "got=1,1,0", "keptPicId=101,200,0"]


def test_a_plain_blend_leaves_the_spread_and_a_plain_keep_invalidates_it(records):
    """between two spread blends: h264bsdmiBlendCurrentPictures (A still hands its spread out), h264bsdmiKeepCurrentPictures (A hands
    out nothing, mode 2 names B alone, A's next spread blend says unset and not fresh), and a keep_after of a sibling"""
    assert records["plain_blend"][1].startswith("blend m=1") and records["plain_blend"][-3:] == ["kept=1", "blended=1", "picId=103"]
    assert records["out_after_a_plain_blend"][-2:] == ["got=1,1,0", "keptPicId=103,200,0"]
    assert records["keep_a"][-2:] == ["kept=1", "picId=104"]
    assert records["out_after_a_keep"] == ["rc=0", "spread_out m=1 stream=0x0", " inst 1 spread=0x20000", "got=0,1,0", "keptPicId=104,200,0"]
    assert records["after_a_keep"][2:4] == [" pic 0 index=0 slot=0 win=0,0,640,368 fresh=0 unset=1", " pic 1 index=1 slot=3 win=0,0,1920,1088 fresh=0 unset=0"]
    assert records["out_again"][-2:] == ["got=1,1,0", "keptPicId=105,200,0"]
    rec = records["change_with_keep_after"]
    assert rec[0] == "rc=0" and rec[1].startswith("change m=1") and any(ln.startswith("keep m=1") for ln in rec) and rec[-1] == "got=1"
    assert records["out_after_keep_after"][-2:] == ["got=0,1,0", "keptPicId=105,200,0"]


def test_mode_2_names_only_instances_with_a_current_a_kept_picture_and_a_valid_spread(records):
    """through the sink's cell_maps / cell_boxes members, the spec as given; C has nothing, and after the keep A lacks the spread"""
    assert records["cells_kept_but_no_spread"] == ["rc=0", "sink: not called", "got=0,0,0", "current=1,1,0", "kept=1,1,0", "picId=100,200,0",
                                                   "keptPicId=100,200,0"]
    body = [" pic 0 slot=2 win=0,0,640,360 mr=0,0", " pic 1 slot=3 win=0,0,1920,1080 mr=0,0", " reg 0 index=0 0,0,640,360", " reg 1 index=1 0,0,1920,1080", MODE2]
    tail = ["got=1,1,0", "current=1,1,0", "kept=1,1,0", "picId=102,200,0", "keptPicId=102,200,0"]
    assert records["cells_ab"] == ["rc=0", "cells m=2 k=2 stream=0x0"] + body + tail
    assert records["boxes_ab"] == ["rc=0", "boxes m=2 k=2 stream=0x0"] + body + \
        [" boxes 0x2000 max=16 plane=8 channel=2 sense=0 level=5 conn=8 min_cells=1"] + tail
    assert records["cells_after_a_keep"] == ["rc=0", "cells m=1 k=1 stream=0x0", " pic 1 slot=3 win=0,0,1920,1080 mr=0,0", " reg 0 index=1 0,0,1920,1080", MODE2,
                                             "got=0,1,0", "current=1,1,0", "kept=1,1,0", "picId=104,200,0", "keptPicId=104,200,0"]


@pytest.mark.parametrize("what", ["cells_refused_keep_after", "boxes_refused_keep_after", "cells_refused_rgb", "cells_refused_plane_16", "cells_refused_mode_3",
                                  "cells_refused_sink_without_entry", "boxes_refused_sink_without_entry"])
def test_mode_2_refusals_call_no_sink_and_write_nothing(records, what):
    assert records[what] == ["rc=-1", "sink: not called"] + CELLS_BLANK


@pytest.mark.parametrize("what", ["unaligned", "no_buffer", "repeated", "capture", "sink_without_entry"])
def test_a_refused_readback_calls_nothing_and_writes_nothing(records, what):
    assert records[f"out_refused_{what}"] == ["rc=-1", "sink: not called"] + OUT_BLANK


@pytest.mark.parametrize("sanitize", host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def test_an_engine_without_the_table_refuses_the_spread_and_its_siblings_go_on(sanitize, tmp_path):
    recs = host_program.records("spread_absent", str(tmp_path), sanitize)
    assert recs["keep_a"][-2:] == ["kept=1", "picId=100"]
    assert recs["blend_refused_engine_without_entry"] == ["rc=-1", "sink: not called"] + BLEND_BLANK
    assert recs["out_refused_engine_without_entry"] == ["rc=-1", "sink: not called"] + OUT_BLANK
    for name in ("cells_refused_engine_without_entry", "boxes_refused_engine_without_entry"):
        assert recs[name] == ["rc=-1", "sink: not called"] + CELLS_BLANK
    assert recs["sibling_goes_on"][:2] == ["rc=0", "cells m=1 k=1 stream=0x0"] and recs["sibling_goes_on"][-5] == "got=1"
    assert recs["plain_blend_goes_on"][:2] == ["rc=0", "blend m=1 n_moving=1 stream=0x0"] and recs["plain_blend_goes_on"][-3:] == ["kept=1", "blended=1", "picId=100"]


@pytest.mark.parametrize("driver, call, line", [("warp_kept", "replicate_coded_frame", "warp m=2 n_count=3 stream=0x0"),
                                                ("background", "first", "blend m=2 n_moving=3 stream=0x0")])
def test_the_older_drivers_still_build_and_pass_untouched(driver, call, line, tmp_path):
    """their tables initialise the first four members, or none: the new ones are NULL there and the programs link as they stand"""
    recs = host_program.records(driver, str(tmp_path), None)
    assert recs[call][:2] == ["rc=0", line]
