"""What the background model's two calls — h264bsdmiBlendCurrentPictures and h264bsdmiOutputKeptPictures — hand to the engine and write
back, without a GPU: api.c bound to a recording device stand-in (tests/fuzz_asan/mock_engine.c) and driven by a stand-alone C
program (tests/fuzz_asan/background.c), built with gcc, plain and with Address-, UB- and LeakSanitizer: a host program on the CPU that
is run directly.  Instances: A the 640x360 stream (picIds from 100), B the 1920x1080 stream (from 200), C never fed."""
import shutil

import pytest

import host_program

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record"""
    return host_program.records("background", str(tmp_path_factory.mktemp("background")), request.param)


def _sink(rec):
    """rc and what the sink recorded"""
    return rec[0], [ln for ln in rec[1:] if "=" not in ln.split(" ")[0] or ln.startswith(" ")]


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec[1:] if not ln.startswith(" ") and "=" in ln.split(" ")[0])


BLEND_BLANK = dict(kept="untouched", blended="untouched", picId="untouched")
OUT_BLANK = dict(got="untouched", keptPicId="untouched")
NOT_CALLED = ["sink: not called"]


@pytest.mark.parametrize("what", ["no_spec", "shift_8", "shift_max", "hold_256", "moving_shift_9", "moving_shift_max", "no_instances", "no_kept_array",
                                  "repeated_instance", "capture_mode", "sink_without_the_entry"])
def test_a_refused_blend_calls_no_sink_and_writes_nothing(records, what):
    rec = records[f"refused_{what}"]
    assert _sink(rec) == ("rc=-1", NOT_CALLED) and _arrays(rec) == BLEND_BLANK


def test_no_instances_is_nothing_to_do(records):
    assert _sink(records["nothing_to_do"]) == ("rc=0", NOT_CALLED)


def test_the_first_blend_starts_the_model_of_every_instance_with_a_current_picture(records):
    """the sink gets the keep call's pictures (whole coded frames), told that nothing is kept yet, the spec as given, and how many
    moving counters the call has: one per instance, C's included"""
    rc, sink = _sink(records["first"])
    assert rc == "rc=0"
    assert sink == ["blend m=2 n_moving=3 stream=0x0",
                    " pic 0 index=0 slot=3 win=0,0,640,368 mr=0,0 fresh=1",
                    " pic 1 index=1 slot=3 win=0,0,1920,1088 mr=0,0 fresh=1",
                    " spec shift=4 hold=255 moving_shift=4 moving=0x0"]
    assert _arrays(records["first"]) == dict(kept="1,1,0", blended="0,0,0", picId="100,200,0")


def test_nothing_is_marked_after_a_failing_sink_call(records):
    """-2 writes nothing; the call after a failed first blend still starts the models, the one after a failed third still sees 101"""
    assert _sink(records["first_fails"]) == ("rc=-2", _sink(records["first"])[1]) and _arrays(records["first_fails"]) == BLEND_BLANK
    assert records["third_fails"][0] == "rc=-2" and _arrays(records["third_fails"]) == BLEND_BLANK
    assert _arrays(records["kept_out"])["keptPicId"] == "101,200,0"


def test_a_later_blend_goes_into_the_kept_pictures_and_carries_stream_spec_and_counters(records):
    rc, sink = _sink(records["second"])
    assert rc == "rc=0"
    assert sink == ["blend m=2 n_moving=3 stream=0x77",
                    " pic 0 index=0 slot=0 win=0,0,640,368 mr=0,0 fresh=0",
                    " pic 1 index=1 slot=3 win=0,0,1920,1088 mr=0,0 fresh=0",
                    " spec shift=3 hold=12 moving_shift=8 moving=0x3000"]
    assert _arrays(records["second"]) == dict(kept="1,1,0", blended="1,1,0", picId="101,200,0")


def test_a_plain_keep_and_a_blend_share_what_is_known_of_the_kept_picture(records):
    """A kept 102 with h264bsdmiKeepCurrentPictures, then blends 103 into it"""
    assert _sink(records["after_a_keep"])[1][1].endswith("fresh=0")
    assert _arrays(records["after_a_keep"]) == dict(kept="1", blended="1", picId="103")


def test_blended_and_pic_id_are_optional(records):
    assert records["optional_arrays"][0] == "rc=0" and _arrays(records["optional_arrays"]) == dict(kept="1")


def test_a_kept_picture_of_another_coded_size_counts_as_none(records):
    assert _arrays(records["size_a_first"])["blended"] == "0" and _arrays(records["size_a_second"])["blended"] == "1"
    assert _sink(records["kept_out_of_another_size"]) == ("rc=0", NOT_CALLED)
    assert _arrays(records["kept_out_of_another_size"]) == dict(got="0", keptPicId="0")
    rc, sink = _sink(records["size_b_first"])
    assert rc == "rc=0" and sink[1].endswith("win=0,0,1920,1088 mr=0,0 fresh=1")
    assert _arrays(records["size_b_first"])["blended"] == "0" and _arrays(records["size_b_second"])["blended"] == "1"


def test_the_readback_names_the_instances_that_keep_a_picture_and_their_buffers(records):
    assert _sink(records["kept_out_nothing_kept"]) == ("rc=0", NOT_CALLED)
    assert _arrays(records["kept_out_nothing_kept"]) == dict(got="0,0,0", keptPicId="0,0,0")
    assert _sink(records["kept_out"]) == ("rc=0", ["kept_out m=2 stream=0x77", " inst 0 picture=0x10000 fraction=0x40000",
                                                   " inst 1 picture=0x20000 fraction=0x0"])
    assert _arrays(records["kept_out"]) == dict(got="1,1,0", keptPicId="101,200,0")
    assert _sink(records["kept_out_no_fractions"]) == ("rc=0", ["kept_out m=2 stream=0x0", " inst 0 picture=0x10000 fraction=0x0",
                                                                " inst 1 picture=0x20000 fraction=0x0"])
    assert _sink(records["kept_out_ignores_buffers_of_instances_without"])[0] == "rc=0"
    assert records["kept_out_fails"][0] == "rc=-2" and _arrays(records["kept_out_fails"]) == OUT_BLANK


@pytest.mark.parametrize("what", ["capture_mode", "unaligned", "unaligned_fraction", "no_buffer", "repeated_instance", "sink_without_the_entry"])
def test_a_refused_readback_calls_no_sink_and_writes_nothing(records, what):
    rec = records[f"kept_out_refused_{what}"]
    assert _sink(rec) == ("rc=-1", NOT_CALLED) and _arrays(rec) == OUT_BLANK
