"""The four pulls that may compare against kept pictures and may keep afterwards — h264bsdmiOutputRegionChange,
h264bsdmiOutputRegionShift, h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes (CHANGE mode) — share ONE host path in api.c
(kept_pull).  Each feature's own host test says what its entry is handed; this one holds the four to the same sequence of sink calls
and the same output arrays, scenario by scenario: the entry, then keep_pictures, then nothing after a failure.  A stand-alone C program
(tests/fuzz_asan/kept_pulls.c) bound to a recording device stand-in (tests/fuzz_asan/mock_engine_kept.c), built with gcc, plain and
with Address-, UB- and LeakSanitizer: a host program on the CPU that is run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264bsd_amd", "csrc")
HOST_SOURCES = ("hd_nal.c", "hd_params.c", "hd_slice.c", "hd_dpb.c", "hd_cavlc.c", "hd_resid.c", "hd_mb.c", "hd_core.c", "api.c")
STREAMS = [os.path.join(ROOT, "tests", "golden", n) for n in ("test_640x360.h264", "test_1920x1080.h264")]
ENTRIES = ["change", "shift", "cells", "boxes"]

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=[None, "address,undefined"], ids=["plain", "sanitizers"])
def records(request, tmp_path_factory):
    """name -> the lines of that call's record"""
    exe = os.path.join(str(tmp_path_factory.mktemp("kept_pulls")), "kept_pulls")
    srcs = [os.path.join(ROOT, "tests", "fuzz_asan", f) for f in ("kept_pulls.c", "mock_engine_kept.c")] + [os.path.join(CSRC, f) for f in HOST_SOURCES]
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", f"-I{CSRC}", "-DH264BSD_BUILD"]
    if request.param:
        cmd += [f"-fsanitize={request.param}", "-fno-omit-frame-pointer"]
    b = subprocess.run(cmd + srcs + ["-lpthread", "-lm", "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe] + STREAMS, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    err = "\n".join(ln for ln in r.stderr.splitlines() if "left shift of negative" not in ln)      # (mirrors the reference's arithmetic)
    assert "ERROR: AddressSanitizer" not in err and "ERROR: LeakSanitizer" not in err and "runtime error" not in err, err[-2000:]
    out, name = {}, None
    for ln in r.stdout.splitlines():
        if ln.startswith("#"):
            name = ln[1:]
            assert name not in out
            out[name] = []
        else:
            out[name].append(ln)
    return out


def _calls(rec):
    """rc and the sink calls of a record in order"""
    return rec[0], [ln for ln in rec[1:] if "=" not in ln.split(" ")[0]]


def _arrays(rec):
    return dict(ln.split("=", 1) for ln in rec[1:] if "=" in ln.split(" ")[0])


BLANK = dict(got="untouched", current="untouched", kept="untouched", picId="untouched", keptPicId="untouched")


@pytest.mark.parametrize("entry", ENTRIES)
def test_without_a_pair_no_entry_is_called_and_a_failed_keep_marks_nothing(records, entry):
    assert _calls(records[f"{entry}_nothing_kept"]) == ("rc=-2", ["keep m=2 k=0"])
    assert _arrays(records[f"{entry}_nothing_kept"]) == BLANK
    assert _calls(records[f"{entry}_still_nothing_kept"]) == ("rc=0", ["sink: not called"])
    assert _arrays(records[f"{entry}_still_nothing_kept"]) == dict(got="0,0", current="1,1", kept="0,0", picId="100,200", keptPicId="0,0")


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_entry_names_the_instances_with_both_pictures_and_nothing_follows_it(records, entry):
    assert _calls(records[f"{entry}_plain"]) == ("rc=0", [f"{entry} m=1 k=1"])
    assert _arrays(records[f"{entry}_plain"]) == dict(got="1,0", current="1,1", kept="1,0", picId="101,200", keptPicId="100,0")


@pytest.mark.parametrize("entry", ENTRIES)
def test_nothing_is_called_after_a_failure_and_nothing_is_written_or_marked(records, entry):
    assert _calls(records[f"{entry}_entry_fails"]) == ("rc=-2", [f"{entry} m=1 k=1"])
    assert _arrays(records[f"{entry}_entry_fails"]) == BLANK
    assert _calls(records[f"{entry}_keep_fails"]) == ("rc=-2", [f"{entry} m=1 k=1", "keep m=2 k=0"])
    assert _arrays(records[f"{entry}_keep_fails"]) == BLANK
    assert _arrays(records[f"{entry}_marked_nothing"]) == _arrays(records[f"{entry}_plain"])


@pytest.mark.parametrize("entry", ENTRIES)
def test_keep_after_is_the_keep_entry_behind_the_entry_and_reports_what_the_comparison_saw(records, entry):
    assert _calls(records[f"{entry}_keep_after"]) == ("rc=0", [f"{entry} m=1 k=1", "keep m=2 k=0"])
    assert _arrays(records[f"{entry}_keep_after"]) == dict(got="1,0", current="1,1", kept="1,0", picId="101,200", keptPicId="100,0")
    assert _calls(records[f"{entry}_both_kept"]) == ("rc=0", [f"{entry} m=2 k=2"])
    assert _arrays(records[f"{entry}_both_kept"]) == dict(got="1,1", current="1,1", kept="1,1", picId="101,200", keptPicId="101,200")


def test_the_four_entries_differ_in_the_name_of_the_sink_entry_alone(records):
    by_entry = {e: {n[len(e) + 1:]: [ln.replace(e, "ENTRY") for ln in rec] for n, rec in records.items() if n.startswith(e + "_")} for e in ENTRIES}
    assert len(by_entry["change"]) == 8
    assert by_entry["shift"] == by_entry["change"] and by_entry["cells"] == by_entry["change"] and by_entry["boxes"] == by_entry["change"]
