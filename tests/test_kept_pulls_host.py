"""The four pulls that may compare against kept pictures and may keep afterwards — h264bsdmiOutputRegionChange,
h264bsdmiOutputRegionShift, h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes (CHANGE mode) — share ONE host path in api.c
(kept_pull).  Each feature's own host test says what its entry is handed; this one holds the four to the same sequence of sink calls
and the same output arrays, scenario by scenario: the entry, then keep_pictures, then nothing after a failure (read off the header
lines of the records).  A stand-alone C program
(tests/fuzz_asan/kept_pulls.c) bound to a recording device stand-in (tests/fuzz_asan/mock_engine.c), built with gcc, plain and
with Address-, UB- and LeakSanitizer: a host program on the CPU that is run directly."""
import shutil

import pytest

import host_program

ENTRIES = ["change", "shift", "cells", "boxes"]

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=host_program.SANITIZERS, ids=host_program.SANITIZER_IDS)
def records(request, tmp_path_factory):
    """name -> the lines of that call's record"""
    return host_program.records("kept_pulls", str(tmp_path_factory.mktemp("kept_pulls")), request.param)


def _calls(rec):
    """rc and the sink calls of a record in order: the name, m and k of every header line (what each entry is handed in full follows its
    header on lines that start with a blank, and is the business of the four features' own tests)"""
    return rec[0], [" ".join(ln.split(" ")[:3]) for ln in rec[1:] if not ln.startswith(" ") and "=" not in ln.split(" ")[0]]


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
    by_entry = {e: {n[len(e) + 1:]: [ln.replace(e, "ENTRY") for ln in rec if not ln.startswith(" ")] for n, rec in records.items() if n.startswith(e + "_")} for e in ENTRIES}
    assert len(by_entry["change"]) == 8
    assert by_entry["shift"] == by_entry["change"] and by_entry["cells"] == by_entry["change"] and by_entry["boxes"] == by_entry["change"]
