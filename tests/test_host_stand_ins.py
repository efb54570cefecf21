"""The two device stand-ins of the host-side tests against the product's JobSink (h264bsd_amd/csrc/hostdec.h): tests/fuzz_asan/mock_engine.c
records every optional entry and leaves out those a test program asks it to (mock_without), tests/fuzz_asan/stub_engine.c knows none of
them.  That an entry left out is refused and not called is shown where the entry is tested: the records refused_sink_without_entry (shift,
corners), refused_sink_without_boxes, sink_without_boxes_serves_maps, no_keep_picture, refused_sink_without_the_entry and
kept_out_refused_sink_without_the_entry of the test_*_host.py files."""
import os
import re
import shutil
import subprocess

import pytest

from host_program import CSRC, FUZZ


def _members():
    """the function-pointer members of JobSink in their order"""
    hostdec = open(os.path.join(CSRC, "hostdec.h")).read()
    members = hostdec[hostdec.index("typedef struct JobSink {"):hostdec.index("} JobSink;")]
    return re.findall(r"\(\*(\w+)\)\s*\(", re.sub(r"/\*.*?\*/", "", members, flags=re.S))


def _optional():
    """the entries mock_engine.h gives a bit to, as JobSink names them, in the order of the enum"""
    return [n.lower() for n in re.findall(r"\bMOCK_(\w+) = 1 << \d+,", open(os.path.join(FUZZ, "mock_engine.h")).read())]


def test_a_sink_is_handed_over_zeroed_and_grew_at_its_end():
    """what a stand-in does not set is the NULL of the zeroed struct it is handed (hd_create), which the calls refuse"""
    core = open(os.path.join(CSRC, "hd_core.c")).read()
    assert "(HostDec *)calloc(1, sizeof(HostDec))" in core
    hostdec = open(os.path.join(CSRC, "hostdec.h")).read()
    members = hostdec[hostdec.index("typedef struct JobSink {"):hostdec.index("} JobSink;")]
    assert members.index("(*cell_boxes)") < members.index("(*blend_pictures)") < members.index("(*kept_pictures_out)")


@pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")
def test_the_stand_ins_compile_without_a_warning(tmp_path):
    for source in ("stub_engine.c", "mock_engine.c"):
        b = subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", f"-I{CSRC}", "-DH264BSD_BUILD", "-c", os.path.join(FUZZ, source),
                            "-o", str(tmp_path / (source + ".o"))], capture_output=True, text=True)
        assert b.returncode == 0, (source, b.stderr[-3000:])


def test_the_enum_names_the_optional_entries_in_the_order_of_the_struct():
    members, optional = _members(), _optional()
    assert len(optional) >= 12 and set(optional) <= set(members)
    assert optional == [m for m in members if m in optional]


def test_the_stub_names_no_optional_entry():
    stub = open(os.path.join(FUZZ, "stub_engine.c")).read()
    assert not [n for n in _optional() if n in stub]


def test_the_recording_stand_in_sets_every_member_of_the_sink():
    """a future entry that nobody mocks fails here; each optional one is left out on request"""
    mock = open(os.path.join(FUZZ, "mock_engine.c")).read()
    members = _members()
    assert len(members) >= 24
    assert not [m for m in members if not re.search(rf"\bs->{m} = ", mock)]
    assert not [n for n in _optional() if not re.search(rf"\bs->{n} = mock_without & MOCK_{n.upper()} \? NULL : m_{n};", mock)]
