"""What an ACCEPTED pull of current pictures hands to the engine and writes back, without a GPU: the four entries of api.c
(h264bsdmiOutputTensorRegions, h264bsdmiOutputTensorRemap, h264bsdmiOutputMotionRegions, h264bsdmiOutputRegionStats) bound to the
recording device stand-in (tests/fuzz_asan/mock_engine.c) by a stand-alone C program (tests/fuzz_asan/current_pulls.c), over the grid
of tests/golden/make_current_pull_pins.py.  Every record — return code, the deduplicated picture list in its order, windows, resolved
matrix and range, letterbox rectangles, the substituted default specs, got / box / current / picId — must equal
tests/golden/current_pull_pins.json, recorded from the commit before the four entries were put on one host path."""
import importlib.util
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264bsd_amd", "csrc")
_spec = importlib.util.spec_from_file_location("make_current_pull_pins", os.path.join(ROOT, "tests", "golden", "make_current_pull_pins.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="no gcc")


@pytest.fixture(scope="module", params=[None, "address,undefined"], ids=["plain", "sanitizers"])
def run(request, tmp_path_factory):
    """(records, final) of the program built from this tree; the second parametrisation builds it with Address-, UB- and LeakSanitizer —
    a host program on the CPU, as test_parser_fuzz.py::test_batch_calls_under_sanitizers — and must run clean"""
    return gen.run(gen.build(CSRC, str(tmp_path_factory.mktemp("current_pulls")), sanitize=request.param))


def _arrays(record):
    return {k: v for k, v in (ln.split("=", 1) for ln in record.split("\n") if ln and ln[0] != " " and "=" in ln and not ln.startswith("rc="))
            if k in ("got", "box", "current", "picId")}


def test_records_equal_the_pins(run):
    records, final = run
    pins = json.load(open(gen.PINS))
    grid = gen.cases()
    assert pins["cases"] == len(pins["pins"]) == len(grid) == len(records)
    wrong = [(i, c, r) for i, (c, r, want) in enumerate(zip(grid, records, pins["pins"])) if gen.pin(r) != want]
    for i, c, r in wrong[:5]:
        print(f"case {i}: {c}\n{r}")
    assert not wrong, f"{len(wrong)} of {len(grid)} records differ from the pins, the first: case {wrong[0][0]}: {wrong[0][1]}"
    assert final == pins["final"]


def test_refused_and_failed_calls_write_nothing_and_nothing_is_popped(run):
    records, final = run
    for c, r in zip(gen.cases(), records):
        rc = int(r.split("\n")[0][3:])
        assert rc in (0, -1, -2), c
        assert ("sink: not called" in r) == (rc == -1 or " k=" not in r), c
        if rc:
            assert all(v in ("untouched", "null") for v in _arrays(r).values()), (c, r)
        flags = int(c.split()[-1])
        assert (rc == -2) == (bool(flags & 16) and "sink: not called" not in r), c
    assert "twin=1\n" in final            # A's output queue gives what its untouched twin's gives


def test_the_same_call_twice_gives_the_same(run):
    records = run[0]
    grid = gen.cases()
    twice = [(i, k) for i, c in enumerate(grid) for k in range(i + 1, len(grid)) if grid[k] == c]
    assert len(twice) >= 4 and all(records[i] == records[k] and records[i].startswith("rc=0") for i, k in twice)


def test_grid_reaches_every_outcome(run):
    records = run[0]
    grid = gen.cases()
    for entry, name in zip("rmvs", ("regions", "remap", "motion", "stats")):
        mine = [r for c, r in zip(grid, records) if c[0] == entry]
        assert {r.split("\n")[0] for r in mine} == {"rc=0", "rc=-1", "rc=-2"}, entry
        assert all(r.split("\n")[1].startswith(name + " ") for r in mine if "sink: not called" not in r), entry
        got = [_arrays(r)["got"] for r in mine if r.startswith("rc=0")]
        assert any("0" in g.split(",") and "1" in g.split(",") for g in got), entry                  # got mixed
        assert any(set(g.split(",")) == {"0"} for g in got), entry                                   # nobody has a picture: no launch
        assert any(r.split("\n")[1].split()[1] in ("m=2", "m=3") for r in mine if "sink: not called" not in r), entry      # several pictures
        assert any(r.startswith("rc=0\nsink: not called") for r in mine), entry
        assert any("=null" in r for r in mine if r.startswith("rc=0")), entry
    # B is used first where it is named first, and a picture is listed once however many regions name it
    first = records[grid.index(next(c for c in grid if c.startswith("r 2 AB 8")))].split("\n")
    assert first[1].startswith("regions m=2 k=8") and first[2].startswith(" pic 1 ") and first[3].startswith(" pic 0 ")
    # cropping and the VUI: A's window is 640x360 of 640x368 coded, B is full range
    text = "\n".join(records)
    assert "win=0,0,640,360" in text and "win=0,0,640,368" in text and "win=0,0,1920,1080" in text and "win=0,0,1920,1088" in text
    ranges = {ln.split(" mr=")[1].split()[0] for ln in text.split("\n") if ln.startswith(" pic 1 ")}        # B (instance 1 of "AB") / A (of "BA")
    assert {"0,0", "3,2", "2,1"} <= ranges and len(ranges) >= 5
    # a letterboxed rectangle that is not the whole output, for regions and for motion
    for entry in "rv":
        assert any(ln.startswith(" reg ") and not ln.endswith("box=0,0,64,40") for c, r in zip(grid, records) if c[0] == entry and " 64x40 " in r
                   for ln in r.split("\n")), entry
    # the defaults the entries substitute: bilinear stretch, bilinear constant
    assert any(c.split()[7] == "0" and "\n resize 0 0 pad=0,0,0\n" in r for c, r in zip(grid, records) if c[0] == "r")
    assert any(c.split()[7] == "0" and "\n remap 1 0 pad=0,0,0\n" in r for c, r in zip(grid, records) if c[0] == "m")


def test_pins_are_compact():
    assert os.path.getsize(gen.PINS) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "tick_plan_pins.json"))
