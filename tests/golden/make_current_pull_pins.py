#!/usr/bin/env python3
"""The pins of the host path of the four pulls of CURRENT pictures (h264bsd_amd/csrc/api.c: h264bsdmiOutputTensorRegions,
h264bsdmiOutputTensorRemap, h264bsdmiOutputMotionRegions, h264bsdmiOutputRegionStats): for a grid of calls, the return code, all
the engine was handed (tests/fuzz_asan/mock_engine.c records it) and the output arrays afterwards.  tests/test_current_pulls.py
holds api.c to current_pull_pins.json; this file is the generator and holds the one grid both use.

The pins never come from the code under test: the generator is given the csrc directory of the commit BEFORE the change under
review, and builds tests/fuzz_asan/current_pulls.c + mock_engine.c of this tree against it:

    mkdir parent && git archive HEAD~ | tar -x -C parent
    python3 tests/golden/make_current_pull_pins.py parent/h264bsd_amd/csrc "$(git rev-parse --short HEAD~)"

A case is one line for current_pulls.c: entry (r regions, m remap, v motion, s stats), n, the instances (one letter each, '_' a
NULL element, '0' dec == NULL, '-' none), nRegions, the regions i,x,y,w,h or maps i,address joined by ';' ('0' NULL, '-' none), the
entry's spec ('0' NULL), the colour spec, the resize / remap spec ('x' where the entry has none), and flags: 1 got, 2 box,
4 current, 8 picId NULL; 16 the sink fails; 32 a stream is named.  A record is stored as text where it is short, else as its
SHA-256."""
import hashlib
import json
import math
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PINS = os.path.join(HERE, "current_pull_pins.json")
STREAMS = [os.path.join(HERE, "test_640x360.h264"), os.path.join(HERE, "test_1920x1080_fullRange.h264")]
sys.path.insert(0, os.path.join(ROOT, "tests"))
import host_program  # noqa: E402
LIMIT = 16384
TEXT_LIMIT = 150                # records up to this many characters are stored as they are
MAP = 0x2000

TENSOR = dict(data=0x1000, width=64, height=40, layout=0, dtype=1, channels=0, crop=1, resize=1, mean=(0, 0, 0), std=(1, 1, 1))
MOTION = dict(data=0x1000, width=64, height=40, layout=0, dtype=2, planes=3, crop=1, fit=0, sampler=0, units=0, per_picture=0)
STATS = dict(data=0x1000, source=1, bins=256, crop=1)


def _num(v):
    if isinstance(v, float) and (math.isnan(v) or math.isinf(v)):
        return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf")
    return repr(v)


def _join(values):
    flat = []
    for v in values:
        flat += list(v) if isinstance(v, (tuple, list)) else [v]
    return ",".join(_num(v) for v in flat)


def _spec(base, kw):
    if kw is None:
        return "0"
    s = dict(base)
    s.update(kw)
    return _join(s.values())


def case(entry, dec, items, spec=None, colour=None, aux=None, flags=0, n=None, nr=None):
    """one line; dec: the letters, None for dec == NULL; items: tuples, None for NULL (nRegions = n unless given); spec: a dict of
    changes to the entry's good spec, "null" for NULL; colour, aux: tuples or None"""
    base = {"r": TENSOR, "m": TENSOR, "v": MOTION, "s": STATS}[entry]
    n = (len(dec) if dec else 0) if n is None else n
    nr = (n if items is None else len(items)) if nr is None else nr
    d = "0" if dec is None else dec or "-"
    it = "0" if items is None else ";".join(_join(i) for i in items) or "-"
    has_colour, has_aux = entry in "rm", entry in "rm"
    return " ".join([entry, str(n), d, str(nr), it, _spec(base, None if spec == "null" else spec or {}),
                     ("0" if colour is None else _join(colour)) if has_colour else "x",
                     ("0" if aux is None else _join(aux)) if has_aux else "x", str(flags)])


BOXES = [(0, 0, 16, 16), (-5, 3, 17, 31), (7, -9, 33, 1), (LIMIT, -LIMIT, LIMIT, LIMIT), (-LIMIT, LIMIT, 1, LIMIT), (101, 55, 640, 360),
         (0, 0, 1920, 1080), (-1, -1, 3, 1000)]
BAD_BOXES = [(0, 0, 0, 16), (0, 0, 16, 0), (0, 0, LIMIT + 1, 16), (0, 0, 16, LIMIT + 1), (LIMIT + 1, 0, 16, 16), (-LIMIT - 1, 0, 16, 16),
             (0, LIMIT + 1, 16, 16), (0, -LIMIT - 1, 16, 16), (-2 ** 31, 0, 16, 16)]
RESIZES = [None, (0, 0, 0.0, 0.0, 0.0), (1, 0, 0.25, 0.5, 1.0), (0, 1, 0.0, 0.0, 0.0), (2, 1, 1.0, 0.5, 0.0)]
BAD_RESIZES = [(3, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, -0.01, 0, 0), (0, 0, 0, 1.01, 0), (0, 0, 0, 0, math.nan), (0, 0, math.inf, 0, 0)]
REMAPS = [None, (0, 0, 0.0, 0.0, 0.0), (1, 0, 0.0, 0.0, 0.0), (1, 1, 0.0, 0.0, 0.0), (0, 1, 1.0, 0.5, 0.0)]
BAD_REMAPS = [(2, 0, 0, 0, 0), (0, 2, 0, 0, 0), (2 ** 32 - 1, 0, 0, 0, 0), (0, 0, -0.01, 0, 0), (0, 0, 0, 1.01, 0), (0, 0, 0, 0, math.nan),
              (0, 0, math.inf, 0, 0), (0, 0, 0, -math.inf, 0)]
COLOURS = [None, (0, 0, 0, 0), (3, 2, 1, 0), (2, 1, 0, 0), (1, 0, 0, 2), (1, 0, 1, 3), (1, 2, 0, 6), (4, 0, 0, 0), (6, 0, 1, 0)]
BAD_COLOURS = [(7, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 2), (1, 0, 0, 0), (1, 0, 0, 1), (3, 3, 0, 0), (3, 0, 2, 0), (3, 0, 0, 1), (3, 0, 0, 7)]
BAD_TENSOR = [dict(data=0), dict(width=0), dict(height=0), dict(dtype=3), dict(layout=2), dict(channels=5), dict(layout=0, channels=2),
              dict(layout=0, channels=3), dict(std=(1, 0, 1)), dict(dtype=0, mean=(0.5, 0, 0)), dict(dtype=0, std=(1, 2, 1)), dict(resize=0),
              dict(resize=2), "null"]
SIZES = [dict(), dict(width=40, height=64), dict(width=1, height=1), dict(width=1000, height=3), dict(width=224, height=224)]
BAD_MOTION = [dict(data=0), dict(width=0), dict(height=0), dict(layout=2), dict(dtype=0), dict(dtype=3), dict(planes=0), dict(planes=16),
              dict(planes=3 | 32), dict(fit=2), dict(sampler=2), dict(units=2), dict(per_picture=2), "null"]
GOOD_MOTION = [dict(), dict(dtype=1, layout=1), dict(planes=15), dict(planes=8), dict(fit=1, sampler=1, units=1, per_picture=1)]
BAD_STATS = [dict(data=0), dict(data=0x1004), dict(data=0x1001), dict(source=3), dict(source=2 ** 32 - 1), dict(bins=8), dict(bins=1),
             dict(bins=48), dict(bins=255), dict(bins=512), dict(crop=2), "null"]
GOOD_STATS = [dict(), dict(source=0, bins=0), dict(source=2, bins=16), dict(bins=128)]

# B first, A and B interleaved: the first-use order of the picture list shows; then all kinds of instances at once
INTERLEAVED = [(1,) + BOXES[0], (0,) + BOXES[1], (1,) + BOXES[2], (0,) + BOXES[3], (1,) + BOXES[4], (0,) + BOXES[5], (1,) + BOXES[6], (0,) + BOXES[7]]
EVERY = "ABCDEF"
MIXED = [(i, ) + BOXES[(3 * i + k) % len(BOXES)] for k in range(2) for i in (4, 1, 2, 0, 5, 3)]
NO_PICTURE = [(i, ) + BOXES[i] for i in range(4)]


def _region_cases(e, fits, with_null):
    """the cases the three entries that take regions share; fits: (spec, aux) pairs that cover crop and, where the entry has one, fit"""
    out = []
    for spec, aux in fits:
        out += [case(e, "AB", INTERLEAVED, spec, aux=aux), case(e, EVERY, MIXED, spec, aux=aux), case(e, "CDEF", NO_PICTURE, spec, aux=aux)]
        if with_null:
            out += [case(e, "AB", None, spec), case(e, "BA", None, spec), case(e, EVERY, None, spec), case(e, "CDEF", None, spec)]
    out += [case(e, "AB", []), case(e, "AB", None, nr=0, n=2) if not with_null else case(e, "AB", [], flags=1),
            case(e, "", []), case(e, None, [], n=0), case(e, "", None), case(e, None, None, n=0, flags=15)]
    for flags in (2, 4, 8, 6, 14, 32, 16, 16 | 2, 16 | 12):
        out.append(case(e, EVERY, MIXED, flags=flags))
    out += [case(e, "BA", INTERLEAVED)] * 2                                             # the same call twice
    out += [case(e, "A", [(0,) + b]) for b in BOXES] + [case(e, "B", [(0,) + BOXES[1]] * 3)]
    # refusals
    for d in ("A", "G"):
        out += [case(e, d, [(0,) + b]) for b in BAD_BOXES] + [case(e, d, [(1, 0, 0, 16, 16)]), case(e, d, [(2 ** 32 - 1, 0, 0, 16, 16)])]
        out += [case(e, d, [(0, 0, 0, 16, 16)], flags=1), case(e, d, [(0, 0, 0, 16, 16)], nr=65536), case(e, d, None, nr=2)]
    out += [case(e, "AB", [BAD if k == 5 else INTERLEAVED[k] for k in range(8)]) for BAD in [(0,) + BAD_BOXES[0], (2, 0, 0, 16, 16)]]
    out += [case(e, "", [(0, 0, 0, 16, 16)]), case(e, "", None, nr=65536), case(e, "", None, nr=1)]
    out += [case(e, "G", [(0,) + b]) for b in BOXES[:3]] + [case(e, "G", []), case(e, "AG", [(0, 0, 0, 16, 16)]), case(e, "GA", [(1, 0, 0, 16, 16)])]
    out += [case(e, "AA", [(0, 0, 0, 16, 16), (1, 0, 0, 16, 16)]), case(e, "ABA", [(1, 0, 0, 16, 16)]), case(e, "GG", [(0, 0, 0, 16, 16)]),
            case(e, "BCB", [])]
    out += [case(e, None, [(0, 0, 0, 16, 16)], n=1), case(e, None, [], n=2), case(e, "_", [(0, 0, 0, 16, 16)]), case(e, "A_", [(0, 0, 0, 16, 16)]),
            case(e, "A_", [])]
    return out


def cases():
    out = []
    # ---- h264bsdmiOutputTensorRegions
    out += _region_cases("r", [(dict(crop=crop), aux) for crop in (0, 1) for aux in RESIZES], False)
    out += [case("r", "AB", INTERLEAVED, size, aux=aux) for size in SIZES[1:] for aux in RESIZES[2:]]
    out += [case("r", "BA", INTERLEAVED[:4], dict(crop=crop), colour=c, aux=RESIZES[3]) for crop in (0, 1) for c in COLOURS]
    out += [case("r", "AB", INTERLEAVED[:2], dict(layout=1, dtype=2, channels=3, mean=(0.5, 0.25, 0.125), std=(2, 4, 0.5))),
            case("r", "AB", INTERLEAVED[:2], dict(dtype=0, channels=4))]
    out += [case("r", d, [(0, 0, 0, 16, 16)], aux=bad) for d in ("A", "G", "") for bad in BAD_RESIZES]
    out += [case("r", d, [(0, 0, 0, 16, 16)] if d else [], bad, aux=aux) for d in ("A", "") for bad in BAD_TENSOR for aux in (None, RESIZES[1])]
    out += [case("r", d, [(0, 0, 0, 16, 16)] if d else [], colour=bad) for d in ("A", "") for bad in BAD_COLOURS]
    out += [case("r", "A", None, nr=1), case("r", "", [], aux=RESIZES[4], colour=COLOURS[2])]
    # ---- h264bsdmiOutputTensorRemap
    maps = lambda regions: [(r[0], MAP + 8 * k * (k % 3)) for k, r in enumerate(regions)]      # some maps repeat
    for crop in (0, 1):
        for aux in REMAPS:
            out += [case("m", "AB", maps(INTERLEAVED), dict(crop=crop), aux=aux), case("m", EVERY, maps(MIXED), dict(crop=crop), aux=aux),
                    case("m", "CDEF", maps(NO_PICTURE), dict(crop=crop), aux=aux)]
    out += [case("m", "BA", maps(INTERLEAVED[:4]), dict(crop=crop), colour=c) for crop in (0, 1) for c in COLOURS]
    out += [case("m", "AB", []), case("m", "AB", None, nr=0, n=2), case("m", "", []), case("m", None, [], n=0), case("m", "", None, nr=0),
            case("m", None, None, n=0, nr=0, flags=13)]
    out += [case("m", EVERY, maps(MIXED), flags=f) for f in (4, 8, 12, 32, 16, 16 | 12)] + [case("m", "BA", maps(INTERLEAVED))] * 2
    out += [case("m", "AB", maps(INTERLEAVED[:2]), size) for size in SIZES[1:]]
    for d in ("A", "G"):
        out += [case("m", d, [bad]) for bad in [(1, MAP), (2 ** 32 - 1, MAP), (0, 0), (0, MAP + 4), (0, MAP + 1), (0, MAP + 7)]]
        out += [case("m", d, [(0, MAP)], aux=bad) for bad in BAD_REMAPS]
        out += [case("m", d, [(0, MAP)], flags=1), case("m", d, [(0, MAP)], nr=65536), case("m", d, None, nr=1)]
    out += [case("m", "AB", [(0, MAP), (1, MAP), (2, MAP)]), case("m", "AB", [(0, MAP), (1, MAP + 4), (0, MAP)])]
    out += [case("m", "", [(0, MAP)]), case("m", "", None, nr=65536), case("m", "G", [(0, MAP)], aux=REMAPS[3]), case("m", "G", []),
            case("m", "AG", [(0, MAP)]), case("m", "AA", [(0, MAP), (1, MAP)]), case("m", "ABA", [(1, MAP)]), case("m", None, [(0, MAP)], n=1),
            case("m", None, [], n=2), case("m", "_", [(0, MAP)]), case("m", "A_", [(0, MAP)]), case("m", "A_", [])]
    out += [case("m", d, [(0, MAP)] if d else [], bad, aux=aux) for d in ("A", "") for bad in BAD_TENSOR for aux in (None, REMAPS[1])]
    out += [case("m", d, [(0, MAP)] if d else [], colour=bad) for d in ("A", "") for bad in BAD_COLOURS]
    out += [case("m", "", [], aux=bad) for bad in BAD_REMAPS]
    # ---- h264bsdmiOutputMotionRegions
    out += _region_cases("v", [(dict(crop=crop, fit=fit), None) for crop in (0, 1) for fit in (0, 1)], True)
    out += [case("v", "AB", INTERLEAVED, dict(fit=1, **size)) for size in SIZES[1:]] + [case("v", "BA", None, dict(fit=1, **size)) for size in SIZES[1:]]
    out += [case("v", "AB", INTERLEAVED[:3], good) for good in GOOD_MOTION] + [case("v", "", [], good) for good in GOOD_MOTION]
    out += [case("v", d, [(0, 0, 0, 16, 16)] if d else [], bad) for d in ("A", "G", "") for bad in BAD_MOTION]
    out += [case("v", "H", [(0, 0, 0, 16, 16)]), case("v", "H", None), case("v", "H", []), case("v", "AH", [(0, 0, 0, 16, 16)]),
            case("v", "HB", None), case("v", "G", None)]
    # ---- h264bsdmiOutputRegionStats
    out += _region_cases("s", [(dict(crop=crop), None) for crop in (0, 1)], True)
    out += [case("s", "ABH", [(2, 1, 1, 9, 9), (0,) + BOXES[1], (1,) + BOXES[2]], good) for good in GOOD_STATS]
    out += [case("s", "HBA", None, good) for good in GOOD_STATS] + [case("s", "", [], good) for good in GOOD_STATS]
    out += [case("s", d, [(0, 0, 0, 16, 16)] if d else [], bad) for d in ("A", "G", "") for bad in BAD_STATS]
    out += [case("s", "G", None)]
    return out


def build(csrc, workdir, sanitize=None):
    """the stand-alone program — current_pulls.c and the device stand-in of this tree, the host parser and api.c of `csrc` —
    built with gcc; no HIP, no Python"""
    return host_program.build("current_pulls", workdir, sanitize, csrc)


def run(exe):
    """(records, final): one record per case of cases(), what the instances' queues give at the end; the run must be clean"""
    grid = cases()
    body, final = host_program.run(exe, STREAMS, stdin="".join(c + "\n" for c in grid)).split("#final\n")
    records = ["\n".join(part.split("\n")[1:]) for part in body.split("#")[1:]]
    assert len(records) == len(grid), (len(records), len(grid))
    return records, final


def pin(record):
    return record if len(record) <= TEXT_LIMIT else "sha256:" + hashlib.sha256(record.encode()).hexdigest()


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit("usage: make_current_pull_pins.py <csrc of the commit the pins are taken from> <its name>")
    with tempfile.TemporaryDirectory() as tmp:
        records, final = run(build(os.path.abspath(sys.argv[1]), tmp))
    with open(PINS, "w") as f:
        json.dump({"recorded_from": sys.argv[2], "cases": len(records), "final": final, "pins": [pin(r) for r in records]}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{PINS}: {len(records)} cases from {sys.argv[2]}, {sum(r.startswith('rc=-1') for r in records)} refused, "
          f"{os.path.getsize(PINS)} bytes", file=sys.stderr)
