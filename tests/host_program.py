"""The stand-alone C programs of the host-path tests, built and run in one place: a driver under tests/fuzz_asan/ (on host_harness.h)
and the recording device stand-in (mock_engine.c) with the host parser and api.c, compiled by gcc, plain or with sanitizers, run
directly on the CPU, and its output cut into the named records the drivers print.  No HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264bsd_amd", "csrc")
FUZZ = os.path.join(ROOT, "tests", "fuzz_asan")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST_SOURCES = ("hd_nal.c", "hd_params.c", "hd_slice.c", "hd_dpb.c", "hd_cavlc.c", "hd_resid.c", "hd_mb.c", "hd_core.c", "api.c")
STREAMS = [os.path.join(GOLDEN, n) for n in ("test_640x360.h264", "test_1920x1080.h264")]
SANITIZERS = [None, "address,undefined"]                # the parametrisations of a `records` fixture ...
SANITIZER_IDS = ["plain", "sanitizers"]                 # ... and their ids


def build(driver, workdir, sanitize=None, csrc=CSRC):
    """the program of tests/fuzz_asan/<driver>.c bound to mock_engine.c, with the host sources of `csrc`; returns its path"""
    exe = os.path.join(workdir, driver + ("_" + sanitize.replace(",", "_") if sanitize else ""))
    srcs = [os.path.join(FUZZ, f) for f in (driver + ".c", "mock_engine.c")] + [os.path.join(csrc, f) for f in HOST_SOURCES]
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", f"-I{csrc}", "-DH264BSD_BUILD"]
    if sanitize:
        cmd += [f"-fsanitize={sanitize}", "-fno-omit-frame-pointer"]
    b = subprocess.run(cmd + srcs + ["-lpthread", "-lm", "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(exe, args, stdin=None):
    """the stdout of a run, which must end with 0 and without a sanitizer report"""
    r = subprocess.run([exe] + list(args), input=stdin, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    err = "\n".join(ln for ln in r.stderr.splitlines() if "left shift of negative" not in ln)      # (mirrors the reference's arithmetic)
    assert "ERROR: AddressSanitizer" not in err and "ERROR: LeakSanitizer" not in err and "runtime error" not in err, err[-2000:]
    return r.stdout


def parse(stdout):
    """name -> the lines behind "#name"; "pops": the pop lines in order"""
    out = {"pops": []}
    name = None
    for ln in stdout.splitlines():
        if ln.startswith("pop "):
            out["pops"].append(ln)
        elif ln.startswith("#"):
            name = ln[1:]
            assert name not in out
            out[name] = []
        else:
            out[name].append(ln)
    return out


def records(driver, workdir, sanitize=None, streams=STREAMS):
    """the records of one run of `driver` over `streams`"""
    return parse(run(build(driver, workdir, sanitize), streams))
