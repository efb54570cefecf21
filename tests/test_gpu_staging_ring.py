"""GPU: the two-half pinned staging ring (Staged, h264bsd_amd/csrc/hip_owned.h) growing while launches that read it are in flight —
the ring of the tensor pulls' items (Engine) and the ring of k_motion_keep's items (Lane).  Where a ring stands depends on
everything the process did before, so each case runs in a process of its own, on the smallest stream tests/h264writer.py makes
(4 x 3 macroblocks): the first allocation and each growth then fall where the case says."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _stream():
    from h264writer import StreamWriter
    return StreamWriter(n_pics=3).build()


def _pulls(built):
    """One decoder, one popped picture; pull_regions with 8, 300 and 700 boxes of 8 x 8 back to back on one busy stream, no host
    wait in between.  The first call allocates 2 x 256 items, the second grows the ring to 300 while the first is in flight, the
    third to 700.  Each result is, bit for bit, the same boxes pulled in chunks of at most 128 (which fit every ring)."""
    import numpy as np
    import torch
    data = _stream()
    buf = ctypes.create_string_buffer(data, len(data))
    dec = built.Decoder(1)
    off = 0
    while True:
        r, rb = dec.decode(ctypes.addressof(buf) + off, len(data) - off)
        off += rb
        assert r < built.H264BSD_ERROR and off <= len(data)
        if r == built.H264BSD_PIC_RDY:
            break
    assert dec.next_output_info() is not None
    W, H = 16 * dec.pic_width(), 16 * dec.pic_height()
    rng = np.random.default_rng(700)
    kw = dict(dtype=torch.uint8, mode="bilinear", pad=(0.25, 114 / 255, 1.0))
    calls = []
    for k in (8, 300, 700):                                # boxes inside, across every edge, some wholly outside
        regions = [(0, int(x), int(y), 8, 8) for x, y in zip(rng.integers(-10, W + 4, k), rng.integers(-10, H + 4, k))]
        calls.append((regions, torch.zeros((k, 3, 8, 8), dtype=torch.uint8, device="cuda")))
    side = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(10):
            big = (big @ big).clamp_(-1, 1)                 # the pulls queue up behind this while the host runs ahead
    for regions, out in calls:
        _, got, _, cur, _ = built.pull_regions([dec], regions, 8, out=out, stream=side, **kw)
        assert got == [1] * len(regions) and cur == [1]
    side.synchronize()
    for regions, out in calls:
        want = torch.cat([built.pull_regions([dec], regions[i:i + 128], 8, **kw)[0] for i in range(0, len(regions), 128)])
        assert torch.equal(out, want), len(regions)
    assert len({bytes(c[1][k].cpu().numpy().tobytes()) for c in calls for k in range(len(c[0]))}) > 100      # (the boxes do differ)
    dec.close()


def _motion(built):
    """One lane (H264BSDMI_LANES=1,0: a flush is one tick per round).  70 decoders with motion export decode a picture in one flush:
    the tick keeps 70 items, the ring's first allocation is 2 x 140.  Then all 70 and 80 more decode in one flush: the tick keeps
    150 items and the ring grows to 2 x 300 behind the first tick's launch.  Every decoder's motion field is the model's."""
    import numpy as np
    import torch
    import motion_model as mm
    from test_gpu_motion_tensor import Pair, _hwc
    data = _stream()
    planes = ("mv", "valid", "age", "qp")

    def check(pairs):
        for p in pairs:
            assert p.step()
        pops = [p.pop() for p in pairs]
        t, got, _, cur, ids = built.pull_motion([p.dec for p in pairs], crop=False, dtype=torch.float32, planes=planes)
        assert got == [1] * len(pairs) and cur == [1] * len(pairs) and ids == [pop[1] for pop in pops]
        wants = {}
        for k, (p, pop) in enumerate(zip(pairs, pops)):
            if pop not in wants:                            # the decoders share the stream: one model answer per (frame buffer, picture)
                window = p.window(False)
                wants[pop] = mm.motion_region(p.side(pop[0]), window, (0, 0, window[2], window[3]), mm.native_size(window))[1]
            assert np.array_equal(_hwc(t, k, "NCHW"), wants[pop]), (k, pop)
        return wants

    first = [Pair(built, data) for _ in range(70)]
    assert len(check(first)) == 1
    more = [Pair(built, data) for _ in range(80)]
    wants = check(first + more)
    assert len(wants) == 2 and any(w[..., 2].any() for w in wants.values())      # the second picture does carry vectors
    for p in first + more:
        p.close()


def _fresh_process(case, **env):
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), case],
                       cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{case} ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_pull_ring_grows_under_calls_in_flight():
    _fresh_process("pulls")


def test_motion_keep_ring_grows_between_two_ticks():
    _fresh_process("motion", H264BSDMI_LANES="1,0")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import h264bsd_amd
    h264bsd_amd.build()
    h264bsd_amd.use_product_library(True)
    {"pulls": _pulls, "motion": _motion}[sys.argv[1]](h264bsd_amd)
    assert h264bsd_amd.device_errors() == 0
    print(sys.argv[1], "ok")
