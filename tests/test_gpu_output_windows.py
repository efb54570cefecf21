"""Where pictures leave the device: h264bsdmiNextOutputPictureDevice on cropped windows (k_output, k_detile: kernels/k_pixels_io.hip.h)
and the colour conversion of pictures one or two macroblocks wide (conv_pic, kernels/convert.hip.h), against tests/output_window_model.py.

Every stream is all I_PCM (tests/pcm_pictures.py) with uniformly random samples, so every expected byte is a slice of the chosen picture
or the reference's formula on it, and every comparison is exact.  The windows are the smallest at which k_output can go wrong: its
one-sample-per-lane half (window width 2 mod 4), x0 and y0 other than 0, quads and chroma pairs that straddle tile seams, a window of
one chroma sample, more than one trip of each loop.  The narrow pictures take conv_pic's ppr == 1 branch and ppr == 2, with fewer tile
pairs than one batch, through every caller: k_convert_tiles, k_convert_rest and the wavefronts of k_frame_dbk.  The GPU tests go
through the product library, the replay ones through the harness library, which alone has the replay exports."""
import ctypes
import os
import re

import numpy as np
import pytest

import output_window_model as ow
import pcm_pictures as pp
from conftest import ROOT
from oracle import pyoracle
from test_gpu_tensor_colour import Feed

CSRC = os.path.join(ROOT, "h264bsd_amd", "csrc")


# ------------------------------------------------------------------ without a GPU: what the cases reach
def _all_pulls():
    """(case, fmt, window) of every device pull of the window tests"""
    out = []
    for c in ow.CASES + [ow.BIG]:
        for fmt in range(4) if c is not ow.BIG else (3, 1):
            out.append((c, fmt, c.window))
            if c.uncropped:
                out.append((c, fmt, ow.coded_window(c)))
    return out


def test_classifier_mirrors_the_source():
    kernels = open(os.path.join(CSRC, "kernels", "k_pixels_io.hip.h")).read()
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    convert = open(os.path.join(CSRC, "kernels", "convert.hip.h")).read()
    assert kernels.count(ow.K_OUTPUT_BRANCH) == 1
    assert engine.count(ow.K_OUTPUT_GRID) == 1 and engine.count(ow.K_OUTPUT_ITEMS) == 1
    assert int(re.search(r"#define CONV_BATCH_N (\d+)", convert).group(1)) == ow.CONV_BATCH
    assert "c.ppr == 1u ? 0u : 0xFFFFFFFFu / c.ppr + 1u" in convert


def test_cases_reach_the_paths_they_are_for():
    seen = [(c, fmt, window, ow.reach(fmt, window, (16 * c.wmb, 16 * c.hmb))) for c, fmt, window in _all_pulls()]
    small = [r for c, _, _, r in seen if c is not ow.BIG]
    assert any(r.kernel == "k_detile" for r in small)
    for path in ("sample_i420", "sample_conv", "quad_i420", "quad_conv"):
        assert any(r.path == path for r in small), path
        assert any(r.path == path and r.grid > 2 for r in small), path               # more than one workgroup with work
    assert any(r.path == "quad_i420" and r.luma_seam for r in small) and any(r.path == "quad_conv" and r.luma_seam for r in small)
    assert any(r.path == "quad_i420" and r.chroma_seam for r in small) and any(r.path == "quad_conv" and r.chroma_seam for r in small)
    assert any(r.path == "quad_i420" and not r.luma_seam and not r.chroma_seam for r in small)
    for path in ("sample_i420", "sample_conv"):
        assert any(r.path == path and r.trips > 1 for r in small), path
    # the converted quad path has as many items as the grid was sized for (w h / 4), so it loops only on a capped grid: that second
    # trip is test_gpu_chosen_content's cube.  The I420 quad path has w h / 2 items (w h / 4 luma quads, w h / 4 chroma pairs) on a
    # grid sized for 3 w h / 8: its lanes make a second trip from about 2048 items on, and on the capped grid of the large window
    assert not any(r.path == "quad_conv" and r.trips > 1 for r in small)
    assert any(r.path == "quad_i420" and r.trips == 2 and r.grid < 2048 for r in small)
    big = {fmt: r for c, fmt, _, r in seen if c is ow.BIG}
    assert big[3].path == "quad_i420" and big[3].grid == 2048 and big[3].trips == 2 and big[3].luma_seam and big[3].chroma_seam
    assert big[3].items == 1034640 and 1916 * 1080 * 3 // 8 == 775980 > 2047 * 256
    assert big[1].path == "quad_conv" and big[1].trips == 1
    assert any(r.one_chroma_sample for r in small)
    # the windows of single cases
    by_window = {(c.window, fmt): r for c, fmt, w, r in seen if w == c.window}
    assert by_window[(14, 14, 4, 4), 3].luma_seam and by_window[(14, 14, 4, 4), 3].chroma_seam and by_window[(14, 14, 4, 4), 3].items == 8
    assert by_window[(0, 0, 2, 2), 3].items == 6 and by_window[(0, 0, 2, 2), 0].items == 4
    assert by_window[(2, 2, 138, 72), 3].trips == 4 and by_window[(2, 0, 140, 80), 3].grid > 2
    assert by_window[(0, 0, 48, 16), 3].kernel == "k_detile" and by_window[(0, 0, 48, 16), 0].path == "quad_conv"


def test_narrow_sizes_reach_the_pair_counts_they_are_for():
    got = [ow.pairs(w, h) for w, h in ow.NARROW]
    assert [p[2] for p in got] == [1, 1, 3, 9, 17, 4, 6]
    assert {p[0] for p in got} == {1, 2} and {p[1] for p in got} == {0, 0x80000000}
    counts = [p[2] for p in got]
    assert 1 in counts and any(1 < n < ow.CONV_BATCH for n in counts) and any(ow.CONV_BATCH < n <= 2 * ow.CONV_BATCH for n in counts)
    assert any(n > 2 * ow.CONV_BATCH for n in counts)                           # three batches
    assert any(w & 1 and w > 1 for w, _ in ow.NARROW)                           # a last pair without a right-hand tile behind a whole one


@pytest.mark.parametrize("case", ow.CASES + [ow.BIG], ids=ow.case_id)
def test_streams_report_the_windows_of_the_table(built, case):
    """capture mode alone: the host parser accepts the stream and reports the window"""
    n = 1 if case is ow.BIG else 3
    jobs, _, info = built.capture_stream(pp.pcm_stream(ow.pictures(case, n), crop=case.crop, idc=0))
    assert len(jobs) == n and (info["width_mbs"], info["height_mbs"]) == (case.wmb, case.hmb)
    x0, y0, w, h = case.window
    assert info["cropping"] == ((1, x0, w, y0, h) if case.crop is not None else (0, 0, 0, 0, 0))
    if case.crop is None:
        assert case.window == ow.coded_window(case)


@pytest.mark.parametrize("size", ow.NARROW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("idc", [0, 1])
def test_narrow_jobs_alternate_frame_buffers(built, size, idc):
    """what the replay test relies on: four jobs in frame buffers 1, 0, 1, 0 (so every tick can host the conversion of the picture
    before it), filtered pictures for idc 0 and unfiltered ones for idc 1"""
    heads = [pyoracle.blob_header(j) for j in _narrow_jobs(built, size, idc)[1]]
    assert [h["cur_slot"] for h in heads] == [1, 0, 1, 0]
    assert [h["any_deblock"] for h in heads] == [1 - idc] * 4


def _narrow_case(size):
    return ow.Case(size[0], size[1], None, (0, 0, 16 * size[0], 16 * size[1]), False)


def _narrow_jobs(built, size, idc):
    pics = ow.pictures(_narrow_case(size), 4, tag=7)
    jobs, _, info = built.capture_stream(pp.pcm_stream(pics, idc=idc))
    assert len(jobs) == 4 and (info["width_mbs"], info["height_mbs"]) == size
    return pics, jobs


# ------------------------------------------------------------------ on the GPU
@pytest.fixture
def product(built):
    """the product library for the test's decoders; no tripwire of the kernels has fired when the test ends"""
    built.use_product_library(True)
    try:
        yield built
        assert built.device_errors() == 0
    finally:
        built.use_product_library(False)


def _same(got, want, fmt, window, what):
    """two flat arrays, equal; on failure: how many elements differ and the first ones as (plane, x, y, got, want)"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        first = [ow.where(fmt, window, int(i)) + (hex(int(got[i])), hex(int(want[i]))) for i in at[:8]]
        print(f"MISMATCH {what}: {at.size} of {got.size} differ, first {first}")
        raise AssertionError((what, at.size, first))


def _flat(t, fmt):
    """the bytes of a device tensor as want() lays them out"""
    a = t.cpu().numpy().reshape(-1)
    return a if fmt == 3 else a.view(np.uint32)


def _check_pull(got, fmt, picture, window, meta, what):
    assert got is not None, what
    t, pid, idr, err = got
    _, _, w, h = window
    assert t.is_cuda and tuple(t.shape) == ((h * 3 // 2, w) if fmt == 3 else (h, w, 4)), (what, tuple(t.shape))
    assert (pid, idr, err) == meta, (what, (pid, idr, err), meta)
    _same(_flat(t, fmt), ow.want(fmt, picture, window), fmt, window, what)


def _run_windows(built, case, n_pics, fmts):
    pics = ow.pictures(case, n_pics)
    data = pp.pcm_stream(pics, crop=case.crop, idc=0)
    twin = Feed(built, data)
    pulls = [(fmt, crop, Feed(built, data)) for crop in ((True, False) if case.uncropped else (True,)) for fmt in fmts]
    try:
        for k, pic in enumerate(pics):
            assert twin.step()
            frame = twin.dec.next_output_picture()
            assert frame is not None and np.array_equal(frame[0], pp.i420(pic)), (ow.case_id(case), k)
            assert frame[3] == 0
            for fmt, crop, feed in pulls:
                assert feed.step()
                if k == 0:
                    x0, y0, w, h = case.window
                    assert feed.dec.cropping_params() == ((1, x0, w, y0, h) if case.crop is not None else (0, 0, 0, 0, 0))
                window = case.window if crop else ow.coded_window(case)
                _check_pull(feed.dec.next_output_picture_device(fmt, crop=crop), fmt, pic, window, frame[1:], (ow.case_id(case), fmt, crop, k))
                assert feed.dec.next_output_picture_device(fmt, crop=crop) is None
    finally:
        twin.close()
        for _, _, feed in pulls:
            feed.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ow.CASES, ids=ow.case_id)
def test_windows(product, case):
    """three pictures per case, one decoder per format (and per crop flag where the case is also pulled uncropped): shape, picId /
    isIdr / numErrMbs against a twin decoder's h264bsdNextOutputPicture, the twin's frame against the chosen picture (k_detile at
    these sizes), the tensor's bytes against the model"""
    _run_windows(product, case, 3, range(4))


@pytest.mark.gpu
def test_second_trip_of_the_i420_quad_loop(product):
    """one picture of 120 x 68 macroblocks cropped to 1916 x 1080 at (2, 0): 1,034,640 items on the capped grid of 2048 workgroups,
    so nearly every lane of the I420 quad path makes a second trip, with straddling quads and chroma pairs; BGRA of the same window"""
    _run_windows(product, ow.BIG, 1, (3, 1))


def _raw_pull(built, dec, fmt, crop=True):
    pic = built.capi.DevicePicture()
    rc = built.api_lib().h264bsdmiNextOutputPictureDevice(dec._st, fmt, 1 if crop else 0, ctypes.byref(pic))
    return rc, pic


def _device_bytes(addr, n):
    """a writable torch view of n bytes of device memory at addr"""
    import torch

    class _Buf:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (addr, False), "version": 2}
    return torch.as_tensor(_Buf(), device="cuda")


@pytest.mark.gpu
def test_the_fields_of_the_device_picture(product):
    """the library entry point itself on the 9 x 5 stream: return values, width, height, format and pitch (w for I420, 4 w else)"""
    case = ow.SMALL
    x0, y0, w, h = case.window
    pics = ow.pictures(case, 4)
    feed = Feed(product, pp.pcm_stream(pics, crop=case.crop, idc=0))
    try:
        for fmt, pic in enumerate(pics):
            assert feed.step()
            rc, out = _raw_pull(product, feed.dec, fmt)
            assert rc == 1 and (out.width, out.height, out.format) == (w, h, fmt) and out.pitch == (w if fmt == 3 else 4 * w)
            assert (out.picId, out.isIdrPic, out.numErrMbs) == (0, 1, 0) and out.data
            n = w * h * 3 // 2 if fmt == 3 else w * h * 4
            _same(_flat(_device_bytes(out.data, n), fmt), ow.want(fmt, pic, case.window), fmt, case.window, ("raw", fmt))
            rc, _ = _raw_pull(product, feed.dec, fmt)
            assert rc == 0
    finally:
        feed.close()


@pytest.mark.gpu
def test_formats_in_turn_on_one_instance(product):
    """six pictures of the 9 x 5 stream through ONE decoder as I420, RGBA, the uncropped I420 frame, YCbCrA, BGRA, I420: k_output and
    k_detile take turns on the instance's one conversion buffer, whose layout changes from pull to pull"""
    case = ow.SMALL
    pics = ow.pictures(case, 6, tag=1)
    feed = Feed(product, pp.pcm_stream(pics, crop=case.crop, idc=0))
    try:
        for k, (pic, (fmt, crop)) in enumerate(zip(pics, [(3, True), (0, True), (3, False), (2, True), (1, True), (3, True)])):
            assert feed.step()
            window = case.window if crop else ow.coded_window(case)
            _check_pull(feed.dec.next_output_picture_device(fmt, crop=crop), fmt, pic, window, (0, 1, 0), ("in turn", k, fmt, crop))
    finally:
        feed.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [3, 0])
def test_nothing_is_written_behind_the_window(product, fmt):
    """The engine allocates an instance's conversion buffer once, 16 wmb x 16 hmb x 4 bytes (sink_fetch_device, engine.hip).  After
    picture 0 the whole allocation is filled with 0xA5; picture 1 comes back at the same address, its window equals the model, and
    every byte from the end of the output to the end of the allocation still reads 0xA5."""
    import torch
    case = ow.SMALL
    _, _, w, h = case.window
    pics = ow.pictures(case, 2, tag=2)
    total = 16 * case.wmb * 16 * case.hmb * 4
    n = w * h * 3 // 2 if fmt == 3 else w * h * 4
    assert n < total
    feed = Feed(product, pp.pcm_stream(pics, crop=case.crop, idc=0))
    try:
        assert feed.step()
        rc, first = _raw_pull(product, feed.dec, fmt)
        assert rc == 1
        view = _device_bytes(first.data, total)
        _same(_flat(view[:n], fmt), ow.want(fmt, pics[0], case.window), fmt, case.window, ("picture 0", fmt))
        view.fill_(0xA5)
        torch.cuda.synchronize()
        assert feed.step()
        rc, second = _raw_pull(product, feed.dec, fmt)
        assert rc == 1 and second.data == first.data
        got = view.cpu().numpy()
        _same(got[:n] if fmt == 3 else got[:n].view(np.uint32), ow.want(fmt, pics[1], case.window), fmt, case.window, ("picture 1", fmt))
        behind = np.flatnonzero(got[n:] != 0xA5)
        assert behind.size == 0, (fmt, behind.size, (behind[:8] + n).tolist())
    finally:
        feed.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ow.NARROW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_narrow_pictures_through_the_converted_output_entry_points(product, size):
    """h264bsdNextOutputPictureRGBA / BGRA / YCbCrA (k_convert_tiles into the host mirror), h264bsdmiNextOutputPictureDevice in the
    same format (k_output on the whole frame) and the stateless h264bsdConvertTo* on four random pictures, each against the formula"""
    case = _narrow_case(size)
    W, H = case.window[2:]
    pics = ow.pictures(case, 4, tag=7)
    data = pp.pcm_stream(pics, idc=0)
    for fmt in range(3):
        host, dev = Feed(product, data), Feed(product, data)
        try:
            for k, pic in enumerate(pics):
                want = ow.want(fmt, pic, case.window)
                assert host.step() and dev.step()
                got = host.dec.next_output_picture_converted(fmt)
                assert got is not None and got[1:] == (0, 1, 0)
                _same(got[0], want, fmt, case.window, ("host", size, fmt, k))
                _check_pull(dev.dec.next_output_picture_device(fmt), fmt, pic, case.window, (0, 1, 0), ("device", size, fmt, k))
                _same(product.convert(fmt, W, H, pp.i420(pic)), want, fmt, case.window, ("stateless", size, fmt, k))
        finally:
            host.close()
            dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ow.NARROW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("idc", [0, 1])
def test_narrow_pictures_through_the_replay_conversions(built, size, idc):
    """The hosted conversion (set_convert, trailing=False, ticks 0 .. k + 1) and the conversion launch (rep.convert: k_convert_tiles)
    of pictures 0 .. 2 on three replay streams, every format, each against the formula.  Consecutive pictures lie in different frame
    buffers, so every tick hosts the conversion of the picture before it and rep.convert_timings() reports no conversion launch
    (asserted for both idc).  idc 0: every tick launches k_frame_dbk (asserted through rep.timings()), whose wavefronts convert;
    idc 1: no tick does, and k_convert_rest converts."""
    pics, jobs = _narrow_jobs(built, size, idc)
    case = _narrow_case(size)
    W, H = case.window[2:]
    heads = [pyoracle.blob_header(j) for j in jobs]
    assert [h["cur_slot"] for h in heads] == [1, 0, 1, 0] and [h["any_deblock"] for h in heads] == [1 - idc] * 4
    streams = 3
    errs_before = built.device_error_events()
    rep = built.Replay(jobs, n_streams=streams)
    try:
        for fmt in range(3):
            for k in range(3):
                want = ow.want(fmt, pics[k], case.window)
                rep.set_convert(fmt, trailing=False)
                rep.run(0, k + 2); rep.sync()
                _, launches = rep.convert_timings()
                assert launches == 0
                assert rep.timings()["k_frame_dbk"][1] == ((k + 2) if idc == 0 else 0)
                for s in range(streams):
                    _same(rep.fetch_converted(s, W * H), want, fmt, case.window, ("hosted", size, idc, fmt, k, s))
                rep.set_convert(-1)
                rep.run(0, k + 1)
                rep.convert(heads[k]["cur_slot"], fmt)
                for s in range(streams):
                    _same(rep.fetch_converted(s, W * H), want, fmt, case.window, ("launch", size, idc, fmt, k, s))
                    assert np.array_equal(rep.fetch(s, heads[k]["cur_slot"]), pp.i420(pics[k])), (size, idc, k, s)
        assert built.device_error_events() == errs_before
    finally:
        rep.close()
