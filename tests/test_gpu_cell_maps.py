"""GPU: h264bsdmiOutputCellMaps / pull_cells through the product library.  Beside every decoder runs a twin, a second device decoder fed
the same bytes; both pop in lock-step, the twin through h264bsdNextOutputPicture, whose I420 coded frames are what tests/cells_model.py
computes the maps from.  Everything is an integer: every comparison is an equality."""
import ctypes

import numpy as np
import pytest

import cells_model as clm
import stats_model as sm
from conftest import stream_bytes
from h264writer import StreamWriter
from synth_configs import CONFIGS
from test_gpu_tensor_colour import _synthetic

pytestmark = pytest.mark.gpu

SOURCES = ["y", "ycbcr", "rgb"]
PICTURE_PLANES = ("count", "sum", "sumsq", "min", "max")
CHANGE_PLANES = ("count", "sad", "ssd", "dsum", "dmax", "above")
S32 = 0x5A5A5A5A


@pytest.fixture(autouse=True, scope="module")
def _through_the_product_library(built):
    built.use_product_library(True)
    yield
    built.use_product_library(False)


@pytest.fixture(autouse=True)
def _no_device_errors(built):
    yield
    assert built.device_errors() == 0


def _data(name):
    if isinstance(name, bytes):
        return name
    return StreamWriter(**CONFIGS[name]).build() if name in CONFIGS else stream_bytes(name)


def _cropped():
    """6 x 4 macroblocks, SPS crop (1, 2, 1, 1): the window is 90 x 60 at (2, 2) — no cell is ever tile-aligned, and a dword straddles
    two cells at every cell size"""
    return _synthetic(1, 1, crop=(1, 2, 1, 1))


class Pair:
    """a decoder and its twin, fed the same NAL units.  step(): one more picture decoded by both; pop(): the next output picture of
    both, current in the decoder, as the I420 coded frame from the twin -> picId; keep(): the decoder's current picture becomes its
    kept one, and the twin's frame the model's"""

    def __init__(self, built, *names):
        self.built = built
        self.data = b"".join(_data(n) for n in names)
        self.bufs = [ctypes.create_string_buffer(self.data, len(self.data)) for _ in range(2)]
        self.off = self.n = 0
        self.dec, self.twin = built.Decoder(1), built.Decoder(1)
        self.frame = self.frame_size = self.kept = self.kept_size = None
        self.pic_id = self.kept_id = 0
        self._planes = {}

    def step(self):
        stall = 0
        while self.off < len(self.data) and stall <= 3:
            left = len(self.data) - self.off
            r, rb = self.dec.decode(ctypes.addressof(self.bufs[0]) + self.off, left, pic_id=100 + self.n)
            assert (r, rb) == self.twin.decode(ctypes.addressof(self.bufs[1]) + self.off, left, pic_id=100 + self.n)
            self.off += rb
            stall = stall + 1 if rb == 0 else 0
            if r == self.built.H264BSD_PIC_RDY:
                self.n += 1
                return True
        return False

    def pop(self):
        info, pic = self.dec.next_output_info(), self.twin.next_output_picture()
        assert info is not None and pic is not None and info[1:] == pic[1:]
        self.frame, self.frame_size, self.pic_id = np.array(pic[0], copy=True), self.size(), info[1]
        return info[1]

    def advance(self, pictures):
        for _ in range(pictures):
            assert self.step()
            pic_id = self.pop()
        return pic_id

    def keep(self, stream=None):
        assert self.built.keep_pictures([self.dec], stream=stream) == ([1], [self.pic_id])
        self.kept_now()

    def kept_now(self):
        self.kept, self.kept_size, self.kept_id = self.frame, self.frame_size, self.pic_id

    def size(self):
        return 16 * self.dec.pic_width(), 16 * self.dec.pic_height()

    def window(self, crop):
        W, H = self.size()
        flag, left, cw, top, ch = self.dec.cropping_params()
        return (left, top, cw, ch) if crop and flag else (0, 0, W, H)

    def planes(self, source, kept=False):
        """the channel planes of the current (kept) frame, computed once per frame"""
        frame, size = (self.kept, self.kept_size) if kept else (self.frame, self.frame_size)
        key = (source, id(frame))
        if key not in self._planes:
            self._planes[key] = (frame, sm.channels(frame, *size, source))          # (the frame is held: its id stays its own)
        return self._planes[key][1]

    def want(self, names, source, crop, box, cell, grid, threshold=(0, 0, 0)):
        """the model's slice of `box` (None: the whole window)"""
        mode = clm.CHANGE if set(names) - set(PICTURE_PLANES) else clm.PICTURE
        if mode == clm.CHANGE:
            assert self.kept is not None and self.kept_size == self.frame_size
        window = self.window(crop)
        box = (0, 0) + window[2:] if box is None else box
        return clm.maps(mode, clm.plane_bits(mode, names), self.planes(source), self.planes(source, True) if mode else None, window, box, cell,
                        grid, threshold)

    def close(self):
        self.dec.close()
        self.twin.close()


def _equal(cm, k, want, what=None):
    """slice k of a CellMaps against a model slice"""
    got = cm.maps[k].cpu().numpy().astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, k, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])


def _grid(size, cell):
    return clm.default_grid([(size[1], size[0])], cell)


@pytest.mark.parametrize("pictures", [1, 4])
@pytest.mark.parametrize("source", SOURCES)
def test_whole_windows_of_the_640x360_stream_in_picture_mode(built, source, pictures):
    """picture 0 (intra) and picture 3 (P), crop on (360 rows: the last macroblock row is cut in half, and at cell 16 the last cell row
    is half a cell) and off (the 640 x 368 coded frame), all five cell sizes, all planes"""
    pair = Pair(built, "test_640x360")
    pic_id = pair.advance(pictures)
    for crop in (True, False):
        rows = 360 if crop else 368
        assert pair.window(crop) == (0, 0, 640, rows)
        for cell in clm.CELLS:
            cm = built.pull_cells([pair.dec], None, cell=cell, source=source, planes=PICTURE_PLANES, crop=crop)
            grid = _grid((640, rows), cell)
            assert tuple(cm.maps.shape) == (1, clm.n_maps(0, len(cm.sum[0]), 31)) + grid and cm.maps.dtype.is_signed
            assert cm.got == [1] and cm.current == [1] and cm.pic_id == [pic_id] and cm.kept == [0] and cm.kept_pic_id == [0]
            _equal(cm, 0, pair.want(PICTURE_PLANES, source, crop, None, cell, grid), (source, pictures, crop, cell))
            count = cm.count[0].cpu().numpy()
            assert int(count.sum()) == 640 * rows
            if crop and cell == 16:
                assert (count[-1] == 16 * 8).all() and (count[:-1] == 256).all()       # the last cell row is half a cell
    pair.close()


@pytest.mark.parametrize("source", SOURCES)
def test_the_cropped_synthetic_stream_in_both_modes(built, source):
    """window origin (2, 2), 90 x 60: both modes, all planes, all cell sizes, crop on and off, whole windows and a box with a negative
    origin; the CHANGE calls compare picture 1 with picture 0"""
    pair = Pair(built, _cropped())
    pair.advance(1)
    pair.keep()
    pair.advance(1)
    assert pair.window(True) == (2, 2, 90, 60) and pair.size() == (96, 64)
    thr = (6, 0, 3)
    for crop in (True, False):
        size = pair.window(crop)[2:]
        for cell in clm.CELLS:
            grid = _grid(size, cell)
            boxes = [(0, 0) + size, (-3, 5, 61, 41)]
            regions = [(0,) + b for b in boxes]
            pm = built.pull_cells([pair.dec], regions, cell=cell, source=source, planes=PICTURE_PLANES, crop=crop)
            ch = built.pull_cells([pair.dec], regions, cell=cell, source=source, planes=CHANGE_PLANES, against="kept",
                                  threshold=list(thr)[:1 if source == "y" else 3], crop=crop)
            assert tuple(pm.maps.shape[2:]) == tuple(ch.maps.shape[2:]) == grid
            assert pm.got == ch.got == [1, 1] and ch.kept == [1] and ch.kept_pic_id == [pair.kept_id] and ch.pic_id == [pair.pic_id]
            for k, b in enumerate(boxes):
                _equal(pm, k, pair.want(PICTURE_PLANES, source, crop, b, cell, grid), ("picture", source, crop, cell, b))
                want = pair.want(CHANGE_PLANES, source, crop, b, cell, grid, thr)
                _equal(ch, k, want, ("change", source, crop, cell, b))
                assert want[1].any()                                                   # the guard: the two pictures differ
    pair.close()


# (x, y, w, h) in a 640-wide window of 360 rows: the whole window, one sample, one aligned macroblock, odd everything across a tile
# corner, leaving the window on each side (negative origins included), outside it on either side
BOXES = [(0, 0, 640, 360), (5, 7, 1, 1), (32, 48, 16, 16), (13, 11, 37, 23), (-9, 10, 30, 20), (601, 3, 81, 17), (20, -7, 25, 19),
         (11, 338, 23, 45), (700, 50, 20, 20), (-40, 5, 40, 9)]


@pytest.mark.parametrize("source", ["ycbcr", "y"])
def test_boxes_on_a_fixed_grid(built, source):
    """cols 6, rows 5, cell 8 over the sibling tests' boxes: (13, 11, 37, 23) has a last column 5 wide, a last row 7 tall and empty
    cells beyond; (-9, 10, 30, 20) a first column entirely outside the window and a second 7 wide; the boxes that miss the window are
    all count 0.  Then a grid smaller than the boxes, which truncates."""
    pair = Pair(built, "test_640x360")
    pair.advance(2)
    pair.keep()
    pair.advance(1)
    regions = [(0,) + b for b in BOXES]
    for grid in ((5, 6), (2, 3)):
        pm = built.pull_cells([pair.dec], regions, cell=8, grid=grid, source=source, planes=PICTURE_PLANES)
        ch = built.pull_cells([pair.dec], regions, cell=8, grid=grid, source=source, planes=CHANGE_PLANES, against="kept", threshold=5)
        assert pm.got == ch.got == [1] * len(BOXES) and tuple(pm.maps.shape[2:]) == grid
        for k, b in enumerate(BOXES):
            _equal(pm, k, pair.want(PICTURE_PLANES, source, True, b, 8, grid), ("picture", grid, b))
            _equal(ch, k, pair.want(CHANGE_PLANES, source, True, b, 8, grid, (5, 5, 5)), ("change", grid, b))
        count = pm.count.cpu().numpy()
        if grid == (5, 6):
            assert count[3, 0].tolist() == [64, 64, 64, 64, 40, 0] and count[3, :, 0].tolist() == [64, 64, 56, 0, 0]
            assert count[4, 0].tolist() == [0, 56, 64, 48, 0, 0]
        else:
            assert (count[0] == 64).all() and (count[3] == 64).all()
        assert not count[8].any() and not count[9].any()
        mn, mx = pm.min.cpu().numpy(), pm.max.cpu().numpy()
        assert (mn[8:] == 255).all() and not mx[8:].any() and not ch.maps[8:].any()      # count 0: min 255, max 0; CHANGE all zeros
    pair.close()


@pytest.mark.parametrize("names,against,P", [(("sad",), "kept", 3), (("count", "above"), "kept", 4), (("max",), None, 3)])
def test_plane_subsets_write_their_slices_and_nothing_behind_them(built, names, against, P):
    """ycbcr: ("sad",) is 3 maps, ("count", "above") 1 + 3, ("max",) 3; slice r starts at r * P * rows * cols words; the words behind
    the last slice keep their sentinel"""
    import torch
    pair = Pair(built, _cropped())
    pair.advance(1)
    pair.keep()
    pair.advance(1)
    grid, cell = (7, 11), 8
    boxes = [(0, 0, 90, 60), (7, 3, 50, 31), (200, 0, 8, 8)]
    words = len(boxes) * P * grid[0] * grid[1]
    flat = torch.full((words + 64,), S32, dtype=torch.int32, device="cuda")
    out = flat[:words].view(len(boxes), P, *grid)
    cm = built.pull_cells([pair.dec], [(0,) + b for b in boxes], cell=cell, grid=grid, source="ycbcr", planes=names, against=against,
                          threshold=[2, 0, 1] if against else 0, out=out)
    assert cm.maps is out and cm.got == [1, 1, 1]
    host = flat.cpu().numpy().astype(np.int64)
    assert (host[words:] == S32).all()
    for k, b in enumerate(boxes):
        want = pair.want(names, "ycbcr", True, b, cell, grid, (2, 0, 1))
        assert want.shape[0] == P
        assert np.array_equal(host[k * P * 77:(k + 1) * P * 77].reshape(P, *grid), want), (names, b)
    for name in PICTURE_PLANES + CHANGE_PLANES:
        if hasattr(cm, name):
            assert (getattr(cm, name) is not None) == (name in names), name
    pair.close()


@pytest.mark.parametrize("later", [1, 3])
def test_change_mode_against_a_picture_kept_earlier(built, later):
    """keep at picture 2 of the 640x360 stream, decode and pop 1 or 3 more pictures, compare: per-channel thresholds 0 / 7 / 255"""
    pair = Pair(built, "test_640x360")
    kept_id = pair.advance(3)
    pair.keep()
    pic_id = pair.advance(later)
    for cell in (8, 16):
        grid = _grid((640, 360), cell)
        ch = built.pull_cells([pair.dec], None, cell=cell, source="ycbcr", planes=CHANGE_PLANES, against="kept", threshold=[0, 7, 255])
        assert ch.got == [1] and ch.kept == [1] and ch.pic_id == [pic_id] and ch.kept_pic_id == [kept_id]
        want = pair.want(CHANGE_PLANES, "ycbcr", True, None, cell, grid, (0, 7, 255))
        _equal(ch, 0, want, (later, cell))
        above = ch.above[0].cpu().numpy()
        assert above[0].any() and not above[2].any() and int(ch.sad[0, 0].sum()) > 0
    pair.close()


def test_keep_then_compare_at_once_is_all_zero_except_count(built):
    pair = Pair(built, "plain_ip")
    pic_id = pair.advance(2)
    pair.keep()
    for source in SOURCES:
        ch = built.pull_cells([pair.dec], [(0, 0, 0, 96, 80), (0, 3, 5, 30, 17)], cell=16, source=source, planes=CHANGE_PLANES, against="kept")
        assert ch.got == [1, 1] and ch.pic_id == ch.kept_pic_id == [pic_id]
        count = ch.count.cpu().numpy()
        assert count[0].tolist() == [[256] * 6] * 5 and int(count[1].sum()) == 30 * 17
        assert not ch.maps[:, 1:].any()
    pair.close()


def test_keep_chains_four_consecutive_pictures(built):
    """keep=True: call t gives the maps of the difference to the picture of call t - 1; the first call has nothing to compare with,
    leaves its slice untouched and starts the chain"""
    import torch
    pair = Pair(built, "test_640x360")
    grid = _grid((640, 360), 16)
    for t in range(4):
        pic_id = pair.advance(1)
        out = torch.full((1, 7) + grid, S32, dtype=torch.int32, device="cuda")
        ch = built.pull_cells([pair.dec], None, cell=16, source="ycbcr", planes=("count", "sad", "above"), against="kept", threshold=[4, 2, 2],
                              keep=True, out=out)
        assert ch.current == [1] and ch.pic_id == [pic_id] and ch.maps is out
        if t == 0:
            assert ch.got == [0] and ch.kept == [0] and ch.kept_pic_id == [0] and bool((out == S32).all())
        else:
            assert ch.got == [1] and ch.kept == [1] and ch.kept_pic_id == [pic_id - 1]
            want = pair.want(("count", "sad", "above"), "ycbcr", True, None, 16, grid, (4, 2, 2))
            assert want[1].any()
            _equal(ch, 0, want, t)
        pair.kept_now()
    pair.close()


def test_the_maps_equal_the_siblings_called_with_the_cell_boxes(built):
    """the definition, on the device: every cell of pull_cells is the record (bins 0) pull_stats / pull_change give for its cell box"""
    pair = Pair(built, _cropped())
    pair.advance(1)
    pair.keep()
    pair.advance(1)
    cell, grid = 8, (6, 9)
    for box in ((0, 0, 90, 60), (-5, 3, 47, 40)):
        cells = [(i, j) for i in range(grid[0]) for j in range(grid[1])]
        real = [(i, j) for i, j in cells if min(clm.cell_box(box, cell, i, j)[2:]) > 0]
        regions = [(0,) + clm.cell_box(box, cell, i, j) for i, j in real]
        at = ([i for i, _ in real], [j for _, j in real])
        for source in ("ycbcr", "rgb"):
            pm = built.pull_cells([pair.dec], [(0,) + box], cell=cell, grid=grid, source=source, planes=PICTURE_PLANES)
            st = built.pull_stats([pair.dec], regions, source=source, bins=0)
            ch = built.pull_cells([pair.dec], [(0,) + box], cell=cell, grid=grid, source=source, planes=CHANGE_PLANES, against="kept", threshold=[3, 1, 0])
            rc = built.pull_change([pair.dec], regions, source=source, bins=0, threshold=[3, 1, 0])
            assert st.got == rc.got == [1] * len(regions)
            for maps, recs, names in ((pm, st, (("count", "count"), ("sum", "sum"), ("sumsq", "sumsq"), ("min", "min"), ("max", "max"))),
                                      (ch, rc, (("count", "count"), ("sad", "sad"), ("ssd", "ssd"), ("dsum", "sum"), ("dmax", "max"), ("above", "above")))):
                for mine, theirs in names:
                    a = getattr(maps, mine)[0].cpu().numpy().astype(np.int64)
                    b = getattr(recs, theirs).cpu().numpy().astype(np.int64)
                    if mine == "count":
                        assert np.array_equal(a[at], b), (box, source, mine)
                        assert int(a.sum()) == int(b.sum())                    # the cells beyond the box hold nothing
                    else:
                        assert np.array_equal(a[:, at[0], at[1]].T, b), (box, source, mine)
    pair.close()


@pytest.mark.parametrize("against", [None, "kept"])
def test_four_instances_of_different_sizes_in_one_call(built, against):
    """regions=None with the grid of the largest window: 640x360, 1080p, the cropped synthetic stream and one that has not popped, whose
    slice keeps the sentinel (got 0); in CHANGE mode the same holds for the synthetic one, which has kept nothing"""
    import torch
    pairs = [Pair(built, "test_640x360"), Pair(built, "test_1920x1080"), Pair(built, _cropped()), Pair(built, "plain_ip")]
    for i, p in enumerate(pairs[:3]):
        p.advance(1)
        if against and i != 2:
            p.keep()
            p.advance(1)
    assert pairs[3].step()                                       # decoded, not popped: no current picture
    names = CHANGE_PLANES if against else ("count", "sum", "min")
    cell, grid = 32, (34, 60)
    auto = built.pull_cells([p.dec for p in pairs], None, cell=cell, source="ycbcr", planes=names, against=against)
    assert tuple(auto.maps.shape[2:]) == grid                    # ceil(1080 / 32), ceil(1920 / 32)
    P = auto.maps.shape[1]
    out = torch.full((4, P) + grid, S32, dtype=torch.int32, device="cuda")
    cm = built.pull_cells([p.dec for p in pairs], None, cell=cell, grid=grid, source="ycbcr", planes=names, against=against, out=out)
    have = [1, 1, 0 if against else 1, 0]
    assert cm.got == have and cm.current == [1, 1, 1, 0] and cm.kept == ([1, 1, 0, 0] if against else [0] * 4)
    assert cm.pic_id == [p.pic_id for p in pairs[:3]] + [0]
    for k, p in enumerate(pairs):
        if have[k]:
            _equal(cm, k, p.want(names, "ycbcr", True, None, cell, grid), (against, k))
            assert bool(torch.equal(auto.maps[k], out[k]))
        else:
            assert bool((out[k] == S32).all())
    for p in pairs:
        p.close()


def test_one_region_over_many_workgroups_and_one_in_a_single_workgroup(built):
    """A workgroup owns 128 x 64 luma samples of the grid: at cell 4 that is 32 x 16 cells, so the 480 x 270 cells of one 1080p window
    are 15 rectangles across and 17 down (16.875: the last row of rectangles holds 14 of its 16 cell rows) — one region split over 255
    workgroups along both axes.  With the whole window the rectangle borders fall between macroblocks; the box at (5, 3) then moves
    every border into the macroblocks, so that each border tile is read by the two or four workgroups that share it, each masking what
    is not its own.  cols 6, rows 5 at cell 8 is 48 x 40 samples, less than one rectangle: a single workgroup."""
    pair = Pair(built, "test_1920x1080")
    pair.advance(1)
    grid = (270, 480)
    cm = built.pull_cells([pair.dec], None, cell=4, source="y", planes=("count", "sum"))
    assert tuple(cm.maps.shape) == (1, 2) + grid
    _equal(cm, 0, pair.want(("count", "sum"), "y", True, None, 4, grid), "1080p at cell 4")
    box = (5, 3, 1900, 1070)
    cm = built.pull_cells([pair.dec], [(0,) + box], cell=4, grid=grid, source="y", planes=("count", "sum"))
    _equal(cm, 0, pair.want(("count", "sum"), "y", True, box, 4, grid), "1080p at cell 4, off the tiles")
    one = built.pull_cells([pair.dec], [(0, 700, 500, 48, 40)], cell=8, grid=(5, 6), source="y", planes=("count", "sum"))
    _equal(one, 0, pair.want(("count", "sum"), "y", True, (700, 500, 48, 40), 8, (5, 6)), "one workgroup")
    assert (one.count.cpu().numpy() == 64).all()
    pair.close()


def test_a_side_stream_orders_itself_with_the_next_decode(built):
    """a call on a torch side stream, then the next picture decoded and popped with no host wait in between: after the stream is
    synchronised the maps are those of the picture that was current at the call"""
    import torch
    twin = Pair(built, "test_640x360")                      # the frames first, from a pair of its own
    frames = []
    for _ in range(3):
        twin.advance(1)
        frames.append(twin.frame)
    twin.close()
    data = _data("test_640x360")
    buf = ctypes.create_string_buffer(data, len(data))
    dec, off = built.Decoder(1), 0

    def picture(k):
        nonlocal off
        r = stall = 0
        while r != built.H264BSD_PIC_RDY and stall <= 3:
            r, rb = dec.decode(ctypes.addressof(buf) + off, len(data) - off, pic_id=100 + k)
            off += rb
            stall = stall + 1 if rb == 0 else 0
        assert r == built.H264BSD_PIC_RDY
        assert dec.next_output_info()[1] == 100 + k

    side = torch.cuda.Stream()
    grid = _grid((640, 360), 16)
    picture(0)
    first = built.pull_cells([dec], None, cell=16, source="ycbcr", planes=PICTURE_PLANES, stream=side)
    picture(1)
    second = built.pull_cells([dec], None, cell=16, source="ycbcr", planes=PICTURE_PLANES, stream=side)
    picture(2)
    assert first.got == second.got == [1] and first.pic_id == [100] and second.pic_id == [101]
    side.synchronize()
    for cm, frame in ((first, frames[0]), (second, frames[1])):
        planes = sm.channels(frame, 640, 368, "ycbcr")
        _equal(cm, 0, clm.maps(clm.PICTURE, 31, planes, None, (0, 0, 640, 360), (0, 0, 640, 360), 16, grid))
    dec.close()


def test_raw_calls_that_need_a_live_decoder_are_refused_and_write_nothing(built):
    import torch
    from test_tensor_output import _capture_until_output
    pair = Pair(built, "plain_ip")
    pair.advance(2)
    capture, keep_alive = _capture_until_output(built)
    L = built.api_lib()
    grid, words = (5, 6), 2 * 2 * 30
    out = torch.full((words + 8,), S32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    S = 0xA5A5A5A5

    def call(decs, regions, mode=0, planes=3):
        regs = (built.Region * 2)(*[built.Region(*r) for r in regions])
        spec = built.CellsSpec(out.data_ptr(), grid[1], grid[0], 16, 0, 1, mode, planes, (ctypes.c_uint32 * 3)(0, 0, 0), 0)
        arrays = [(ctypes.c_uint32 * 2)(S, S) for _ in range(5)]
        rc = L.h264bsdmiOutputCellMaps(len(decs), (ctypes.c_void_p * len(decs))(*decs), 2, regs, ctypes.byref(spec), None, *arrays)
        return rc, [list(a) for a in arrays]

    good = [(0, 0, 0, 96, 80), (0, 10, 10, 16, 16)]
    untouched = (-1, [[S, S]] * 5)
    assert call([pair.dec._st, pair.dec._st], good) == untouched                      # repeated instances
    assert call([pair.dec._st, capture._st], good) == untouched                       # an instance in capture mode
    assert call([pair.dec._st], [good[0], (1, 0, 0, 16, 16)]) == untouched            # an instance index >= n
    assert call([pair.dec._st], good, mode=1, planes=64) == untouched
    torch.cuda.synchronize()
    assert bool((out == S32).all())
    rc, arrays = call([pair.dec._st], good)                                           # and the accepted call, on the library's own stream
    assert rc == 0 and arrays[0] == [1, 1] and arrays[1][0] == 1 and arrays[2][0] == 0 and arrays[3][0] == pair.pic_id
    host = out.cpu().numpy().astype(np.int64)
    assert (host[words:] == S32).all()
    for k, b in enumerate(good):
        assert np.array_equal(host[k * 60:(k + 1) * 60].reshape(2, *grid), pair.want(("count", "sum"), "y", True, b[1:], 16, grid)), b
    capture.close()
    pair.close()
