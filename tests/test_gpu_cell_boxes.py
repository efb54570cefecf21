"""GPU: h264bsdmiOutputCellBoxes / pull_boxes through the product library.  Every call is checked three ways: the maps tensor equals
what pull_cells gives for the same arguments on the same pictures; the boxes tensor equals tests/boxes_model.py applied to that map;
and the device reported no error.  Both output tensors are prefilled with a sentinel, so "the whole slice is written" and "the slice is
untouched" are both visible.  Everything is an integer: every comparison is an equality.  The patterns are all-I_PCM pictures
(tests/pcm_pictures.py) whose luma is 255 in chosen cells and 0 elsewhere, read in PICTURE mode through the plane "max" at level 0."""
import ctypes

import numpy as np
import pytest

import boxes_model as bm
from pcm_pictures import pcm_stream
from test_gpu_cell_maps import Pair, _cropped

pytestmark = pytest.mark.gpu

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


def _check(built, pairs, regions, cell, planes, grid=None, source="y", against=None, threshold=0, crop=True, plane=None, channel=0, level=0,
           sense="above", connectivity=8, min_cells=1, max_boxes=64, keep=False, stream=None):
    """pull_cells, then pull_boxes with the same arguments into sentinel-filled tensors -> (CellBoxes, its boxes on the host as unsigned
    words); the three checks of the module's docstring on every slice"""
    import torch
    decs = [p.dec for p in pairs]
    cells_kw = dict(cell=cell, grid=grid, source=source, planes=planes, against=against, threshold=threshold, crop=crop, stream=stream)
    cm = built.pull_cells(decs, regions, **cells_kw)
    R, M = cm.maps.shape[0], max_boxes
    out = torch.full(tuple(cm.maps.shape), S32, dtype=torch.int32, device="cuda")
    bout = torch.full((R, 1 + M, 8), S32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cb = built.pull_boxes(decs, regions, plane=plane, channel=channel, level=level, sense=sense, connectivity=connectivity, min_cells=min_cells,
                          max_boxes=M, keep=keep, out=out, boxes_out=bout, **cells_kw)
    torch.cuda.synchronize()
    assert cb.boxes is bout and cb.cells.maps is out
    assert (cb.cells.got, cb.cells.current, cb.cells.kept, cb.cells.pic_id, cb.cells.kept_pic_id) == (cm.got, cm.current, cm.kept, cm.pic_id, cm.kept_pic_id)
    theirs, mine = cm.maps.cpu().numpy(), out.cpu().numpy()
    boxes = bout.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    names = (planes,) if isinstance(planes, str) else tuple(planes)
    name = plane or next((p for p in names if p != "count"), "count")
    rows_cols = tuple(cm.maps.shape[2:])
    for k in range(R):
        if not cm.got[k]:
            assert (mine[k] == S32).all() and (boxes[k] == S32).all(), k
            continue
        assert np.array_equal(mine[k], theirs[k]), ("maps", k)
        view = getattr(cm, name)[k].cpu().numpy()
        values = view if name == "count" else view[channel]
        inst = regions[k][0] if regions is not None else k
        window = pairs[inst].window(crop)
        box = tuple(regions[k][1:]) if regions is not None else (0, 0) + window[2:]
        want = bm.boxes(values, bm.reached(window, box, cell, rows_cols), window, box, cell, M, bm.BELOW if sense == "below" else bm.ABOVE, level,
                        connectivity, min_cells)
        bad = np.argwhere(boxes[k] != want)
        assert not len(bad), ("boxes", k, bad[:4].tolist(), boxes[k][bad[:4, 0]].tolist(), want[bad[:4, 0]].tolist())
        written = int(boxes[k, 0, 1])
        assert (boxes[k, 1:1 + written, 2:5] >= 1).all()                       # w, h, cells of a written record
    assert built.device_errors() == 0
    return cb, boxes


def _painted(W, H, box, cell, mask):
    """a picture whose luma is 255 where the cells of `mask` ([rows, cols] bool, the grid laid over `box` from its origin) lie"""
    Y = np.zeros((H, W), np.uint8)
    for i, j in np.argwhere(mask):
        x0, y0 = box[0] + j * cell, box[1] + i * cell
        Y[max(y0, 0):max(min(y0 + cell, H), 0), max(x0, 0):max(min(x0 + cell, W), 0)] = 255
    return Y, np.full((H // 2, W // 2), 128, np.uint8), np.full((H // 2, W // 2), 128, np.uint8)


def _pcm_pair(built, pictures):
    return Pair(built, pcm_stream(pictures))


# ---- at the cap: 512 x 512 at cell 4 is 128 x 128 = 16384 cells ----
def _serpentine():
    m = np.zeros((128, 128), bool)
    m[0::2] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    return m


@pytest.fixture(scope="module")
def cap_pair(built):
    i, j = np.indices((128, 128))
    masks = [_serpentine(), (i + j) % 2 == 0, np.ones((128, 128), bool)]
    pair = _pcm_pair(built, [_painted(512, 512, (0, 0), 4, m) for m in masks])
    yield pair
    pair.close()


def test_at_the_cap_serpentine_checkerboard_and_full(built, cap_pair):
    """one picture each, in this order.  The serpentine, one cell wide, visits every other row: ONE component of 8256 cells whose
    length is half the grid — labelling it by propagation until nothing changes would take thousands of rounds.  The checkerboard: 8192
    single cells with 4 neighbours (found above M: the first M in raster order are written), one component with 8.  All cells: 16384."""
    pair = cap_pair
    kw = dict(cell=4, planes=("max",))
    pair.advance(1)
    for conn in (4, 8):
        cb, boxes = _check(built, [pair], None, connectivity=conn, max_boxes=3, **kw)
        assert boxes[0, 0, :4].tolist() == [1, 1, 8256, 0] and boxes[0, 1].tolist() == [0, 0, 512, 512, 8256, 255, 8256 * 255, 0]
    pair.advance(1)
    cb, boxes = _check(built, [pair], None, connectivity=4, max_boxes=64, **kw)
    assert boxes[0, 0, :4].tolist() == [8192, 64, 8192, 0] and boxes[0, 64].tolist() == [8 * 63, 0, 4, 4, 1, 255, 255, 0]
    assert cb.found == [8192] and len(cb.regions()) == 64
    cb, boxes = _check(built, [pair], None, connectivity=4, max_boxes=512, **kw)
    assert boxes[0, 0, :4].tolist() == [8192, 512, 8192, 0] and boxes[0, 512].tolist() == [8 * 63 + 4, 7 * 4, 4, 4, 1, 255, 255, 0]
    cb, boxes = _check(built, [pair], None, connectivity=4, max_boxes=5, min_cells=2, **kw)
    assert boxes[0, 0, :4].tolist() == [0, 0, 8192, 8192] and not boxes[0, 1:].any()
    cb, boxes = _check(built, [pair], None, connectivity=8, max_boxes=2, **kw)
    assert boxes[0, 0, :4].tolist() == [1, 1, 8192, 0] and boxes[0, 1].tolist() == [0, 0, 512, 512, 8192, 255, 8192 * 255, 0]
    pair.advance(1)
    for conn in (4, 8):
        cb, boxes = _check(built, [pair], None, connectivity=conn, max_boxes=1, **kw)
        assert boxes[0].tolist() == [[1, 1, 16384, 0, 0, 0, 0, 0], [0, 0, 512, 512, 16384, 255, 16384 * 255, 0]]


def test_the_sum_of_a_component_passes_two_to_the_thirty_two(built):
    """1024 x 1024 of luma 255 at cell 8, plane "sumsq": one component of 16384 cells x 64 * 255^2 = 6.8e10"""
    pair = _pcm_pair(built, [_painted(1024, 1024, (0, 0), 8, np.ones((128, 128), bool))])
    pair.advance(1)
    cb, boxes = _check(built, [pair], None, cell=8, planes=("count", "sumsq"), max_boxes=2)
    total = 16384 * 64 * 255 * 255
    assert total > 2 ** 32 and boxes[0, 1].tolist() == [0, 0, 1024, 1024, 16384, 64 * 255 * 255, total & 0xFFFFFFFF, total >> 32]
    assert cb.sums()[0].tolist() == [total, 0]
    pair.close()


# ---- an odd grid, 37 x 53 at cell 4, over a box that is not cell-aligned and leaves the 256 x 192 window to the left and above ----
ODD_BOX, ODD_GRID, ODD_SIZE = (-6, -5, 209, 146), (37, 53), (256, 192)


def _odd_masks():
    rows, cols = ODD_GRID
    i, j = np.indices(ODD_GRID)
    up = np.zeros(ODD_GRID, bool)                                  # combs and U shapes open upward: their parts meet in their LAST row
    up[30, 2:40] = True
    up[3:30, 2:40:2] = True
    up[10:20, 44], up[10:20, 50], up[19, 44:51] = True, True, True
    left = np.zeros(ODD_GRID, bool)                                # ... and open to the left: the spine is the last column of each tooth
    left[2:34, 48] = True
    left[2:34:2, 5:48] = True
    rings = np.zeros(ODD_GRID, bool)                               # rectangles that contain other components
    for d in (2, 4, 6, 8, 10, 12):
        rings[d, d:cols - d] = rings[rows - 1 - d, d:cols - d] = True
        rings[d:rows - d, d] = rings[d:rows - d, cols - 1 - d] = True
    rings[18, 20:30] = True
    diagonals = (i - 2 == j) | (i + j == 45)                       # 4 neighbours: single cells; 8: two lines that cross
    return dict(up=up, left=left, rings=rings, diagonals=diagonals, nothing=np.zeros(ODD_GRID, bool))


@pytest.fixture(scope="module")
def odd_pair(built):
    rng = np.random.default_rng(2024)
    masks = list(_odd_masks().values()) + [rng.random(ODD_GRID) < d for d in (0.3, 0.5, 0.6)]
    pair = _pcm_pair(built, [_painted(*ODD_SIZE, ODD_BOX, 4, m) for m in masks])
    yield pair
    pair.close()


def test_shapes_on_an_odd_grid(built, odd_pair):
    """column 0 and row 0 of the grid lie outside the window, column 1 and row 1 are cut by it, the last column is 1 sample wide and the
    last row 2 tall; the pictures follow _odd_masks() and the random maps, in order"""
    pair = odd_pair
    kw = dict(cell=4, grid=ODD_GRID, planes=("max",))
    regions = [(0,) + ODD_BOX]
    found = {}
    for name in _odd_masks():
        pair.advance(1)
        for conn in (4, 8):
            cb, boxes = _check(built, [pair], regions, connectivity=conn, max_boxes=64, **kw)
            found[name, conn] = boxes[0, 0, :4].tolist()
            cb, boxes = _check(built, [pair], regions, connectivity=conn, max_boxes=2, min_cells=3, **kw)
    assert found["up", 4][:2] == found["up", 8][:2] == [2, 2] and found["left", 4][:2] == found["left", 8][:2] == [1, 1]
    assert found["rings", 4][:2] == found["rings", 8][:2] == [7, 7]
    assert found["diagonals", 8][:2] == [1, 1] and found["diagonals", 4][:2] == [67, 64]       # 70 cells, which touch only where the lines cross
    assert found["nothing", 4] == found["nothing", 8] == [0, 0, 0, 0]
    for min_cells, M in ((1, 512), (2, 7), (5, 1)):                # densities 0.3, 0.5, 0.6
        pair.advance(1)
        for conn in (4, 8):
            cb, boxes = _check(built, [pair], regions, connectivity=conn, max_boxes=M, min_cells=min_cells, **kw)
            assert boxes[0, 0, 0] >= 1 and boxes[0, 0, 2] > 300
            if min_cells > 1 and conn == 4:
                assert boxes[0, 0, 3] > 0 and boxes[0, 0, 0] > M       # some were dropped, and more remain than are written
        _check(built, [pair], regions, connectivity=8, max_boxes=1 if M > 1 else 512, min_cells=min_cells, **kw)


def test_below_on_the_cropped_stream_never_takes_unreached_cells(built):
    """window 90 x 60 at (2, 2); the box reaches beyond it on three sides.  Plane "sum", BELOW a level inside the value range: the cells
    the window does not reach hold 0, which would pass, and are background; the rectangles end at the window's edge"""
    pair = Pair(built, _cropped())
    pair.advance(1)
    box = (-11, 5, 130, 70)
    regions = [(0,) + box, (0, 0, 0, 90, 60)]
    for cell in (4, 8):
        cm = built.pull_cells([pair.dec], regions, cell=cell, planes=("count", "sum"))
        count, total = cm.count[0].cpu().numpy(), cm.sum[0, 0].cpu().numpy()
        full = total[count == cell * cell]
        level = int(np.median(full))
        assert full.min() < level < full.max() and (count == 0).any()
        for conn in (4, 8):
            cb, boxes = _check(built, [pair], regions, cell=cell, planes=("count", "sum"), plane="sum", sense="below", level=level, connectivity=conn,
                               max_boxes=64)
            assert 0 < boxes[0, 0, 2] < (count > 0).sum() and boxes[0, 0, 0] >= 1
            for x, y, w, h in boxes[0, 1:1 + boxes[0, 0, 1], :4].tolist():
                assert 0 <= x and x + w <= 90 and 5 <= y and y + h <= 60
        _check(built, [pair], regions, cell=cell, planes=("count", "sum"), plane="count", sense="below", level=cell * cell, max_boxes=8)      # the cut cells
    pair.close()


def _level_for(values, reach, want=3):
    """a level from the model: the highest of a few quantiles of the map at which at least `want` components remain"""
    for q in (0.97, 0.95, 0.9, 0.8, 0.7, 0.5):
        level = int(np.quantile(values, q))
        if bm.boxes(values, reach, (0, 0, 640, 360), (0, 0, 640, 360), 16, 64, level=level, min_cells=2)[0, 0] >= want:
            return level
    raise AssertionError("no level gives three components")


@pytest.mark.parametrize("source,channel", [("y", 0), ("ycbcr", 1)])
def test_real_content_in_change_mode_and_the_boxes_fed_back(built, source, channel):
    """two consecutive pictures of the 640x360 stream, plane "sad": at least three boxes, which pull_change takes as they are — each
    record's count is its rectangle's area, and its sad the sum of its cells' only when the component fills the rectangle"""
    pair = Pair(built, "test_640x360")
    pair.advance(3)
    pair.keep()
    pair.advance(1)
    cm = built.pull_cells([pair.dec], None, cell=16, source=source, planes=("sad",), against="kept")
    values = cm.sad[0, channel].cpu().numpy().astype(np.int64)
    level = _level_for(values, np.ones(values.shape, bool))
    cb, boxes = _check(built, [pair], None, cell=16, source=source, planes=("sad",), against="kept", channel=channel, level=level, min_cells=2, max_boxes=64)
    assert cb.found[0] >= 3 and cb.found[0] == boxes[0, 0, 0]
    regions = cb.regions()
    assert len(regions) == boxes[0, 0, 1] and all(r[0] == 0 for r in regions)
    rc = built.pull_change([pair.dec], regions, source=source)
    assert rc.got == [1] * len(regions)
    assert rc.count.cpu().tolist() == [w * h for _, _, _, w, h in regions]
    padded = cb.regions(pad=8)
    assert padded[0] == (0, regions[0][1] - 8, regions[0][2] - 8, regions[0][3] + 16, regions[0][4] + 16)
    assert built.pull_change([pair.dec], padded, source=source).got == [1] * len(regions)          # boxes may leave the window
    pair.close()


def test_keep_chains_three_pictures(built):
    """keep=True: call t labels the difference to the picture of call t - 1; the first call has nothing to compare with, leaves both
    slices untouched and starts the chain"""
    pair = Pair(built, "test_640x360")
    for t in range(3):
        pic_id = pair.advance(1)
        cb, boxes = _check(built, [pair], None, cell=16, source="ycbcr", planes=("count", "sad", "dmax"), against="kept", threshold=[4, 2, 2],
                           plane="dmax", level=6, min_cells=2, max_boxes=16, keep=True)
        assert cb.cells.current == [1] and cb.cells.pic_id == [pic_id]
        if t == 0:
            assert cb.cells.got == [0] and cb.cells.kept == [0] and cb.found == [0] and cb.regions() == []
        else:
            assert cb.cells.got == [1] and cb.cells.kept_pic_id == [pic_id - 1] and boxes[0, 0, 2] > 0
        pair.kept_now()
    pair.close()


@pytest.mark.parametrize("against", [None, "kept"])
def test_several_regions_of_two_instances_and_instances_without_pictures(built, against):
    """regions of A (640x360) and B (the cropped synthetic stream) in one call; C has decoded but not popped: no current picture; in
    CHANGE mode B has kept nothing.  got = 0: both slices keep their sentinel."""
    a, b, c = Pair(built, "test_640x360"), Pair(built, _cropped()), Pair(built, "plain_ip")
    a.advance(1)
    if against:
        a.keep()
        a.advance(1)
    b.advance(1)
    assert c.step()
    regions = [(0, 0, 0, 640, 360), (1, -3, 5, 61, 41), (2, 0, 0, 32, 32), (0, 300, 100, 200, 150), (1, 0, 0, 90, 60), (0, 13, 11, 37, 23)]
    planes = ("count", "sad") if against else ("count", "sumsq", "max")
    cb, boxes = _check(built, [a, b, c], regions, cell=8, grid=(45, 80), source="ycbcr", planes=planes, against=against,
                       plane="sad" if against else "max", channel=0, level=40 if against else 128, max_boxes=32, min_cells=2)
    assert cb.cells.got == ([1, 0, 0, 1, 0, 1] if against else [1, 1, 0, 1, 1, 1]) and cb.cells.current == [1, 1, 0]
    assert all(r[0] in (0, 1) for r in cb.regions()) and cb.found[2] == 0
    for p in (a, b, c):
        p.close()


def test_whole_windows_on_a_side_stream_and_on_the_default_one(built):
    import torch
    a, b = Pair(built, "test_640x360"), Pair(built, "test_640x360")
    a.advance(1)
    b.advance(4)
    side = torch.cuda.Stream()
    for stream in (side, None):
        cb, boxes = _check(built, [a, b], None, cell=16, planes=("sum",), level=256 * 100, connectivity=4, max_boxes=24, stream=stream)
        assert cb.cells.got == [1, 1] and tuple(cb.boxes.shape) == (2, 25, 8) and tuple(cb.cells.maps.shape) == (2, 1, 23, 40)
        assert boxes[0, 0, 0] >= 1 and boxes[1, 0, 0] >= 1
        assert [r[0] for r in cb.regions()] == [0] * int(boxes[0, 0, 1]) + [1] * int(boxes[1, 0, 1])
    a.close()
    b.close()


def test_the_raw_entry_with_null_arrays_and_the_librarys_own_stream(built):
    import torch
    pair = Pair(built, _cropped())
    pair.advance(1)
    L = built.api_lib()
    grid, M = (8, 12), 5
    maps = torch.full((2, 1) + grid, S32, dtype=torch.int32, device="cuda")
    bout = torch.full((2, 1 + M, 8), S32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    regs = (built.Region * 2)(built.Region(0, 0, 0, 90, 60), built.Region(0, 7, 3, 50, 31))
    cells = built.CellsSpec(maps.data_ptr(), grid[1], grid[0], 8, 0, 1, 0, 16, (ctypes.c_uint32 * 3)(0, 0, 0), 0)
    spec = built.BoxesSpec(bout.data_ptr(), M, 16, 0, 0, 100, 8, 1)
    got = (ctypes.c_uint32 * 2)(7, 7)
    dec = (ctypes.c_void_p * 1)(pair.dec._st)
    assert L.h264bsdmiOutputCellBoxes(1, dec, 2, regs, ctypes.byref(cells), ctypes.byref(spec), None, got, None, None, None, None) == 0
    assert list(got) == [1, 1]
    want = built.pull_cells([pair.dec], [(0, 0, 0, 90, 60), (0, 7, 3, 50, 31)], cell=8, grid=grid, planes=("max",))
    torch.cuda.synchronize()
    assert bool(torch.equal(maps, want.maps))
    host = bout.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for k, box in enumerate([(0, 0, 90, 60), (7, 3, 50, 31)]):
        values = want.max[k, 0].cpu().numpy()
        assert np.array_equal(host[k], bm.boxes(values, bm.reached((2, 2, 90, 60), box, 8, grid), (2, 2, 90, 60), box, 8, M, level=100)), k
    bad = built.BoxesSpec(bout.data_ptr(), M, 2, 0, 0, 100, 8, 1)                      # SUM was not asked for: refused, nothing written
    bout.fill_(S32)
    torch.cuda.synchronize()
    assert L.h264bsdmiOutputCellBoxes(1, dec, 2, regs, ctypes.byref(cells), ctypes.byref(bad), None, got, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert bool((bout == S32).all())
    pair.close()
