"""h264bsd_amd — MI355X-native macroblock-reconstruction back end behind the h264bsd C API.

The product is the C-ABI shared library h264bsd_amd/lib/libh264bsd_mi355x.so (host parser in C,
HIP kernels for gfx950).  This package is a thin ctypes mirror of that ABI, named after the reference's
own entry points so tests read like /root/reference/posix/test_h264bsd.c.
"""
from .capi import (  # noqa: F401
    H264BSD_RDY, H264BSD_PIC_RDY, H264BSD_HDRS_RDY, H264BSD_ERROR, H264BSD_PARAM_SET_ERROR, H264BSD_MEMALLOC_ERROR,
    EXPORTED_SYMBOLS, LIB_PATH, FMT_RGBA, FMT_BGRA, FMT_YCBCRA, FMT_I420, Decoder, DevicePicture, BatchDriver, Replay, build, capture_stream, job_header, job_mvs, convert, device_count, device_errors, device_error_events, lib, api_lib, use_product_library, set_tail, pull_batch,
    TensorSpec, ColourSpec, ResizeSpec, pull_tensor, Region, pull_regions, MotionSpec, pull_motion, Remap, RemapSpec, pull_remap, affine_maps,
    StatsSpec, RegionStats, pull_stats, stats_record_bytes,
    ChangeSpec, RegionChange, keep_pictures, pull_change, change_record_bytes,
    ShiftSpec, RegionShift, pull_shift, shift_record_bytes,
    CornersSpec, CornerPoints, pull_corners, corners_record_bytes,
    CellsSpec, CellMaps, pull_cells,
    BoxesSpec, CellBoxes, pull_boxes,
    CellShiftSpec, CellShift, pull_flow,
    MatchesSpec, PointMatches, pull_matches, matches_record_bytes, descriptor_pattern,
    ModelSpec, PointModel, pull_model, model_record_bytes,
    BlendSpec, BLEND_FROZEN, blend_pictures, pull_kept, SpreadSpec, SPREAD_UPDATES,
    WarpSpec, WarpMap, WARP_OUTSIDE, WARP_MAX_COEFFICIENT, warp_coefficients, warp_kept,
)

# 0.2: pull_remap / affine_maps (h264bsdmiOutputTensorRemap); 0.3: pull_stats (h264bsdmiOutputRegionStats);
# 0.4: keep_pictures / pull_change (h264bsdmiKeepCurrentPictures, h264bsdmiOutputRegionChange); 0.5: pull_cells (h264bsdmiOutputCellMaps)
# 0.6: pull_boxes (h264bsdmiOutputCellBoxes); 0.7: pull_shift (h264bsdmiOutputRegionShift)
# 0.8: blend_pictures / pull_kept (h264bsdmiBlendCurrentPictures, h264bsdmiOutputKeptPictures)
# 0.9: pull_corners (h264bsdmiOutputCornerPoints); 0.10: pull_flow (h264bsdmiOutputCellShift)
# 0.11: pull_matches (h264bsdmiOutputPointMatches); 0.12: pull_model (h264bsdmiOutputPointModel)
# 0.13: warp_kept / warp_coefficients (h264bsdmiWarpKeptPictures)
# 0.14: blend_pictures(spread=), pull_kept(spread=), pull_cells / pull_boxes(against="spread") (h264bsdmiBlendCurrentPicturesSpread,
#       h264bsdmiOutputKeptSpread, H264BSDMI_CELLS_SPREAD)
__version__ = "0.14.0"
