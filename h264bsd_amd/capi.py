"""ctypes mirror of include/h264bsd_decoder.h + include/h264bsd_mi355x.h.

No pixel is ever produced in Python or on the CPU here: every call goes through the C ABI of
libh264bsd_mi355x.so, and anything that needs pixels fails loudly when the HIP engine is unavailable.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "lib", "libh264bsd_mi355x.so")                  # the product: what a C application links
BENCH_LIB_PATH = os.path.join(HERE, "lib", "libh264bsd_mi355x_bench.so")      # same objects + the harness exports; what
                                                                              # this mirror loads (Replay, job tools)
if os.environ.get("H264BSD_VARIANT"):      # A/B experiments: a library built with other kernel flags (tools/experiments/build_variant.sh)
    BENCH_LIB_PATH = os.path.join(HERE, "lib_" + os.environ["H264BSD_VARIANT"], "libh264bsd_mi355x_bench.so")

(H264BSD_RDY, H264BSD_PIC_RDY, H264BSD_HDRS_RDY, H264BSD_ERROR, H264BSD_PARAM_SET_ERROR,
 H264BSD_MEMALLOC_ERROR) = range(6)

# every symbol include/*.h declares (checked by tests/test_abi.py); PRODUCT_SYMBOLS: those of the product library
EXPORTED_SYMBOLS = [
    "h264bsdInit", "h264bsdDecode", "h264bsdShutdown", "h264bsdNextOutputPicture",
    "h264bsdNextOutputPictureRGBA", "h264bsdNextOutputPictureBGRA", "h264bsdNextOutputPictureYCbCrA",
    "h264bsdPicWidth", "h264bsdPicHeight", "h264bsdVideoRange", "h264bsdMatrixCoefficients",
    "h264bsdCroppingParams", "h264bsdSampleAspectRatio", "h264bsdCheckValidParamSets", "h264bsdFlushBuffer",
    "h264bsdProfile", "h264bsdAlloc", "h264bsdFree", "h264bsdConvertToRGBA", "h264bsdConvertToBGRA",
    "h264bsdConvertToYCbCrA",
    "h264bsdmiInitCapture", "h264bsdmiNextOutputInfo", "h264bsdmiNextOutputPictureDevice", "h264bsdmiNextOutputTensorBatch", "h264bsdmiNextOutputTensorBatchColour", "h264bsdmiNextOutputTensorBatchResize", "h264bsdmiOutputTensorRegions", "h264bsdmiOutputTensorRemap", "h264bsdmiSetMotionExport", "h264bsdmiOutputMotionRegions", "h264bsdmiOutputRegionStats", "h264bsdmiKeepCurrentPictures", "h264bsdmiBlendCurrentPictures", "h264bsdmiBlendCurrentPicturesSpread", "h264bsdmiOutputKeptPictures", "h264bsdmiOutputKeptSpread", "h264bsdmiWarpKeptPictures", "h264bsdmiOutputRegionChange", "h264bsdmiOutputRegionShift", "h264bsdmiOutputCornerPoints", "h264bsdmiOutputCellMaps", "h264bsdmiOutputCellBoxes", "h264bsdmiOutputCellShift", "h264bsdmiOutputPointMatches", "h264bsdmiDescriptorPattern", "h264bsdmiOutputPointModel", "h264bsdmiJobFinalize", "h264bsdmiDeviceCount", "h264bsdmiSetDevice", "h264bsdmiFlush", "h264bsdmiFlushAsync", "h264bsdmiDeviceErrors",
    "h264bsdmiDecodePicture", "h264bsdmiDecodePictureBatch", "h264bsdmiNextOutputPictureBatch", "h264bsdmiPullAndDecodePictureBatch", "h264bsdmiSetParserThreads", "h264bsdmiSetInputReadOnly", "h264bsdmiSetCopyElision",
    "h264bsdmiReplayCreate", "h264bsdmiReplayCreateStaggered", "h264bsdmiReplayCreateDesync", "h264bsdmiReplayCreateSched", "h264bsdmiReplayReschedule", "h264bsdmiReplayDestroy", "h264bsdmiReplayRun", "h264bsdmiReplaySync",
    "h264bsdmiReplayFetch", "h264bsdmiReplayDbkRecords", "h264bsdmiReplayChecksums", "h264bsdmiReplayConvert", "h264bsdmiReplayFetchConverted",
    "h264bsdmiReplayTimings", "h264bsdmiReplaySetConvert", "h264bsdmiReplayConvertTimings", "h264bsdmiReplaySetStages", "h264bsdmiReplaySetTimedKernels", "h264bsdmiReplaySetGroups", "h264bsdmiDebugTailProfile", "h264bsdmiDebugSetTail", "h264bsdmiDebugDeviceErrorEvents", "h264bsdmiReplayJobBytes", "h264bsdmiReplayFrameBytes",
]

class DevicePicture(ctypes.Structure):
    """h264bsdmi_device_picture (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pitch", ctypes.c_uint32),
                ("format", ctypes.c_uint32), ("picId", ctypes.c_uint32), ("isIdrPic", ctypes.c_uint32),
                ("numErrMbs", ctypes.c_uint32), ("stream", ctypes.c_void_p)]


FMT_RGBA, FMT_BGRA, FMT_YCBCRA, FMT_I420 = 0, 1, 2, 3


class TensorSpec(ctypes.Structure):
    """h264bsdmi_tensor_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("layout", ctypes.c_uint32),
                ("dtype", ctypes.c_uint32), ("channels", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("resize", ctypes.c_uint32),
                ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


class ColourSpec(ctypes.Structure):
    """h264bsdmi_colour_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("matrix", ctypes.c_uint32), ("range", ctypes.c_uint32), ("chroma", ctypes.c_uint32), ("unspecified", ctypes.c_uint32)]


class ResizeSpec(ctypes.Structure):
    """h264bsdmi_resize_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("filter", ctypes.c_uint32), ("fit", ctypes.c_uint32), ("pad", ctypes.c_float * 3)]


class Region(ctypes.Structure):
    """h264bsdmi_region (include/h264bsd_mi355x.h)"""
    _fields_ = [("instance", ctypes.c_uint32), ("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32)]


class Remap(ctypes.Structure):
    """h264bsdmi_remap (include/h264bsd_mi355x.h)"""
    _fields_ = [("instance", ctypes.c_uint32), ("map", ctypes.c_void_p)]


class RemapSpec(ctypes.Structure):
    """h264bsdmi_remap_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("filter", ctypes.c_uint32), ("border", ctypes.c_uint32), ("pad", ctypes.c_float * 3)]


class MotionSpec(ctypes.Structure):
    """h264bsdmi_motion_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("layout", ctypes.c_uint32),
                ("dtype", ctypes.c_uint32), ("planes", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("fit", ctypes.c_uint32),
                ("sampler", ctypes.c_uint32), ("units", ctypes.c_uint32), ("per_picture", ctypes.c_uint32)]


class StatsSpec(ctypes.Structure):
    """h264bsdmi_stats_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("source", ctypes.c_uint32), ("bins", ctypes.c_uint32), ("crop", ctypes.c_uint32)]


class ChangeSpec(ctypes.Structure):
    """h264bsdmi_change_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("source", ctypes.c_uint32), ("bins", ctypes.c_uint32), ("crop", ctypes.c_uint32),
                ("threshold", ctypes.c_uint32 * 3), ("keep_after", ctypes.c_uint32)]


class BlendSpec(ctypes.Structure):
    """h264bsdmi_blend_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("shift", ctypes.c_uint32), ("hold", ctypes.c_uint32), ("moving_shift", ctypes.c_uint32), ("moving", ctypes.c_void_p)]


BLEND_FROZEN = 8                                                                 # H264BSDMI_BLEND_FROZEN


class SpreadSpec(ctypes.Structure):
    """h264bsdmi_spread_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("gain", ctypes.c_uint32), ("lowest", ctypes.c_uint32), ("highest", ctypes.c_uint32), ("update", ctypes.c_uint32)]


SPREAD_UPDATES = {"none": 0, "all": 1, "still": 2}                               # H264BSDMI_SPREAD_*


class WarpMap(ctypes.Structure):
    """h264bsdmi_warp_map (include/h264bsd_mi355x.h): output -> source, 16.16 fixed point"""
    _fields_ = [(k, ctypes.c_int32) for k in "abcdef"]


class WarpSpec(ctypes.Structure):
    """h264bsdmi_warp_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("maps", ctypes.POINTER(WarpMap)), ("outside", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("count", ctypes.c_void_p)]


WARP_OUTSIDE = {"replicate": 0, "current": 1}                                    # H264BSDMI_WARP_*
WARP_MAX_COEFFICIENT = 16 * 65536                                                # H264BSDMI_WARP_MAX_COEFFICIENT


class ShiftSpec(ctypes.Structure):
    """h264bsdmi_shift_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("radius", ctypes.c_uint32), ("surface", ctypes.c_uint32), ("crop", ctypes.c_uint32),
                ("keep_after", ctypes.c_uint32)]


class CornersSpec(ctypes.Structure):
    """h264bsdmi_corners_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("score", ctypes.c_uint32), ("block", ctypes.c_uint32), ("nms", ctypes.c_uint32),
                ("max_points", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("zero", ctypes.c_uint32), ("min_score", ctypes.c_uint64)]


class CellsSpec(ctypes.Structure):
    """h264bsdmi_cells_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("cols", ctypes.c_uint32), ("rows", ctypes.c_uint32), ("cell", ctypes.c_uint32),
                ("source", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("planes", ctypes.c_uint32),
                ("threshold", ctypes.c_uint32 * 3), ("keep_after", ctypes.c_uint32)]


class CellShiftSpec(ctypes.Structure):
    """h264bsdmi_cell_shift_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("cols", ctypes.c_uint32), ("rows", ctypes.c_uint32), ("cell", ctypes.c_uint32),
                ("radius", ctypes.c_uint32), ("planes", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("keep_after", ctypes.c_uint32)]


class MatchesSpec(ctypes.Structure):
    """h264bsdmi_matches_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("kept_points", ctypes.c_void_p), ("current_points", ctypes.c_void_p),
                ("max_points", ctypes.c_uint32), ("max_distance", ctypes.c_uint32), ("ratio", ctypes.c_uint32), ("max_move", ctypes.c_uint32),
                ("mutual_only", ctypes.c_uint32), ("crop", ctypes.c_uint32), ("keep_after", ctypes.c_uint32), ("zero", ctypes.c_uint32)]


class ModelSpec(ctypes.Structure):
    """h264bsdmi_model_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("matches", ctypes.c_void_p), ("kept_points", ctypes.c_void_p), ("current_points", ctypes.c_void_p),
                ("max_points", ctypes.c_uint32), ("model", ctypes.c_uint32), ("tolerance", ctypes.c_uint32), ("max_scale", ctypes.c_uint32),
                ("min_inliers", ctypes.c_uint32), ("zero", ctypes.c_uint32 * 3)]


class BoxesSpec(ctypes.Structure):
    """h264bsdmi_boxes_spec (include/h264bsd_mi355x.h)"""
    _fields_ = [("data", ctypes.c_void_p), ("max_boxes", ctypes.c_uint32), ("plane", ctypes.c_uint32), ("channel", ctypes.c_uint32),
                ("sense", ctypes.c_uint32), ("level", ctypes.c_uint32), ("connectivity", ctypes.c_uint32), ("min_cells", ctypes.c_uint32)]


SHIFT_MAX_RADIUS, SHIFT_MAX_SIDE = 16, 4096                                       # H264BSDMI_SHIFT_MAX_*
CORNER_SCORES = {"min_eigen": 0, "harris": 1}                                    # H264BSDMI_CORNERS_*
CORNERS_MAX_NMS, CORNERS_MAX_POINTS = 7, 256                                     # H264BSDMI_CORNERS_MAX_*
BOXES_MAX_CELLS, BOXES_MAX_BOXES = 16384, 512                                     # H264BSDMI_BOXES_MAX_*
BOXES_SENSES = {"above": 0, "below": 1}                                          # H264BSDMI_BOXES_*
# per mode (H264BSDMI_CELLS_PICTURE, _CHANGE): name -> H264BSDMI_CELL_*, in the order of the maps
CELL_PLANES = ({"count": 1, "sum": 2, "sumsq": 4, "min": 8, "max": 16}, {"count": 1, "sad": 2, "ssd": 4, "dsum": 8, "dmax": 16, "above": 32})
CELL_SPREAD_PLANES = {"count": 1, "fore": 2, "excess": 4, "spread": 8}              # ... and of H264BSDMI_CELLS_SPREAD
CELL_MODE_PLANES = CELL_PLANES + (CELL_SPREAD_PLANES,)                            # by H264BSDMI_CELLS_*
CELL_AGAINST = {None: 0, "kept": 1, "spread": 2}                                  # pull_cells(against=) -> H264BSDMI_CELLS_*
CELL_SIZES = (4, 8, 16, 32, 64)
FLOW_PLANES = {"count": 1, "dx": 2, "dy": 4, "best": 8, "still": 16, "ties": 32}    # name -> H264BSDMI_FLOW_*, in the order of the maps
FLOW_CELL_SIZES = (8, 16, 32, 64)
MATCH_FLAGS = {"valid": 1, "mutual": 2, "accepted": 4}                           # H264BSDMI_MATCH_*
MATCHES_MAX_POINTS = 256
MODEL_KINDS = {"translation": 0, "similarity": 1}                                 # name -> H264BSDMI_MODEL_*
MODEL_FLAGS = {"usable": 1, "inlier": 2}                                         # H264BSDMI_MODEL_USABLE / _INLIER
STATS_SOURCES = {"y": (0, 1), "ycbcr": (1, 3), "rgb": (2, 3)}                    # name -> (H264BSDMI_STATS_*, channels)
STATS_BINS = (0, 16, 32, 64, 128, 256)
MOTION_PLANES = {"mv": (1, 2), "valid": (2, 1), "age": (4, 1), "qp": (8, 1)}     # name -> (H264BSDMI_MOTION_PLANE_*, channels), in channel order
MOTION_SAMPLERS = {"nearest": 0, "area": 1}                                      # H264BSDMI_MOTION_*
MOTION_UNITS = {"source": 0, "output": 1}                                        # H264BSDMI_MOTION_UNITS_*
MATRICES = {"reference": 0, "auto": 1, "bt601": 2, "bt709": 3, "bt2020": 4, "fcc": 5, "smpte240": 6}    # H264BSDMI_MATRIX_*
RANGES = {"auto": 0, "limited": 1, "full": 2}                                                          # H264BSDMI_RANGE_*
CHROMA = {"nearest": 0, "bilinear": 1}                                                                 # H264BSDMI_CHROMA_*
FILTERS = {("bilinear", False): 0, ("bilinear", True): 1, ("bicubic", True): 2}                           # H264BSDMI_FILTER_*
FITS = {"stretch": 0, "letterbox": 1}                                                                   # H264BSDMI_FIT_*
REMAP_FILTERS = {"nearest": 0, "bilinear": 1}                                                          # H264BSDMI_REMAP_*
BORDERS = {"constant": 0, "replicate": 1}                                                              # H264BSDMI_BORDER_*
LAYOUTS = {"NCHW": 0, "NHWC": 1}
CHANNELS = {"RGB": (0, 3), "BGR": (1, 3), "RGBA": (2, 4), "BGRA": (3, 4), "Y": (4, 1)}     # name -> (H264BSDMI_CH_*, channels)

JOB_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint32)
P32 = ctypes.POINTER(ctypes.c_uint32)


def build(force=False):
    """Compile the library in-tree for gfx950 (hipcc cross-compiles; no GPU needed)."""
    if force:
        subprocess.run(["make", "-s", "-C", CSRC, "clean"], check=True)
    subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return LIB_PATH


_lib = None


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's).  A process that loads this
    library first and imports torch later would end up with torch bound to a runtime it was not built for
    ("No HIP GPUs are available").  When torch is installed, load its runtime first so that both share it — the
    configuration `import torch` before `h264bsd_amd.lib()` gives anyway.  Plain C consumers are unaffected."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
        if os.path.exists(path):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                return


_api = None
_use_product = False


def use_product_library(on=True):
    """Decoder / BatchDriver / pull_batch / convert / device_* go through libh264bsd_mi355x.so — what a C application links — instead
    of the harness library (same objects plus the replay exports).  tests/test_gpu_api.py switches it on for its module."""
    global _use_product
    _use_product = bool(on)


def api_lib():
    """the library the drop-in API is called through: the product library when use_product_library() is on, else the harness one"""
    global _api
    if not _use_product:
        return lib()
    if _api is None:
        if not os.path.exists(LIB_PATH):
            build()
        _share_torch_hip_runtime()
        _api = _declare(ctypes.CDLL(LIB_PATH), harness=False)
    return _api


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) or not os.path.exists(BENCH_LIB_PATH):
        build()
    _share_torch_hip_runtime()
    _lib = _declare(ctypes.CDLL(BENCH_LIB_PATH), harness=True)
    return _lib


def _declare(L, harness):
    vp, u32, u8p = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p
    L.h264bsdAlloc.restype = vp
    L.h264bsdFree.argtypes = [vp]
    L.h264bsdInit.argtypes = [vp, u32]
    L.h264bsdInit.restype = u32
    L.h264bsdmiInitCapture.argtypes = [vp, u32, JOB_CB, vp]
    L.h264bsdmiInitCapture.restype = u32
    L.h264bsdDecode.argtypes = [vp, u8p, u32, u32, P32]
    L.h264bsdDecode.restype = u32
    L.h264bsdShutdown.argtypes = [vp]
    for n in ("h264bsdNextOutputPicture", "h264bsdNextOutputPictureRGBA", "h264bsdNextOutputPictureBGRA",
              "h264bsdNextOutputPictureYCbCrA"):
        getattr(L, n).argtypes = [vp, P32, P32, P32]
        getattr(L, n).restype = vp
    for n in ("h264bsdPicWidth", "h264bsdPicHeight", "h264bsdVideoRange", "h264bsdMatrixCoefficients",
              "h264bsdCheckValidParamSets", "h264bsdProfile"):
        getattr(L, n).argtypes = [vp]
        getattr(L, n).restype = u32
    L.h264bsdFlushBuffer.argtypes = [vp]
    L.h264bsdCroppingParams.argtypes = [vp, P32, P32, P32, P32, P32]
    L.h264bsdSampleAspectRatio.argtypes = [vp, P32, P32]
    for n in ("h264bsdConvertToRGBA", "h264bsdConvertToBGRA", "h264bsdConvertToYCbCrA"):
        getattr(L, n).argtypes = [u32, u32, vp, vp]
        getattr(L, n).restype = None
    L.h264bsdmiNextOutputInfo.argtypes = [vp, P32, P32, P32]
    L.h264bsdmiNextOutputInfo.restype = ctypes.c_int
    L.h264bsdmiNextOutputPictureDevice.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DevicePicture)]
    L.h264bsdmiNextOutputPictureDevice.restype = ctypes.c_int
    L.h264bsdmiNextOutputTensorBatch.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(TensorSpec), vp, P32, P32, P32, P32]
    L.h264bsdmiNextOutputTensorBatch.restype = ctypes.c_int
    L.h264bsdmiNextOutputTensorBatchColour.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(TensorSpec), ctypes.POINTER(ColourSpec), vp,
                                                       P32, P32, P32, P32]
    L.h264bsdmiNextOutputTensorBatchColour.restype = ctypes.c_int
    L.h264bsdmiNextOutputTensorBatchResize.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(TensorSpec), ctypes.POINTER(ColourSpec),
                                                       ctypes.POINTER(ResizeSpec), vp, P32, P32, P32, P32, P32]
    L.h264bsdmiNextOutputTensorBatchResize.restype = ctypes.c_int
    L.h264bsdmiOutputTensorRegions.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(TensorSpec),
                                               ctypes.POINTER(ColourSpec), ctypes.POINTER(ResizeSpec), vp, P32, P32, P32, P32]
    L.h264bsdmiOutputTensorRegions.restype = ctypes.c_int
    L.h264bsdmiOutputTensorRemap.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Remap), ctypes.POINTER(TensorSpec),
                                             ctypes.POINTER(ColourSpec), ctypes.POINTER(RemapSpec), vp, P32, P32, P32]
    L.h264bsdmiOutputTensorRemap.restype = ctypes.c_int
    L.h264bsdmiSetMotionExport.argtypes = [vp, u32]
    L.h264bsdmiSetMotionExport.restype = ctypes.c_int
    L.h264bsdmiOutputMotionRegions.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(MotionSpec), vp,
                                               P32, P32, P32, P32]
    L.h264bsdmiOutputMotionRegions.restype = ctypes.c_int
    L.h264bsdmiOutputRegionStats.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(StatsSpec), vp, P32, P32, P32]
    L.h264bsdmiOutputRegionStats.restype = ctypes.c_int
    L.h264bsdmiKeepCurrentPictures.argtypes = [u32, ctypes.POINTER(vp), vp, P32, P32]
    L.h264bsdmiKeepCurrentPictures.restype = ctypes.c_int
    L.h264bsdmiBlendCurrentPictures.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(BlendSpec), vp, P32, P32, P32]
    L.h264bsdmiBlendCurrentPictures.restype = ctypes.c_int
    L.h264bsdmiOutputKeptPictures.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), vp, P32, P32]
    L.h264bsdmiOutputKeptPictures.restype = ctypes.c_int
    L.h264bsdmiBlendCurrentPicturesSpread.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(BlendSpec), ctypes.POINTER(SpreadSpec), vp, P32, P32, P32]
    L.h264bsdmiBlendCurrentPicturesSpread.restype = ctypes.c_int
    L.h264bsdmiOutputKeptSpread.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, P32, P32]
    L.h264bsdmiOutputKeptSpread.restype = ctypes.c_int
    L.h264bsdmiOutputRegionChange.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(ChangeSpec), vp,
                                              P32, P32, P32, P32, P32]
    L.h264bsdmiOutputRegionChange.restype = ctypes.c_int
    L.h264bsdmiOutputRegionShift.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(ShiftSpec), vp,
                                             P32, P32, P32, P32, P32]
    L.h264bsdmiOutputRegionShift.restype = ctypes.c_int
    L.h264bsdmiOutputCornerPoints.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(CornersSpec), vp, P32, P32, P32]
    L.h264bsdmiOutputCornerPoints.restype = ctypes.c_int
    L.h264bsdmiOutputCellMaps.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(CellsSpec), vp,
                                          P32, P32, P32, P32, P32]
    L.h264bsdmiOutputCellMaps.restype = ctypes.c_int
    L.h264bsdmiOutputCellBoxes.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(CellsSpec), ctypes.POINTER(BoxesSpec), vp,
                                           P32, P32, P32, P32, P32]
    L.h264bsdmiOutputCellBoxes.restype = ctypes.c_int
    L.h264bsdmiOutputCellShift.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(CellShiftSpec), vp,
                                           P32, P32, P32, P32, P32]
    L.h264bsdmiOutputCellShift.restype = ctypes.c_int
    L.h264bsdmiOutputPointMatches.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(Region), ctypes.POINTER(MatchesSpec), vp,
                                              P32, P32, P32, P32, P32]
    L.h264bsdmiOutputPointMatches.restype = ctypes.c_int
    L.h264bsdmiWarpKeptPictures.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(WarpSpec), vp, P32, P32]
    L.h264bsdmiWarpKeptPictures.restype = ctypes.c_int
    L.h264bsdmiOutputPointModel.argtypes = [u32, ctypes.POINTER(vp), u32, ctypes.POINTER(ModelSpec), vp]
    L.h264bsdmiOutputPointModel.restype = ctypes.c_int
    L.h264bsdmiDescriptorPattern.argtypes = []
    L.h264bsdmiDescriptorPattern.restype = ctypes.POINTER(ctypes.c_int8)
    L.h264bsdmiDecodePicture.argtypes = [vp, u8p, u32, u32, P32, P32]
    L.h264bsdmiDecodePicture.restype = u32
    L.h264bsdmiDecodePictureBatch.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(vp), P32, P32, P32, P32, P32]
    L.h264bsdmiPullAndDecodePictureBatch.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(vp), P32, P32, P32, ctypes.POINTER(vp), P32, P32, P32, P32, P32]
    L.h264bsdmiSetParserThreads.argtypes = [ctypes.c_int]
    L.h264bsdmiSetInputReadOnly.argtypes = [vp, u32]
    L.h264bsdmiSetCopyElision.argtypes = [vp, u32]
    L.h264bsdmiSetCopyElision.restype = ctypes.c_int
    L.h264bsdmiSetDevice.argtypes = [ctypes.c_int]
    L.h264bsdmiDeviceErrors.restype = ctypes.c_uint
    L.h264bsdmiNextOutputPictureBatch.argtypes = [u32, ctypes.POINTER(vp), ctypes.POINTER(vp), P32, P32, P32]
    if not harness:
        return L
    L.h264bsdmiJobFinalize.argtypes = [ctypes.c_void_p, u32, u32]
    L.h264bsdmiReplayCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p), P32, u32, u32]
    L.h264bsdmiReplayCreate.restype = vp
    L.h264bsdmiReplayCreateStaggered.argtypes = [ctypes.POINTER(ctypes.c_void_p), P32, u32, u32, u32]
    L.h264bsdmiReplayCreateStaggered.restype = vp
    L.h264bsdmiReplayCreateDesync.argtypes = [ctypes.POINTER(ctypes.c_void_p), P32, u32, u32, P32, u32, u32]
    L.h264bsdmiReplayCreateDesync.restype = vp
    L.h264bsdmiReplayCreateSched.argtypes = [ctypes.POINTER(ctypes.c_void_p), P32, u32, u32, P32, u32, u32, u32]
    L.h264bsdmiReplayCreateSched.restype = vp
    L.h264bsdmiReplayReschedule.argtypes = [vp, P32, u32, u32, u32]
    L.h264bsdmiReplayDestroy.argtypes = [vp]
    L.h264bsdmiReplayDestroy.restype = None
    L.h264bsdmiReplayRun.argtypes = [vp, u32, u32]
    L.h264bsdmiReplaySync.argtypes = [vp]
    L.h264bsdmiReplayFetch.argtypes = [vp, u32, u32, vp]
    L.h264bsdmiReplayDbkRecords.argtypes = [vp, u32, u32, vp, u32]
    L.h264bsdmiReplayChecksums.argtypes = [vp, u32, vp]
    L.h264bsdmiReplayConvert.argtypes = [vp, u32, ctypes.c_int]
    L.h264bsdmiReplayFetchConverted.argtypes = [vp, u32, vp]
    L.h264bsdmiReplayTimings.argtypes = [vp, ctypes.POINTER(ctypes.c_float), P32]
    L.h264bsdmiReplaySetConvert.argtypes = [vp, ctypes.c_int]
    L.h264bsdmiReplayConvertTimings.argtypes = [vp, ctypes.POINTER(ctypes.c_float), P32]
    L.h264bsdmiReplaySetStages.argtypes = [vp, ctypes.c_uint]
    L.h264bsdmiReplaySetTimedKernels.argtypes = [vp, ctypes.c_uint]
    L.h264bsdmiReplaySetGroups.argtypes = [vp, u32]
    L.h264bsdmiDebugSetTail.argtypes = [u32] * 7
    L.h264bsdmiReplayJobBytes.argtypes = [vp]
    L.h264bsdmiReplayJobBytes.restype = ctypes.c_ulonglong
    L.h264bsdmiReplayFrameBytes.argtypes = [vp]
    L.h264bsdmiReplayFrameBytes.restype = u32
    return L


def device_count():
    return int(api_lib().h264bsdmiDeviceCount())


KEEP = 0xFFFFFFFF


def set_tail(dbk_rows_light=KEEP, dbk_rows_heavy=KEEP, dbk_waves=KEEP, intra_rows_light=KEEP, intra_rows_heavy=KEEP, intra_waves=KEEP,
             band_budget=KEEP):
    """How the per-picture kernels split the pictures of replay sets / decoders created from now on into row bands
    (h264bsdmiDebugSetTail): rows per band for light / heavy pictures (0 = one band) and wavefronts per workgroup."""
    lib().h264bsdmiDebugSetTail(dbk_rows_light, dbk_rows_heavy, dbk_waves, intra_rows_light, intra_rows_heavy, intra_waves, band_budget)


def device_errors():
    """sticky DEVERR_* bits of the engine (0 = none): tripwires of the kernels that must never fire"""
    return int(api_lib().h264bsdmiDeviceErrors())


def device_error_events():
    """how often a tripwire of the kernels has fired since the library was loaded (monotonic; bench library)"""
    L = lib()
    L.h264bsdmiDebugDeviceErrorEvents.restype = ctypes.c_uint
    return int(L.h264bsdmiDebugDeviceErrorEvents())


class Decoder:
    """One decoder instance.  Method names follow the reference API (h264bsd_decoder.h)."""

    def __init__(self, no_output_reordering=0, capture=None, copy_elision=None, motion=False):
        """capture: None -> pixels on the GPU (h264bsdInit; raises when there is no device);
        a callable(bytes) -> parser only, every picture's frame job is handed to it.
        copy_elision: None -> the library's default (on with a device, off in capture mode), else h264bsdmiSetCopyElision.
        motion: keep the motion side information of every picture on the device for pull_motion (h264bsdmiSetMotionExport)."""
        L = api_lib()
        self._L = L
        self._st = L.h264bsdAlloc()
        self._cb = None
        if capture is None:
            rc = L.h264bsdInit(self._st, no_output_reordering)
        elif capture == "discard":           # parser only, frame jobs dropped (parser benchmarks)
            rc = L.h264bsdmiInitCapture(self._st, no_output_reordering, ctypes.cast(None, JOB_CB), None)
        else:
            self._cb = JOB_CB(lambda user, p, n: capture(ctypes.string_at(p, n)))
            rc = L.h264bsdmiInitCapture(self._st, no_output_reordering, self._cb, None)
        if rc != 0:
            L.h264bsdFree(self._st)
            self._st = None
            raise RuntimeError("h264bsdInit failed: the HIP engine is not available (no CPU pixel path exists)")
        if copy_elision is not None:
            L.h264bsdmiSetCopyElision(self._st, 1 if copy_elision else 0)
        if motion and L.h264bsdmiSetMotionExport(self._st, 1) != 0:
            self.close()
            raise RuntimeError("h264bsdmiSetMotionExport failed: motion export needs a decoder bound to a device")

    def close(self):
        if self._st:
            self._L.h264bsdShutdown(self._st)
            self._L.h264bsdFree(self._st)
            self._st = None

    __del__ = close

    def decode(self, buf_addr, length, pic_id=0):
        """h264bsdDecode on raw memory: returns (status, readBytes)."""
        rb = ctypes.c_uint32(0)
        r = self._L.h264bsdDecode(self._st, buf_addr, length, pic_id, ctypes.byref(rb))
        return int(r), int(rb.value)

    def _next(self, fn, nbytes, dtype):
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        p = fn(self._st, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        if not p:
            return None
        arr = np.frombuffer(ctypes.string_at(p, nbytes), dtype=dtype)
        return arr, int(a.value), int(b.value), int(c.value)

    def next_output_info(self):
        """(slot, picId, isIdr, numErrMbs) of the next output picture, or None (works in capture mode)"""
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        slot = self._L.h264bsdmiNextOutputInfo(self._st, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return None if slot < 0 else (slot, int(a.value), int(b.value), int(c.value))

    def next_output_picture_device(self, fmt=FMT_I420, crop=False):
        """Pop the next output picture and leave it in HBM.  Returns (tensor, picId, isIdr, numErrMbs) or None;
        tensor is a zero-copy torch.uint8 CUDA tensor: [h*3/2, w] for I420 (Y rows, then Cb and Cr rows of w/2 bytes
        packed back to back), [h, w, 4] for the converted formats.  It aliases decoder memory: valid until the next
        decode()/close() of this instance — clone() to keep it."""
        import torch
        pic = DevicePicture()
        rc = self._L.h264bsdmiNextOutputPictureDevice(self._st, fmt, 1 if crop else 0, ctypes.byref(pic))
        if rc == 0:
            return None
        if rc < 0:
            raise RuntimeError(f"h264bsdmiNextOutputPictureDevice failed ({rc})")
        n = pic.width * pic.height * 3 // 2 if fmt == FMT_I420 else pic.width * pic.height * 4

        class _Buf:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (pic.data, False), "version": 2}
        t = torch.as_tensor(_Buf(), device="cuda")
        t = t.view(pic.height * 3 // 2, pic.width) if fmt == FMT_I420 else t.view(pic.height, pic.width, 4)
        return t, int(pic.picId), int(pic.isIdrPic), int(pic.numErrMbs)

    def frame_bytes(self):
        return self.pic_width() * self.pic_height() * 384

    def next_output_picture(self):
        """(uint8 I420 frame copy, picId, isIdr, numErrMbs) or None"""
        return self._next(self._L.h264bsdNextOutputPicture, self.frame_bytes(), np.uint8)

    def next_output_picture_converted(self, fmt):
        fn = (self._L.h264bsdNextOutputPictureRGBA, self._L.h264bsdNextOutputPictureBGRA,
              self._L.h264bsdNextOutputPictureYCbCrA)[fmt]
        return self._next(fn, self.pic_width() * self.pic_height() * 256 * 4, np.uint32)

    def pic_width(self):
        return int(self._L.h264bsdPicWidth(self._st))

    def pic_height(self):
        return int(self._L.h264bsdPicHeight(self._st))

    def video_range(self):
        return int(self._L.h264bsdVideoRange(self._st))

    def matrix_coefficients(self):
        return int(self._L.h264bsdMatrixCoefficients(self._st))

    def profile(self):
        return int(self._L.h264bsdProfile(self._st))

    def check_valid_param_sets(self):
        return int(self._L.h264bsdCheckValidParamSets(self._st))

    def flush_buffer(self):
        self._L.h264bsdFlushBuffer(self._st)

    def cropping_params(self):
        v = [ctypes.c_uint32() for _ in range(5)]
        self._L.h264bsdCroppingParams(self._st, *[ctypes.byref(x) for x in v])
        return tuple(int(x.value) for x in v)   # flag, left, width, top, height

    def sample_aspect_ratio(self):
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        self._L.h264bsdSampleAspectRatio(self._st, ctypes.byref(w), ctypes.byref(h))
        return int(w.value), int(h.value)

    def decode_stream(self, data, on_picture=None, drain=True):
        """The reference harness loop (posix/test_h264bsd.c:146-177) over a whole byte stream.
        Returns the call trace [(status, readBytes)]."""
        buf = ctypes.create_string_buffer(data, len(data))
        base, off, trace = ctypes.addressof(buf), 0, []
        while off < len(data):
            r, rb = self.decode(base + off, len(data) - off)
            trace.append((r, rb))
            off += rb
            if r == H264BSD_PIC_RDY and drain:
                while True:
                    pic = self.next_output_picture() if on_picture is not None else None
                    if pic is None:
                        break
                    on_picture(*pic)
            elif r >= H264BSD_ERROR:
                break
        return trace


class BatchDriver:
    """Advance many Decoder instances picture by picture on the library's parser threads
    (h264bsdmiDecodePictureBatch): one call parses the next picture of every stream that still has data."""

    def __init__(self, decoders, streams):
        """streams: one bytes object per decoder (each is copied once into a private buffer)"""
        self.L = api_lib()
        self.n = len(decoders)
        self.decoders = decoders
        self._bufs = [ctypes.create_string_buffer(b, len(b)) for b in streams]
        self.size = [len(b) for b in streams]
        self.off = [0] * self.n
        self.pictures = [0] * self.n
        VP = ctypes.c_void_p * self.n
        U32 = ctypes.c_uint32 * self.n
        self._dec = VP(*[d._st for d in decoders])
        self._ptr, self._len, self._pid = VP(), U32(), U32()
        self._status, self._consumed, self._errs = U32(), U32(), U32()
        self._out, self._oid, self._oidr, self._onerr = VP(), U32(), U32(), U32()
        self.pulled = {}
        self._draining = set()

    def step(self, pull=False):
        """parse the next picture of every unfinished stream; returns the indices that produced a picture.
        pull=True: h264bsdmiPullAndDecodePictureBatch — every stream's next output picture is pulled first (self.pulled: stream index ->
        (host pointer, picId, isIdrPic, numErrMbs) of the streams that had one), on the same threads, beside the parsing of the other streams."""
        live = [k for k in range(self.n) if self.off[k] < self.size[k]]
        self.pulled = {}
        if pull:
            # a stream that has consumed its input stays in the batch with len = 0 ("pull only", include/h264bsd_mi355x.h) until a
            # pull comes back empty: the pictures still in its output queue are not silently dropped
            live = live + [k for k in sorted(self._draining) if k not in live]
        if not live:
            return []
        if pull:
            for i, k in enumerate(live):
                self._dec[i] = self.decoders[k]._st
                self._ptr[i] = ctypes.addressof(self._bufs[k]) + min(self.off[k], self.size[k] - 1)
                self._len[i] = self.size[k] - self.off[k]
                self._pid[i] = self.pictures[k]
            rc = self.L.h264bsdmiPullAndDecodePictureBatch(len(live), self._dec, self._out, self._oid, self._oidr, self._onerr,
                                                           self._ptr, self._len, self._pid, self._status, self._consumed, self._errs)
            if rc != 0:
                raise RuntimeError("h264bsdmiPullAndDecodePictureBatch failed")
            ready = []
            for i, k in enumerate(live):
                if self._out[i]:
                    self.pulled[k] = (self._out[i], int(self._oid[i]), int(self._oidr[i]), int(self._onerr[i]))
                elif k in self._draining:
                    self._draining.discard(k)                  # its queue is empty: done
                self.off[k] += self._consumed[i]
                if self.off[k] >= self.size[k] and k not in self._draining and (self._out[i] or self._status[i] == H264BSD_PIC_RDY):
                    self._draining.add(k)                      # input finished: come back for what is still queued
                if self._status[i] == H264BSD_PIC_RDY:
                    self.pictures[k] += 1
                    ready.append(k)
            return ready
        for i, k in enumerate(live):
            self._dec[i] = self.decoders[k]._st
            self._ptr[i] = ctypes.addressof(self._bufs[k]) + self.off[k]
            self._len[i] = self.size[k] - self.off[k]
            self._pid[i] = self.pictures[k]
        rc = self.L.h264bsdmiDecodePictureBatch(len(live), self._dec, self._ptr, self._len, self._pid, self._status,
                                                self._consumed, self._errs)
        if rc != 0:
            raise RuntimeError("h264bsdmiDecodePictureBatch failed")
        ready = []
        for i, k in enumerate(live):
            self.off[k] += self._consumed[i]
            if self._status[i] == H264BSD_PIC_RDY:
                self.pictures[k] += 1
                ready.append(k)
        return ready


def pull_batch(decoders, frame_bytes=None):
    """h264bsdmiNextOutputPictureBatch: the next output picture of every decoder, pulled on the library's threads.
    Returns (pointers, pic ids); with frame_bytes also numpy views of the pinned host pictures (valid until the next decode call)."""
    import numpy as np
    L = api_lib()
    n = len(decoders)
    VP = ctypes.c_void_p * n
    U32 = ctypes.c_uint32 * n
    dec = VP(*[d._st for d in decoders])
    out, ids, idr, nerr = VP(), U32(), U32(), U32()
    if L.h264bsdmiNextOutputPictureBatch(n, dec, out, ids, idr, nerr) != 0:
        raise RuntimeError("h264bsdmiNextOutputPictureBatch failed")
    ptrs = [out[i] for i in range(n)]
    if frame_bytes is None:
        return ptrs, list(ids)
    views = [None if not p else np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (frame_bytes,)) for p in ptrs]
    return views, list(ids)


def _regions_arg(who, n, regions):
    """the regions of pull_regions, pull_motion, pull_stats, pull_change and pull_shift, checked: (K, the Region array); None (one whole window per decoder): (n, None)"""
    if regions is None:
        K, regs = n, None
    else:
        regs = []
        for r in regions:
            r = tuple(r)
            if len(r) != 5 or not all(isinstance(v, int) for v in r):
                raise ValueError(f"{who}: a region is (decoder_index, x, y, w, h) in host integers, not {r}")
            i, x, y, w, h = r
            if not 0 <= i < n or not 1 <= w <= 16384 or not 1 <= h <= 16384 or abs(x) > 16384 or abs(y) > 16384:
                raise ValueError(f"{who}: region {r} names no decoder of the call or is out of range (1 <= w, h <= 16384, |x|, |y| <= 16384)")
            regs.append(Region(i, x, y, w, h))
        K = len(regs)
    if K > 65535:
        raise ValueError(f"{who}: at most 65535 regions per call")
    return K, None if regs is None else (Region * max(K, 1))(*regs)


def _out_and_stream(who, out, shape, dtype, stream, aligned=False):
    """`out` checked (aligned: to 8 bytes as well) or allocated, and the stream the C call gets; returns (out, stream)"""
    import torch
    if out is None:
        out = torch.empty(shape, dtype=dtype, device="cuda")
    elif not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() or (aligned and out.data_ptr() % 8):
        what = "contiguous, 8-byte aligned CUDA uint8" if aligned else f"contiguous CUDA {dtype}"
        raise ValueError(f"{who}: out must be a {what} tensor of shape {shape}")
    if stream is None:
        stream = torch.cuda.current_stream(out.device)
    if not stream.cuda_stream:
        # torch's legacy default stream is handle 0, which the C call reads as "the library's own stream, wait": that stream is not
        # ordered behind torch's work, so what is queued for `out` must be done before the call
        stream.synchronize()
    return out, stream


def _current_pull(name, decoders, K, items, specs, stream, boxes=False, call=True):
    """one pull of current pictures, C entry `name`: K items (a ctypes array, or None) of the decoders, the entry's spec arguments,
    then the stream and the output arrays.  Returns [got[:K], boxes (where the entry has them), current, pic_ids]"""
    n = len(decoders)
    got, box = (ctypes.c_uint32 * max(K, 1))(), (ctypes.c_uint32 * (4 * max(K, 1)))()
    cur, ids = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
    if call:
        rc = getattr(api_lib(), name)(n, (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders]), K, items, *specs, stream.cuda_stream,
                                      got, *([box] if boxes else []), cur, ids)
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc})")
    res = [list(got)[:K]]
    if boxes:
        res.append([tuple(box[4 * k: 4 * k + 4]) if got[k] else None for k in range(K)])
    return res + [list(cur)[:n], list(ids)[:n]]


def _kept_pull(name, decoders, K, regs, specs, stream, call):
    """one pull that may compare against kept pictures, C entry `name`: K regions (a ctypes array, or None) of the decoders, the
    entry's spec arguments, then the stream and the output arrays; call: whether the C call is made at all.  Returns (got[:K], current,
    kept, pic_id, kept_pic_id), the last four per decoder"""
    n = len(decoders)
    got = (ctypes.c_uint32 * max(K, 1))()
    per = [(ctypes.c_uint32 * max(n, 1))() for _ in range(4)]                # current, kept, picId, keptPicId
    if call:
        rc = getattr(api_lib(), name)(n, (ctypes.c_void_p * n)(*[d._st for d in decoders]), K, regs, *specs, stream.cuda_stream, got, *per)
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc})")
    return (list(got)[:K], *[list(a)[:n] for a in per])


def _thresholds(who, threshold, C):
    """threshold (one int, or one per channel of C) as the three words of a spec"""
    thr = [threshold] * 3 if isinstance(threshold, int) else list(threshold) + [0] * (3 - C) if isinstance(threshold, (tuple, list)) else []
    if len(thr) != 3 or not all(isinstance(t, int) and 0 <= t <= 255 for t in thr):
        raise ValueError(f"{who}: threshold is one int in 0..255, or one per channel, not {threshold}")
    return thr


def _tensor_call(who, n, decoders, size, layout, dtype, channels, mean, std, crop, out, stream, colour, colour_range, chroma, unspecified,
                 mode, antialias, fit, pad):
    """the argument checks, the output tensor of n slices, the stream handling and the three specs that pull_tensor and pull_regions
    share; returns (out, spec, colour spec, resize spec or None, stream)"""
    import torch
    if dtype is None:
        dtype = torch.float16
    dtypes = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}
    if dtype not in dtypes or layout not in LAYOUTS or channels not in CHANNELS:
        raise ValueError(f"{who}: unsupported dtype / layout / channels {dtype} {layout} {channels}")
    if colour not in MATRICES or colour_range not in RANGES or chroma not in CHROMA or unspecified not in MATRICES or MATRICES[unspecified] < 2:
        raise ValueError(f"{who}: unsupported colour / colour_range / chroma / unspecified {colour} {colour_range} {chroma} {unspecified}")
    if colour == "reference" and (colour_range != "auto" or chroma != "nearest"):
        raise ValueError(f"{who}: colour='reference' is the reference's conversion: colour_range and chroma do not apply")
    if (mode, bool(antialias)) not in FILTERS or fit not in FITS:
        raise ValueError(f"{who}: unsupported mode / antialias / fit {mode} {antialias} {fit} (bicubic needs antialias=True)")
    pad = tuple(float(p) for p in pad)
    if len(pad) != 3 or not all(0.0 <= p <= 1.0 for p in pad):
        raise ValueError(f"{who}: pad must be three values in [0, 1], not {pad}")
    resized = FILTERS[(mode, bool(antialias))] != 0 or fit != "stretch"
    if resized and size is None:
        raise ValueError(f"{who}: antialias, bicubic and letterbox need a size")
    ch, C = CHANNELS[channels]
    if size is None:
        geo = next((d for d in decoders if d.pic_width()), None)
        if geo is None:
            raise ValueError(f"{who}: size=None needs a decoder that has seen a sequence parameter set")
        flag, _, cw, _, chh = geo.cropping_params()
        H, W = (chh, cw) if crop and flag else (16 * geo.pic_height(), 16 * geo.pic_width())
    else:
        H, W = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    shape = (n, C, H, W) if layout == "NCHW" else (n, H, W, C)
    out, stream = _out_and_stream(who, out, shape, dtype, stream)
    spec = TensorSpec(out.data_ptr(), W, H, LAYOUTS[layout], dtypes[dtype], ch, 1 if crop else 0, 0 if size is None else 1,
                      (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std))
    cs = ColourSpec() if colour == "reference" else ColourSpec(MATRICES[colour], RANGES[colour_range], CHROMA[chroma], MATRICES[unspecified])
    rs = ResizeSpec(FILTERS[(mode, bool(antialias))], FITS[fit], (ctypes.c_float * 3)(*pad)) if resized else None
    return out, spec, cs, rs, stream


def pull_tensor(decoders, size=None, layout="NCHW", dtype=None, channels="RGB", mean=(0, 0, 0), std=(1, 1, 1), crop=True,
                out=None, stream=None, colour="reference", colour_range="auto", chroma="nearest", unspecified="bt601",
                mode="bilinear", antialias=False, fit="stretch", pad=(0.0, 0.0, 0.0), return_boxes=False):
    """h264bsdmiNextOutputTensorBatchResize: the next output picture of every decoder, written by one kernel launch into ONE dense CUDA
    tensor, [N, C, H, W] (layout "NCHW") or [N, H, W, C] ("NHWC"), N = len(decoders), in torch.uint8 / float16 (default) / float32.
    channels: "RGB", "BGR", "RGBA", "BGRA" (NHWC only) or "Y" (the luma samples).  Float outputs are (v / 255 - mean[c]) / std[c].
    size: (height, width) or an int for a square; None = no resize, every source window (the SPS cropping window when crop, else
    the coded frame) must have the size of the first decoder's; otherwise bilinear (align_corners=False, no antialiasing).
    out: a contiguous CUDA tensor of that shape and dtype to write into (None: allocated); decoders that have no picture leave
    their slice of it untouched.  stream: a torch.cuda.Stream (default: the current one) — the call returns without waiting,
    the tensor is valid for work on that stream (torch's legacy default stream: the call waits).
    colour: "reference" (the integer BT.601 conversion of next_output_picture(FMT_RGBA), as h264bsdmiNextOutputTensorBatch), or
    "auto" (each stream's VUI matrix_coefficients; `unspecified` where it names none),
    "bt601", "bt709", "bt2020", "fcc" or "smpte240"; colour_range "auto" (video_full_range_flag), "limited" or "full"; chroma
    "nearest" or "bilinear".  Float outputs are then (v - mean[c]) / std[c] of the colour v in [0, 1], U8 round(255 v).
    mode "bilinear" or "bicubic" (antialias=True only), antialias: torch's interpolate(..., antialias=True) weights; fit "stretch" or
    "letterbox" (aspect preserved, centred, the rest of each picture is pad[c] in [0, 1] before mean / std, per output channel); all
    need a size.  Returns (tensor, got, pic_ids, is_idr, num_err_mbs), lists of ints; return_boxes=True appends, per decoder, the
    (left, top, w, h) of the output rectangle its picture fills, or None where it gave no picture."""
    n = len(decoders)
    out, spec, cs, rs, stream = _tensor_call("pull_tensor", n, decoders, size, layout, dtype, channels, mean, std, crop, out, stream, colour,
                                             colour_range, chroma, unspecified, mode, antialias, fit, pad)
    L = api_lib()
    VP = ctypes.c_void_p * n
    U32 = ctypes.c_uint32 * n
    got, ids, idr, nerr, box = U32(), U32(), U32(), U32(), (ctypes.c_uint32 * (4 * n))()
    rc = L.h264bsdmiNextOutputTensorBatchResize(n, VP(*[d._st for d in decoders]), ctypes.byref(spec), ctypes.byref(cs),
                                                None if rs is None else ctypes.byref(rs), stream.cuda_stream, got, ids, idr, nerr, box)
    if rc != 0:
        raise RuntimeError(f"h264bsdmiNextOutputTensorBatchResize failed ({rc})")
    res = (out, list(got), list(ids), list(idr), list(nerr))
    if return_boxes:
        res += ([tuple(box[4 * i: 4 * i + 4]) if got[i] else None for i in range(n)],)
    return res


def pull_regions(decoders, regions, size, layout="NCHW", dtype=None, channels="RGB", mean=(0, 0, 0), std=(1, 1, 1), crop=True,
                 out=None, stream=None, colour="reference", colour_range="auto", chroma="nearest", unspecified="bt601",
                 mode="bilinear", antialias=False, fit="stretch", pad=(0.0, 0.0, 0.0)):
    """h264bsdmiOutputTensorRegions: boxes of the decoders' CURRENT pictures (the picture each popped last, by any output call, valid
    until that decoder decodes again), resized by one kernel launch into ONE dense CUDA tensor [K, C, H, W] or [K, H, W, C], K =
    len(regions).  regions: a sequence of (decoder_index, x, y, w, h), host integers: the box in luma samples relative to the
    decoder's source window (the SPS cropping window when crop, else the coded frame); it may start at a negative or odd position
    and reach beyond the window, where it reads pad.  Nothing is popped: the call may be repeated on the same pictures.  size (an
    int or (height, width)) is required; every other argument as pull_tensor, with each box in the place of the source window
    (fit="letterbox" keeps the BOX's aspect).  Returns (tensor, got, boxes, current, pic_ids): got[k] = 1 when region k was written
    (0: its decoder has no current picture, its slice is untouched), boxes[k] the (left, top, w, h) of the output rectangle it
    fills or None, current[i] / pic_ids[i] per decoder."""
    if size is None:
        raise ValueError("pull_regions: a size is required")
    n = len(decoders)
    K, regs = _regions_arg("pull_regions", n, list(regions))
    out, spec, cs, rs, stream = _tensor_call("pull_regions", K, decoders, size, layout, dtype, channels, mean, std, crop, out, stream, colour,
                                             colour_range, chroma, unspecified, mode, antialias, fit, pad)
    if rs is None:          # bilinear stretch: still a spec of its own here, the pad is what a box reads outside the picture
        rs = ResizeSpec(FILTERS[("bilinear", False)], FITS["stretch"], (ctypes.c_float * 3)(*[float(p) for p in pad]))
    return (out, *_current_pull("h264bsdmiOutputTensorRegions", decoders, K, regs, (ctypes.byref(spec), ctypes.byref(cs), ctypes.byref(rs)),
                                stream, boxes=True))


def pull_remap(decoders, maps, instances=None, layout="NCHW", dtype=None, channels="RGB", mean=(0, 0, 0), std=(1, 1, 1), crop=True,
               out=None, stream=None, colour="reference", colour_range="auto", chroma="nearest", unspecified="bt601",
               mode="bilinear", border="constant", pad=(0.0, 0.0, 0.0), pop=False):
    """h264bsdmiOutputTensorRemap: the decoders' CURRENT pictures (as for pull_regions) sampled through coordinate maps by one kernel
    launch into ONE dense CUDA tensor [R, C, H, W] or [R, H, W, C].  maps: a contiguous float32 CUDA tensor [R, H, W, 2], or a list
    of R contiguous float32 CUDA tensors [H, W, 2] (a tensor may repeat: one calibration for many pictures); maps[r][i, j] = (x, y),
    the position in luma samples of the decoder's source window (the SPS cropping window when crop, else the coded frame) that
    output pixel (i, j) of slice r is taken from, sample (u, v) AT (u, v): cv2.remap's convention; from a normalised
    grid_sample(align_corners=True) grid, x = (gx + 1) (W_src - 1) / 2 and y = (gy + 1) (H_src - 1) / 2.  The maps are read on
    `stream`: what writes them must be ordered before it.  Nothing is copied or converted: other maps raise ValueError.
    instances[r]: the index of the decoder map r samples (default range(R) when R == len(decoders)).  mode "bilinear" or "nearest";
    border "constant" (pad[c] outside the window, in [0, 1] before mean / std) or "replicate"; a non-finite coordinate gives the pad
    in both.  There is no antialiasing.  pop=True first pops every decoder's next picture (h264bsdmiNextOutputInfo), so that it is
    the current one: undistortion as the first stage.  Every other argument as pull_tensor.  Returns (tensor, got, current, pic_ids):
    got[r] = 1 when slice r was written (0: its decoder has no current picture, the slice is untouched), current[i] / pic_ids[i]
    per decoder."""
    import torch
    n = len(decoders)
    if mode not in REMAP_FILTERS or border not in BORDERS:
        raise ValueError(f"pull_remap: unsupported mode / border {mode} {border}")
    if isinstance(maps, torch.Tensor):
        if maps.dim() != 4:
            raise ValueError("pull_remap: maps must be a [R, H, W, 2] tensor or a list of [H, W, 2] tensors")
        whole, maps = maps, [maps[r] for r in range(maps.shape[0])]
    else:
        whole, maps = None, list(maps)
    R = len(maps)
    if R > 65535:
        raise ValueError("pull_remap: at most 65535 maps per call")
    for t in maps if whole is None else [whole]:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != 2 or \
                t.dim() != (3 if whole is None else 4):
            raise ValueError("pull_remap: a map must be a contiguous float32 CUDA tensor [H, W, 2]; nothing is converted or copied")
    if R and any(tuple(t.shape) != tuple(maps[0].shape) or t.device != maps[0].device for t in maps):
        raise ValueError("pull_remap: every map must have the same [H, W, 2] shape and device")
    if R and any(t.data_ptr() % 8 for t in maps):
        raise ValueError("pull_remap: a map must be 8-byte aligned")
    if instances is None:
        if R != n:
            raise ValueError("pull_remap: instances is required unless there is one map per decoder")
        instances = range(n)
    instances = list(instances)
    if len(instances) != R or not all(isinstance(i, int) and 0 <= i < n for i in instances):
        raise ValueError("pull_remap: instances must name one decoder of the call per map")
    if not R:
        raise ValueError("pull_remap: no maps")
    size = (int(maps[0].shape[0]), int(maps[0].shape[1]))
    if not size[0] or not size[1]:
        raise ValueError("pull_remap: empty maps")
    out, spec, cs, _, stream = _tensor_call("pull_remap", R, decoders, size, layout, dtype, channels, mean, std, crop, out, stream, colour,
                                            colour_range, chroma, unspecified, "bilinear", False, "stretch", pad)
    if out.device != maps[0].device:
        raise ValueError("pull_remap: the maps and out must be on the same device")
    rs = RemapSpec(REMAP_FILTERS[mode], BORDERS[border], (ctypes.c_float * 3)(*[float(p) for p in pad]))
    if pop:
        for d in decoders:
            d.next_output_info()
    items = (Remap * R)(*[Remap(i, t.data_ptr()) for i, t in zip(instances, maps)])
    return (out, *_current_pull("h264bsdmiOutputTensorRemap", decoders, R, items, (ctypes.byref(spec), ctypes.byref(cs), ctypes.byref(rs)), stream))


def affine_maps(theta, size, device="cuda"):
    """Maps for pull_remap from affine transforms: theta [R, 2, 3] (anything torch.as_tensor takes), size (H, W) or an int; output
    pixel (i, j) of map r is taken from theta[r] @ (j, i, 1) = (x, y) in luma samples of the source window.  Built in float64, then
    rounded to float32 once.  Returns a contiguous float32 tensor [R, H, W, 2] on `device`."""
    import torch
    H, W = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    theta = torch.as_tensor(theta, dtype=torch.float64, device="cpu")
    if theta.dim() != 3 or tuple(theta.shape[1:]) != (2, 3) or H < 1 or W < 1:
        raise ValueError("affine_maps: theta must be [R, 2, 3] and the size positive")
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    base = torch.stack([j, i, torch.ones_like(i)], dim=-1)                # [H, W, 3]
    maps = torch.einsum("rkc,hwc->rhwk", theta, base)                     # [R, H, W, 2]
    return maps.to(torch.float32).contiguous().to(device)


def pull_motion(decoders, regions=None, size=None, layout="NCHW", dtype=None, planes=("mv", "valid"), crop=True, fit="stretch",
                sampler="nearest", units="source", per_picture=False, out=None, stream=None):
    """h264bsdmiOutputMotionRegions: the decoded motion field of the decoders' CURRENT pictures (Decoder(..., motion=True)), sampled
    by one kernel launch into ONE dense CUDA tensor [K, C, H, W] or [K, H, W, C] in torch.float16 (default) / float32 that lies
    pixel for pixel over what pull_regions gives for the same regions, size, crop and fit.  regions as for pull_regions; None: one
    region per decoder, its whole source window.  size: an int or (height, width); None (regions=None, one common window W x H
    only): the native grid of one value per 4x4 block, ceil(H / 4) x ceil(W / 4).  planes: a subset of "mv" (2 channels: dx, dy in
    luma samples, the displacement of the reference as coded), "valid", "age" (decoded pictures back to the reference), "qp"; the
    channels come in that order whatever the order given.  sampler "nearest" or "area"; units "source" or "output" (pixels of the
    output rectangle); per_picture: dx, dy divided by max(age, 1).  Returns what pull_regions returns."""
    import torch
    n = len(decoders)
    if dtype is None:
        dtype = torch.float16
    dtypes = {torch.float16: 1, torch.float32: 2}
    planes = (planes,) if isinstance(planes, str) else tuple(planes)
    if dtype not in dtypes or layout not in LAYOUTS or not planes or any(p not in MOTION_PLANES for p in planes):
        raise ValueError(f"pull_motion: unsupported dtype / layout / planes {dtype} {layout} {planes}")
    if fit not in FITS or sampler not in MOTION_SAMPLERS or units not in MOTION_UNITS:
        raise ValueError(f"pull_motion: unsupported fit / sampler / units {fit} {sampler} {units}")
    mask = sum(MOTION_PLANES[p][0] for p in set(planes))
    C = sum(c for bit, c in MOTION_PLANES.values() if mask & bit)
    K, regs = _regions_arg("pull_motion", n, regions)
    if size is None:
        if regs is not None:
            raise ValueError("pull_motion: regions need a size")
        windows = set()
        for d in decoders:
            if d.pic_width():
                flag, _, cw, _, chh = d.cropping_params()
                windows.add((chh, cw) if crop and flag else (16 * d.pic_height(), 16 * d.pic_width()))
        if len(windows) != 1:
            raise ValueError("pull_motion: size=None needs decoders that have seen a sequence parameter set and share one window")
        wh, ww = windows.pop()
        H, W = (wh + 3) // 4, (ww + 3) // 4
    else:
        H, W = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    shape = (K, C, H, W) if layout == "NCHW" else (K, H, W, C)
    out, stream = _out_and_stream("pull_motion", out, shape, dtype, stream)
    spec = MotionSpec(out.data_ptr(), W, H, LAYOUTS[layout], dtypes[dtype], mask, 1 if crop else 0, FITS[fit],
                      MOTION_SAMPLERS[sampler], MOTION_UNITS[units], 1 if per_picture else 0)
    return (out, *_current_pull("h264bsdmiOutputMotionRegions", decoders, K, regs, (ctypes.byref(spec),), stream, boxes=True))


def stats_record_bytes(source, bins):
    """the stride of one record of h264bsdmiOutputRegionStats: 8 + 24 C + 4 C B bytes"""
    if source not in STATS_SOURCES or bins not in STATS_BINS:
        raise ValueError(f"stats_record_bytes: unsupported source / bins {source} {bins}")
    C = STATS_SOURCES[source][1]
    return 8 + 24 * C + 4 * C * bins


class RegionStats:
    """what pull_stats returns: count [R] int32; sum, sumsq [R, C] int64; min, max [R, C] int32; hist [R, C, B] int32 or None — views
    of `records` ([R, stride] uint8, one allocation, the C layout); got [R], current and pic_id per decoder, lists of ints"""

    def __init__(self, records, C, B, got, current, pic_id):
        import torch
        w32, w64 = records.view(torch.int32), records.view(torch.int64)
        self.records = records
        self.count = w32[:, 0]
        self.sum, self.sumsq = w64[:, 1:1 + 3 * C:3], w64[:, 2:2 + 3 * C:3]
        self.min, self.max = w32[:, 6:6 + 6 * C:6], w32[:, 7:7 + 6 * C:6]
        self.hist = w32[:, 2 + 6 * C:].unflatten(1, (C, B)) if B else None
        self.got, self.current, self.pic_id = got, current, pic_id


def pull_stats(decoders, regions=None, source="ycbcr", bins=256, crop=True, out=None, stream=None):
    """h264bsdmiOutputRegionStats: integer statistics of boxes of the decoders' CURRENT pictures (as for pull_regions), computed by one
    kernel launch where the pictures lie — nothing is popped and no pixel is pulled.  regions as for pull_regions; None: one region
    per decoder, its whole source window.  source "y" (1 channel), "ycbcr" or "rgb" (3; the reference's integer conversion); bins
    0 (no histogram), 16, 32, 64, 128 or 256 (bin = value >> (8 - log2 bins)).  A record covers the part of its box inside the
    window: count, and per channel sum, sumsq, min, max (255 / 0 when count is 0) and hist.  out: a contiguous CUDA uint8 tensor
    [R, stats_record_bytes(source, bins)] to write into (None: allocated); records of decoders without a current picture are left
    untouched there (got[r] = 0).  stream as for pull_tensor.  Returns a RegionStats."""
    import torch
    n = len(decoders)
    if source not in STATS_SOURCES or bins not in STATS_BINS:
        raise ValueError(f"pull_stats: unsupported source / bins {source} {bins}")
    src, C = STATS_SOURCES[source]
    K, regs = _regions_arg("pull_stats", n, regions)
    shape = (K, stats_record_bytes(source, bins))
    out, stream = _out_and_stream("pull_stats", out, shape, torch.uint8, stream, aligned=True)
    spec = StatsSpec(out.data_ptr(), src, bins, 1 if crop else 0)
    got, cur, ids = _current_pull("h264bsdmiOutputRegionStats", decoders, K, regs, (ctypes.byref(spec),), stream, call=K > 0)     # no records: no call
    return RegionStats(out, C, bins, got, cur, ids)


def change_record_bytes(source, bins):
    """the stride of one record of h264bsdmiOutputRegionChange: 8 + 32 C + 4 C B bytes"""
    if source not in STATS_SOURCES or bins not in STATS_BINS:
        raise ValueError(f"change_record_bytes: unsupported source / bins {source} {bins}")
    C = STATS_SOURCES[source][1]
    return 8 + 32 * C + 4 * C * bins


def _call_stream(stream):
    """the torch stream a call without an output tensor runs on (as _out_and_stream: the legacy default stream is waited for)"""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    if not stream.cuda_stream:
        stream.synchronize()
    return stream


def keep_pictures(decoders, stream=None):
    """h264bsdmiKeepCurrentPictures: the CURRENT picture of every decoder becomes its kept picture, what pull_change compares later
    pictures with; one launch copies them all.  stream as for pull_tensor.  Returns (kept, pic_ids): per decoder 1 when it had a
    current picture (0: what it kept before stays), and the picId of the picture it keeps now (0: none)."""
    n = len(decoders)
    kept, ids = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
    if n:
        rc = api_lib().h264bsdmiKeepCurrentPictures(n, (ctypes.c_void_p * n)(*[d._st for d in decoders]), _call_stream(stream).cuda_stream, kept, ids)
        if rc != 0:
            raise RuntimeError(f"h264bsdmiKeepCurrentPictures failed ({rc})")
    return list(kept)[:n], list(ids)[:n]


def _spread_spec(spread):
    """the SpreadSpec of blend_pictures(spread=dict(...)), checked as h264bsdmiBlendCurrentPicturesSpread checks it"""
    if not isinstance(spread, dict) or set(spread) - {"gain", "lowest", "highest", "update"}:
        raise ValueError(f"blend_pictures: spread is None or a dict of gain, lowest, highest, update, not {spread}")
    gain, lowest, highest, update = spread.get("gain", 2), spread.get("lowest", 2), spread.get("highest", 255), spread.get("update", "all")
    if any(not isinstance(v, int) or isinstance(v, bool) for v in (gain, lowest, highest)) or not 1 <= gain <= 8 or not 0 <= lowest <= highest <= 255:
        raise ValueError(f"blend_pictures: spread has gain 1..8 and 0 <= lowest <= highest <= 255, not {gain} {lowest} {highest}")
    if update not in SPREAD_UPDATES:
        raise ValueError(f"blend_pictures: spread update is one of {tuple(SPREAD_UPDATES)}, not {update}")
    return SpreadSpec(gain, lowest, highest, SPREAD_UPDATES[update])


def blend_pictures(decoders, shift=4, hold=255, moving_shift=None, count_moving=False, stream=None, spread=None):
    """h264bsdmiBlendCurrentPictures: the CURRENT picture of every decoder is blended into its kept picture, which becomes a running
    average — a background model that pull_change, pull_shift, pull_cells(against="kept") and pull_boxes read as they read a copied
    picture; one launch blends them all.  Per sample the state is S = 256 hi + lo (hi: the kept picture), T = 256 c + 128, and
    S' = S + floor((T - S + 2^(shift-1)) / 2^shift); shift 0..7, 0 copies.  hold 0..255: a luma sample with |c - hi| > hold is moving,
    and so is a chroma sample over one; moving samples take moving_shift instead: None (as shift), 0..7, or "frozen" (left as they
    are).  A decoder without a kept picture starts its model with a copy.  count_moving: also the number of moving luma samples of
    every decoder's coded frame.  stream as for pull_tensor.  Returns (kept, blended, pic_ids): per decoder 1 when it had a current
    picture, 1 when that was blended into an existing kept picture (0: the model started), and the picId the kept picture now carries
    — and with count_moving an int32 CUDA tensor [n] behind them.
    spread=dict(gain=2, lowest=2, highest=255, update="all" | "still" | "none"): h264bsdmiBlendCurrentPicturesSpread — beside the kept
    picture a per-sample noise level V (one byte, read with pull_kept(spread=True)): a luma sample is moving when |c - hi| >
    max(hold, V), and V takes one step a call towards min(255, gain |c - hi|), clamped to lowest..highest — on every sample, on the
    still ones only, or not at all.  V reads as lowest until the first such call and after every plain keep."""
    import torch
    n = len(decoders)
    vspec = None if spread is None else _spread_spec(spread)
    if moving_shift is None:
        moving_shift = shift
    elif moving_shift == "frozen":
        moving_shift = BLEND_FROZEN
    for name, v, top in (("shift", shift, 7), ("hold", hold, 255), ("moving_shift", moving_shift, BLEND_FROZEN)):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= top:
            raise ValueError(f"blend_pictures: {name} is an int in 0..{top}" + (' or "frozen"' if name == "moving_shift" else "") + f", not {v}")
    kept, blended, ids = ((ctypes.c_uint32 * max(n, 1))() for _ in range(3))
    moving = None
    if count_moving:
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            moving = torch.zeros((n,), dtype=torch.int32, device="cuda")
    stream = _call_stream(stream)                       # (behind the fill: the legacy default stream is waited for)
    if n:
        spec = BlendSpec(shift, hold, moving_shift, moving.data_ptr() if count_moving else None)
        decs = (ctypes.c_void_p * n)(*[d._st for d in decoders])
        if vspec is None:
            rc = api_lib().h264bsdmiBlendCurrentPictures(n, decs, ctypes.byref(spec), stream.cuda_stream, kept, blended, ids)
        else:
            rc = api_lib().h264bsdmiBlendCurrentPicturesSpread(n, decs, ctypes.byref(spec), ctypes.byref(vspec), stream.cuda_stream, kept, blended, ids)
        if rc != 0:
            raise RuntimeError(f"h264bsdmiBlendCurrentPictures{'' if vspec is None else 'Spread'} failed ({rc})")
    res = (list(kept)[:n], list(blended)[:n], list(ids)[:n])
    return res + (moving,) if count_moving else res


def pull_kept(decoders, fraction=False, spread=False, stream=None):
    """h264bsdmiOutputKeptPictures: the kept picture of every decoder (keep_pictures, blend_pictures) as the planar I420 coded frame —
    Y, Cb, Cr, what next_output_picture returns for a decoded picture — by one launch: to look at the background.  fraction=True:
    also the low byte of every sample of the background model in the same order (128 where a plain keep came last).  stream as for
    pull_tensor.  Returns per decoder a CUDA uint8 tensor [384 * macroblocks] (with fraction a pair of them), or None where it has no
    kept picture.  spread=True (h264bsdmiOutputKeptSpread, one more launch): per decoder a tuple, with the spread frame of
    blend_pictures(spread=...) appended in the same order — or None in its place where the decoder has no valid spread."""
    import torch
    n = len(decoders)
    stream = _call_stream(stream)
    sizes = [384 * d.pic_width() * d.pic_height() for d in decoders]
    with torch.cuda.stream(stream):
        pics = [torch.empty((b,), dtype=torch.uint8, device="cuda") if b else None for b in sizes]
        fracs = [torch.empty((b,), dtype=torch.uint8, device="cuda") if b and fraction else None for b in sizes]
    got = (ctypes.c_uint32 * max(n, 1))()
    if n:
        ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
        rc = api_lib().h264bsdmiOutputKeptPictures(n, (ctypes.c_void_p * n)(*[d._st for d in decoders]), ptrs(pics), ptrs(fracs) if fraction else None,
                                                   stream.cuda_stream, got, None)
        if rc != 0:
            raise RuntimeError(f"h264bsdmiOutputKeptPictures failed ({rc})")
    res = [None if not got[i] else (pics[i], fracs[i]) if fraction else pics[i] for i in range(n)]
    if not spread:
        return res
    with torch.cuda.stream(stream):
        frames = [torch.empty((b,), dtype=torch.uint8, device="cuda") if b else None for b in sizes]
    has = (ctypes.c_uint32 * max(n, 1))()
    if n:
        rc = api_lib().h264bsdmiOutputKeptSpread(n, (ctypes.c_void_p * n)(*[d._st for d in decoders]), ptrs(frames), stream.cuda_stream, has, None)
        if rc != 0:
            raise RuntimeError(f"h264bsdmiOutputKeptSpread failed ({rc})")
    return [None if r is None else (r if isinstance(r, tuple) else (r,)) + (frames[i] if has[i] else None,) for i, r in enumerate(res)]


def _warp_row_refused(row):
    """what h264bsdmiWarpKeptPictures refuses of one map a b c d e f of Python ints, as a message, or None"""
    a, b, c, d, e, f = row
    if max(abs(a), abs(b), abs(d), abs(e)) > WARP_MAX_COEFFICIENT:
        return f"|a|, |b|, |d|, |e| are at most 16 * 65536, not {(a, b, d, e)}"
    if not (-2 ** 31 <= c < 2 ** 31 and -2 ** 31 <= f < 2 ** 31):
        return f"c and f are int32, not {(c, f)}"
    return None


def warp_coefficients(theta):
    """The maps warp_kept takes, from transforms kept -> current as PointModel.theta() returns them: float64 [n, 2, 3] with
    (u, v) = theta @ (x, y, 1) in window samples.  The warp wants the way back, output -> source: every row is inverted in float64,
    scaled by 65536 and rounded with np.rint.  Returns a list of n entries: an int32 numpy array [6] (a b c d e f, 16.16 fixed point),
    or None for a row that holds a NaN or an infinity or is singular.  A row whose coefficients leave the range of the call (|a|, |b|,
    |d|, |e| <= 16 * 65536; c, f int32) raises ValueError."""
    theta = np.asarray(theta, np.float64)
    if theta.ndim != 3 or theta.shape[1:] != (2, 3):
        raise ValueError(f"warp_coefficients: theta is [n, 2, 3], not {list(theta.shape)}")
    out = []
    for r, ((p, q, tx), (s, t, ty)) in enumerate(theta.tolist()):
        det = p * t - q * s
        if not np.isfinite([p, q, tx, s, t, ty]).all() or det == 0.0 or not np.isfinite(det):
            out.append(None)
            continue
        inv = np.array([t / det, -q / det, (q * ty - t * tx) / det, -s / det, p / det, (s * tx - p * ty) / det], np.float64)
        fixed = np.rint(inv * 65536.0)
        if not np.isfinite(fixed).all():
            raise ValueError(f"warp_coefficients: row {r} has no finite inverse in 16.16 fixed point")
        row = [int(v) for v in fixed]
        refused = _warp_row_refused(row)
        if refused:
            raise ValueError(f"warp_coefficients: row {r}: {refused}")
        out.append(np.array(row, np.int32))
    return out


def warp_kept(decoders, theta=None, coefficients=None, outside="replicate", crop=True, count_outside=False, stream=None):
    """h264bsdmiWarpKeptPictures: the kept picture of every decoder (keep_pictures, blend_pictures) is resampled IN PLACE through an
    affine map, the picture and the fraction of the background model, by one launch — the background moved to where the camera now
    looks, so that pull_change, pull_shift, pull_cells(against="kept"), pull_boxes, pull_flow, pull_matches and blend_pictures read it
    registered on the current picture.  theta: float64 [n, 2, 3] kept -> current, as PointModel.theta() returns it (it goes through
    warp_coefficients); or coefficients: per decoder a b c d e f, int32 in 16.16 fixed point, the map from OUTPUT to SOURCE in luma
    samples of the window (crop: the frame-cropping window, else the coded frame) — an [n, 6] array, or a list whose entries may be
    None.  Bilinear on the 16-bit state S = 256 hi + lo, all integers and exact (tests/warp_model.py restates it); the identity changes
    no byte, whole-sample translations are index shifts.  outside "replicate": a source position outside the window takes the nearest
    sample of it; "current": the output sample takes the CURRENT picture's there, as a starting blend writes it (a decoder without a
    current picture is then left alone).  A decoder whose row is None or NaN is left out of the call, one without a kept picture is
    left alone.  count_outside: also the number of luma samples of every decoder's window whose source was outside.  stream as for
    pull_tensor.  Returns (warped, kept_pic_ids): per decoder 1 when its kept picture was resampled, and the picId it carries (0: it
    has none) — and with count_outside an int32 CUDA tensor [n] behind them.  Repeated resampling softens the picture; the 16-bit
    state delays that and does not remove it."""
    import torch
    n = len(decoders)
    if (theta is None) == (coefficients is None):
        raise ValueError("warp_kept: give theta or coefficients, one of them")
    if outside not in WARP_OUTSIDE:
        raise ValueError(f'warp_kept: outside is "replicate" or "current", not {outside!r}')
    rows = warp_coefficients(theta) if coefficients is None else [None if c is None else np.asarray(c) for c in coefficients]
    if len(rows) != n:
        raise ValueError(f"warp_kept: {len(rows)} maps for {n} decoders")
    for r, row in enumerate(rows):
        if row is None:
            continue
        if row.shape != (6,) or row.dtype.kind not in "iu":
            raise ValueError(f"warp_kept: row {r} of coefficients is six integers, not {row.dtype} {list(row.shape)}")
        refused = _warp_row_refused([int(v) for v in row])
        if refused:
            raise ValueError(f"warp_kept: row {r}: {refused}")
    sel = [i for i in range(n) if rows[i] is not None]
    m = len(sel)
    warped, ids = [0] * n, [0] * n
    counts = None
    if count_outside:
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
            part = torch.zeros((max(m, 1),), dtype=torch.int32, device="cuda")
    stream = _call_stream(stream)                       # (behind the fill: the legacy default stream is waited for)
    if m:
        maps = (WarpMap * m)(*[WarpMap(*[int(v) for v in rows[i]]) for i in sel])
        spec = WarpSpec(maps, WARP_OUTSIDE[outside], 1 if crop else 0, part.data_ptr() if count_outside else None)
        got, kid = (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
        rc = api_lib().h264bsdmiWarpKeptPictures(m, (ctypes.c_void_p * m)(*[decoders[i]._st for i in sel]), ctypes.byref(spec), stream.cuda_stream,
                                                 got, kid)
        if rc == -1:
            raise ValueError("warp_kept: h264bsdmiWarpKeptPictures refused the call (a decoder in capture mode, a decoder named twice)")
        if rc != 0:
            raise RuntimeError(f"h264bsdmiWarpKeptPictures failed ({rc})")
        for k, i in enumerate(sel):
            warped[i], ids[i] = got[k], kid[k]
        if count_outside:
            with torch.cuda.stream(stream):
                counts[torch.tensor(sel, dtype=torch.int64, device="cuda")] = part[:m]
    return (warped, ids, counts) if count_outside else (warped, ids)


class RegionChange:
    """what pull_change returns: count [R] int32; sad, ssd, sum [R, C] int64; max, above [R, C] int32; hist [R, C, B] int32 or None —
    views of `records` ([R, stride] uint8, one allocation, the C layout); got [R], and per decoder current, kept, pic_id, kept_pic_id,
    lists of ints"""

    def __init__(self, records, C, B, got, current, kept, pic_id, kept_pic_id):
        import torch
        w32, w64 = records.view(torch.int32), records.view(torch.int64)
        self.records = records
        self.count = w32[:, 0]
        self.sad, self.ssd, self.sum = w64[:, 1:1 + 4 * C:4], w64[:, 2:2 + 4 * C:4], w64[:, 3:3 + 4 * C:4]
        self.max, self.above = w32[:, 8:8 + 8 * C:8], w32[:, 9:9 + 8 * C:8]
        self.hist = w32[:, 2 + 8 * C:].unflatten(1, (C, B)) if B else None
        self.got, self.current, self.kept, self.pic_id, self.kept_pic_id = got, current, kept, pic_id, kept_pic_id

    def mse(self):
        """[R, C] float64: ssd / count (nan where count is 0)"""
        import torch
        return self.ssd.to(torch.float64) / self.count.to(torch.float64)[:, None]

    def psnr(self):
        """[R, C] float64 in dB against a peak of 255: inf where ssd is 0"""
        import torch
        return 10.0 * torch.log10(255.0 * 255.0 / self.mse())


def pull_change(decoders, regions=None, source="y", bins=0, threshold=0, crop=True, keep=False, out=None, stream=None):
    """h264bsdmiOutputRegionChange: integer statistics of (current picture - kept picture, keep_pictures) over boxes, computed by one
    kernel launch where the two pictures lie — nothing is popped and no pixel is pulled.  regions, source, bins, crop, out and stream as
    for pull_stats (out: [R, change_record_bytes(source, bins)]).  threshold: one int 0..255 or one per channel; `above` counts the
    samples with |d| > threshold.  A record: count, per channel sad, ssd, sum (signed), max, above and hist of |d|.  got[r] = 1 only
    where the decoder has a current AND a kept picture: other records are left untouched.  keep=True: behind the comparison the
    current pictures become the kept ones (decoders without a kept picture included: a per-picture loop starts itself); kept and
    kept_pic_id report what the comparison saw.  Returns a RegionChange."""
    import torch
    n = len(decoders)
    if source not in STATS_SOURCES or bins not in STATS_BINS:
        raise ValueError(f"pull_change: unsupported source / bins {source} {bins}")
    src, C = STATS_SOURCES[source]
    thr = _thresholds("pull_change", threshold, C)
    K, regs = _regions_arg("pull_change", n, regions)
    shape = (K, change_record_bytes(source, bins))
    out, stream = _out_and_stream("pull_change", out, shape, torch.uint8, stream, aligned=True)
    spec = ChangeSpec(out.data_ptr(), src, bins, 1 if crop else 0, (ctypes.c_uint32 * 3)(*thr), 1 if keep else 0)
    return RegionChange(out, C, bins, *_kept_pull("h264bsdmiOutputRegionChange", decoders, K, regs, (ctypes.byref(spec),), stream, n > 0))


def shift_record_bytes(radius, surface):
    """the stride of one record of h264bsdmiOutputRegionShift: 32 bytes, with the surface 32 + 4 (D D + 1), D = 2 radius + 1"""
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= SHIFT_MAX_RADIUS:
        raise ValueError(f"shift_record_bytes: radius is an int in 0..{SHIFT_MAX_RADIUS}, not {radius}")
    D = 2 * radius + 1
    return 32 + 4 * (D * D + 1) if surface else 32


class RegionShift:
    """what pull_shift returns: count, dx, dy, best, still, ties [R] int32 (best and still are u32 in the record: above 2^31 they read
    negative, as the u32 fields of RegionChange do; & 0xFFFFFFFF in int64 gives the value); surface [R, D, D] int32 or None,
    surface[r, dy + radius, dx + radius] — views of `records` ([R, stride] uint8, one allocation, the C layout); got [R], and per decoder
    current, kept, pic_id, kept_pic_id, lists of ints"""

    def __init__(self, records, radius, surface, got, current, kept, pic_id, kept_pic_id):
        import torch
        w32 = records.view(torch.int32)
        D = 2 * radius + 1
        self.records, self.radius = records, radius
        self.count, self.dx, self.dy, self.best, self.still, self.ties = w32[:, 0], w32[:, 2], w32[:, 3], w32[:, 4], w32[:, 5], w32[:, 6]
        self.surface = w32[:, 8:8 + D * D].unflatten(1, (D, D)) if surface else None
        self.got, self.current, self.kept, self.pic_id, self.kept_pic_id = got, current, kept, pic_id, kept_pic_id

    def moved(self, regions):
        """the regions the call was given, each translated by its (dx, dy), for those with got: (decoder_index, x + dx, y + dy, w, h),
        ready for pull_regions / pull_stats / pull_shift — the tracking step.  After pull_shift(regions=None) the records are of whole
        windows, whose sizes this object does not hold: pass them as [(i, 0, 0, W_i, H_i), ...] (None raises ValueError).  One copy of
        two columns to the host."""
        if regions is None:
            raise ValueError("RegionShift.moved: pass the regions of the call; after regions=None, the windows as [(i, 0, 0, W, H), ...]")
        regions = [tuple(r) for r in regions]
        if len(regions) != len(self.got):
            raise ValueError(f"RegionShift.moved: {len(regions)} regions for {len(self.got)} records")
        d = self.records.view(self.count.dtype)[:, 2:4].cpu().tolist()
        return [(i, x + d[k][0], y + d[k][1], w, h) for k, (i, x, y, w, h) in enumerate(regions) if self.got[k]]


def pull_shift(decoders, regions=None, radius=4, crop=True, surface=False, keep=False, out=None, stream=None):
    """h264bsdmiOutputRegionShift: where the boxes of the decoders' KEPT pictures (keep_pictures) lie in their CURRENT pictures — a SAD
    search over every displacement |dx|, |dy| <= radius (0..16) in luma, by one kernel launch where the two pictures lie; nothing is
    popped and no pixel is pulled.  regions, crop, out and stream as for pull_change (w, h <= 4096; out: [R, shift_record_bytes(radius,
    surface)]).  A record: count, the displacement (dx, dy) of the smallest SAD (ties: the smallest dx^2 + dy^2, then dy, then dx),
    best = that SAD, still = SAD(0, 0), ties, and with surface=True all (2 radius + 1)^2 SADs.  The current picture is replicated at
    the border of the source window.  got[r] = 1 only where the decoder has a current AND a kept picture: other records are left
    untouched.  keep=True: behind the search the current pictures become the kept ones, as for pull_change.  Returns a RegionShift."""
    import torch
    n = len(decoders)
    K, regs = _regions_arg("pull_shift", n, regions)
    if regs is not None and any(r.w > SHIFT_MAX_SIDE or r.h > SHIFT_MAX_SIDE for r in regs[:K]):
        raise ValueError(f"pull_shift: a region is at most {SHIFT_MAX_SIDE} x {SHIFT_MAX_SIDE}")
    shape = (K, shift_record_bytes(radius, surface))
    out, stream = _out_and_stream("pull_shift", out, shape, torch.uint8, stream, aligned=True)
    spec = ShiftSpec(out.data_ptr(), radius, 1 if surface else 0, 1 if crop else 0, 1 if keep else 0)
    return RegionShift(out, radius, bool(surface),
                       *_kept_pull("h264bsdmiOutputRegionShift", decoders, K, regs, (ctypes.byref(spec),), stream, n > 0))


def corners_record_bytes(max_points):
    """the stride of one record of h264bsdmiOutputCornerPoints: 32 + 16 K bytes, K = max_points"""
    if not isinstance(max_points, int) or isinstance(max_points, bool) or not 1 <= max_points <= CORNERS_MAX_POINTS:
        raise ValueError(f"corners_record_bytes: max_points is an int in 1..{CORNERS_MAX_POINTS}, not {max_points}")
    return 32 + 16 * max_points


class CornerPoints:
    """what pull_corners returns: count, found, written [R] int32; energy [R] int64; x, y [R, K] int32 in the regions' coordinates (the
    source window's); score [R, K] int64; the slots from `written` on are zero — views of `records` ([R, stride] uint8, one allocation,
    the C layout); got [R], current and pic_id per decoder, lists of ints"""

    def __init__(self, records, max_points, got, current, pic_id):
        import torch
        w32, w64 = records.view(torch.int32), records.view(torch.int64)
        K = max_points
        self.records, self.max_points = records, K
        self.count, self.found, self.written, self.energy = w32[:, 0], w32[:, 1], w32[:, 2], w64[:, 2]
        self.x, self.y, self.score = w32[:, 8:8 + 4 * K:4], w32[:, 9:9 + 4 * K:4], w64[:, 5:5 + 2 * K:2]
        self.got, self.current, self.pic_id = got, current, pic_id

    def _host(self):
        """(written [R], points [R, K, 2] int64 of x, y, scores [R, K]) as host lists: one copy of the records"""
        import torch
        rec = self.records.cpu()
        w32, w64 = rec.view(torch.int32), rec.view(torch.int64)
        K = self.max_points
        return w32[:, 2].tolist(), w32[:, 8:8 + 4 * K:4].tolist(), w32[:, 9:9 + 4 * K:4].tolist(), w64[:, 5:5 + 2 * K:2].tolist()

    def points(self, r):
        """the written points of record r as a host list of (x, y, score), in the record's order"""
        written, x, y, score = self._host()
        return [(x[r][k], y[r][k], score[r][k]) for k in range(written[r])]

    def regions(self, side, regions):
        """a side x side box around every written point of every record with got: (decoder_index, x - side // 2, y - side // 2, side,
        side), ready for pull_shift / pull_regions / pull_stats; the decoder index comes from `regions`, those of the call (after
        regions=None: the windows as [(i, 0, 0, W_i, H_i), ...], as for RegionShift.moved), to whose origin the points are relative as
        the boxes are.  One copy of the records to the host."""
        if regions is None:
            raise ValueError("CornerPoints.regions: pass the regions of the call; after regions=None, the windows as [(i, 0, 0, W, H), ...]")
        if not isinstance(side, int) or isinstance(side, bool) or side < 1:
            raise ValueError(f"CornerPoints.regions: side is a positive int, not {side}")
        regions = [tuple(r) for r in regions]
        if len(regions) != len(self.got):
            raise ValueError(f"CornerPoints.regions: {len(regions)} regions for {len(self.got)} records")
        written, x, y, _ = self._host()
        return [(reg[0], x[r][k] - side // 2, y[r][k] - side // 2, side, side)
                for r, reg in enumerate(regions) if self.got[r] for k in range(written[r])]


def pull_corners(decoders, regions=None, score="min_eigen", block=3, nms=3, max_points=64, min_score=0, crop=True, out=None, stream=None):
    """h264bsdmiOutputCornerPoints: the corner points of boxes of the decoders' CURRENT pictures — Sobel gradients, the structure tensor
    over block x block samples (3 or 5), the score "min_eigen" (Shi-Tomasi: about twice the smaller eigenvalue) or "harris" (k = 1/16),
    non-maximum suppression within Chebyshev distance nms (1..7), the strongest max_points (1..256) with score > min_score — and the
    gradient energy of every box, by one kernel launch where the pictures lie, in exact integers; nothing is popped and no pixel is
    pulled.  regions, crop, out and stream as for pull_stats (out: [R, corners_record_bytes(max_points)]); the luma is replicated at the
    border of the source window.  Records of decoders without a current picture are left untouched (got[r] = 0).  Returns a
    CornerPoints, whose .regions(side, regions) are boxes for pull_shift on the next picture."""
    import torch
    n = len(decoders)
    ints = lambda *vs: all(isinstance(v, int) and not isinstance(v, bool) for v in vs)
    if score not in CORNER_SCORES or not ints(block, nms, min_score) or block not in (3, 5) or not 1 <= nms <= CORNERS_MAX_NMS:
        raise ValueError(f"pull_corners: unsupported score / block / nms {score} {block} {nms}")
    if not 0 <= min_score < (1 << 63 if score == "harris" else 1 << 64):
        raise ValueError(f"pull_corners: min_score {min_score} is out of range")
    K, regs = _regions_arg("pull_corners", n, regions)
    shape = (K, corners_record_bytes(max_points))
    out, stream = _out_and_stream("pull_corners", out, shape, torch.uint8, stream, aligned=True)
    spec = CornersSpec(out.data_ptr(), CORNER_SCORES[score], block, nms, max_points, 1 if crop else 0, 0, min_score)
    got, cur, ids = _current_pull("h264bsdmiOutputCornerPoints", decoders, K, regs, (ctypes.byref(spec),), stream, call=K > 0)
    return CornerPoints(out, max_points, got, cur, ids)


class CellMaps:
    """what pull_cells returns: maps [R, P, rows, cols] int32, the C layout, and views of it by name: count [R, rows, cols]; per
    requested plane (PICTURE: sum, sumsq, min, max; CHANGE: sad, ssd, dsum, dmax, above; SPREAD: fore, excess, spread) [R, C, rows, cols]; a plane of the mode that
    was not requested is None.  got [R], and per decoder current, kept, pic_id, kept_pic_id, lists of ints"""

    def __init__(self, maps, mode, C, planes, got, current, kept, pic_id, kept_pic_id):
        self.maps, self.mode, self.planes = maps, mode, planes
        at = 0
        for name, bit in CELL_MODE_PLANES[mode].items():
            width = 0 if not planes & bit else 1 if bit == 1 else C
            view = None if not width else maps[:, at] if bit == 1 else maps[:, at:at + C]
            setattr(self, name, view)
            at += width
        self.got, self.current, self.kept, self.pic_id, self.kept_pic_id = got, current, kept, pic_id, kept_pic_id


def _cells_args(who, decoders, regions, cell, grid, source, planes, against, threshold, crop, keep):
    """the argument checks and the grid of pull_cells, for it and for pull_boxes -> (mode, src, C, bits, thr, K, regs, grid)"""
    n = len(decoders)
    if not (against is None or isinstance(against, str)) or against not in CELL_AGAINST:
        raise ValueError(f"{who}: against is None, 'kept' or 'spread', not {against}")
    mode = CELL_AGAINST[against]
    if source not in STATS_SOURCES or cell not in CELL_SIZES:
        raise ValueError(f"{who}: unsupported source / cell {source} {cell}")
    src, C = STATS_SOURCES[source]
    names = (planes,) if isinstance(planes, str) else tuple(planes)
    if not names or any(p not in CELL_MODE_PLANES[mode] for p in names):
        raise ValueError(f"{who}: planes is a non-empty choice of {tuple(CELL_MODE_PLANES[mode])}, not {planes}")
    bits = sum({CELL_MODE_PLANES[mode][p] for p in names})
    thr = _thresholds(who, threshold, C)
    if not mode and (any(thr) or keep):
        raise ValueError(f"{who}: threshold and keep need against='kept'")
    if mode == 2 and (keep or source == "rgb"):
        raise ValueError(f"{who}: against='spread' has sources 'y' and 'ycbcr' and no keep (a plain keep would invalidate the spread it read)")
    K, regs = _regions_arg(who, n, regions)
    if grid is None:
        if regs is not None:
            sizes = [(r.h, r.w) for r in regs[:K]]
        else:
            sizes = []
            for d in decoders:
                flag, _, cw, _, ch = d.cropping_params()
                sizes.append((ch, cw) if crop and flag else (16 * d.pic_height(), 16 * d.pic_width()))
        grid = (max([-(-h // cell) for h, _ in sizes] + [1]), max([-(-w // cell) for _, w in sizes] + [1]))
    if not (isinstance(grid, (tuple, list)) and len(grid) == 2 and all(isinstance(g, int) and 1 <= g <= 4096 for g in grid)):
        raise ValueError(f"{who}: grid is (rows, cols), 1..4096 each, not {grid}")
    return mode, src, C, bits, thr, K, regs, grid


def pull_cells(decoders, regions=None, cell=16, grid=None, source="y", planes=("count", "sum"), against=None, threshold=0, crop=True,
               keep=False, out=None, stream=None):
    """h264bsdmiOutputCellMaps: dense integer maps, one value per cell x cell luma samples, over boxes of the decoders' CURRENT pictures,
    computed by one kernel launch where the pictures lie.  regions, source, crop and stream as for pull_stats.  cell: 4, 8, 16, 32 or 64.
    grid: (rows, cols) of every slice; None: (ceil(h / cell), ceil(w / cell)) of the largest box (regions=None: source window) of the
    call.  against=None: statistics of the picture, planes out of "count", "sum", "sumsq", "min", "max"; against="kept": of d = current -
    kept picture (keep_pictures), planes out of "count", "sad", "ssd", "dsum", "dmax", "above" (#|d| > threshold: one int 0..255 or one
    per channel); against="spread": of |d| against t = max(threshold, V) per sample, V the spread of blend_pictures(spread=...), planes
    out of "count", "fore" (#|d| > t), "excess" (sum of max(0, |d| - t)), "spread" (sum of V); sources "y" and "ycbcr", no keep, and
    got[r] = 0 without a valid spread; keep=True: behind the comparison the current pictures become the kept ones, as for pull_change.  Cell (i, j) of a
    region holds what pull_stats / pull_change give for the box (x + j cell, y + i cell, min(cell, w - j cell), min(cell, h - i cell));
    cells the box or the window do not reach have count 0.  out: a contiguous CUDA int32 tensor [R, P, rows, cols] to write into;
    slices of decoders without a current (against="kept": or kept) picture are left untouched (got[r] = 0).  Returns a CellMaps."""
    import torch
    n = len(decoders)
    mode, src, C, bits, thr, K, regs, grid = _cells_args("pull_cells", decoders, regions, cell, grid, source, planes, against, threshold, crop, keep)
    P = (bits & 1) + C * bin(bits >> 1).count("1")
    shape = (K, P, grid[0], grid[1])
    out, stream = _out_and_stream("pull_cells", out, shape, torch.int32, stream)
    spec = CellsSpec(out.data_ptr(), grid[1], grid[0], cell, src, 1 if crop else 0, mode, bits, (ctypes.c_uint32 * 3)(*thr), 1 if keep else 0)
    return CellMaps(out, mode, C, bits,
                    *_kept_pull("h264bsdmiOutputCellMaps", decoders, K, regs, (ctypes.byref(spec),), stream, n > 0 and K > 0))


class CellShift:
    """what pull_flow returns: maps [R, P, rows, cols] int32, the C layout, and views of it by name, [R, rows, cols] each: count, dx, dy,
    best, still, ties; a plane that was not requested is None.  gain: still - best, computed on the device.  got [R], and per decoder
    current, kept, pic_id, kept_pic_id, lists of ints"""

    def __init__(self, maps, cell, radius, planes, got, current, kept, pic_id, kept_pic_id):
        self.maps, self.cell, self.radius, self.planes = maps, cell, radius, planes
        at = 0
        for name, bit in FLOW_PLANES.items():
            setattr(self, name, maps[:, at] if planes & bit else None)
            at += 1 if planes & bit else 0
        self.got, self.current, self.kept, self.pic_id, self.kept_pic_id = got, current, kept, pic_id, kept_pic_id

    @property
    def gain(self):
        """[R, rows, cols] int32: still - best, what the best displacement explains of the change; 0 where nothing moved or nothing helps"""
        if self.still is None or self.best is None:
            raise ValueError("CellShift.gain: needs the planes 'still' and 'best'")
        return self.still - self.best


def pull_flow(decoders, regions=None, cell=16, grid=None, radius=4, planes=("dx", "dy", "best"), crop=True, keep=False, out=None, stream=None):
    """h264bsdmiOutputCellShift: dense block-matching motion maps — for every cell x cell luma samples of boxes of the decoders' KEPT
    pictures (keep_pictures, blend_pictures) where it lies in their CURRENT pictures, pull_shift's SAD search over every displacement
    |dx|, |dy| <= radius (0..16) once per cell, by one kernel launch where the two pictures lie; nothing is popped and no pixel is
    pulled.  regions, crop and stream as for pull_shift (no limit on w, h beyond the regions' own); cell: 8, 16, 32 or 64; grid as for
    pull_cells.  planes out of "count", "dx", "dy", "best", "still", "ties".  Cell (i, j) of a region holds what pull_shift gives for the
    box (x + j cell, y + i cell, min(cell, w - j cell), min(cell, h - i cell)); the current picture is replicated at the border of the
    source window, not of the cell; cells the box or the window do not reach have count 0, (0, 0) and ties (2 radius + 1)^2.  out: a
    contiguous CUDA int32 tensor [R, P, rows, cols] to write into; slices of decoders without a current or without a kept picture are
    left untouched (got[r] = 0).  keep=True: behind the search the current pictures become the kept ones, as for pull_change.  Returns
    a CellShift."""
    import torch
    n = len(decoders)
    if cell not in FLOW_CELL_SIZES:
        raise ValueError(f"pull_flow: cell is one of {FLOW_CELL_SIZES}, not {cell}")
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= SHIFT_MAX_RADIUS:
        raise ValueError(f"pull_flow: radius is an int in 0..{SHIFT_MAX_RADIUS}, not {radius}")
    names = (planes,) if isinstance(planes, str) else tuple(planes)
    if not names or any(p not in FLOW_PLANES for p in names):
        raise ValueError(f"pull_flow: planes is a non-empty choice of {tuple(FLOW_PLANES)}, not {planes}")
    bits = sum({FLOW_PLANES[p] for p in names})
    _, _, _, _, _, K, regs, grid = _cells_args("pull_flow", decoders, regions, cell, grid, "y", ("count",), "kept", 0, crop, keep)
    shape = (K, bin(bits).count("1"), grid[0], grid[1])
    out, stream = _out_and_stream("pull_flow", out, shape, torch.int32, stream)
    spec = CellShiftSpec(out.data_ptr(), grid[1], grid[0], cell, radius, bits, 1 if crop else 0, 1 if keep else 0)
    return CellShift(out, cell, radius, bits,
                     *_kept_pull("h264bsdmiOutputCellShift", decoders, K, regs, (ctypes.byref(spec),), stream, n > 0 and K > 0))


def matches_record_bytes(max_points):
    """the stride of one record of h264bsdmiOutputPointMatches: 32 + 80 K bytes, K = max_points"""
    if not isinstance(max_points, int) or isinstance(max_points, bool) or not 1 <= max_points <= MATCHES_MAX_POINTS:
        raise ValueError(f"matches_record_bytes: max_points is an int in 1..{MATCHES_MAX_POINTS}, not {max_points}")
    return 32 + 80 * max_points


def descriptor_pattern():
    """h264bsdmiDescriptorPattern: the 256 tests (px, py, qx, qy) of the binary descriptor, [256, 4] int8 (numpy; needs no device)"""
    p = api_lib().h264bsdmiDescriptorPattern()
    return np.ctypeslib.as_array(p, (256, 4)).copy()


class PointMatches:
    """what pull_matches returns: kept_valid, current_valid, accepted, mutual, sum_dx, sum_dy [R] int32; j, best, second, flags [R, K]
    int32 (j = -1 and best = second = 257 where a kept slot is invalid or has no candidate; flags: MATCH_FLAGS); kept_descriptors,
    current_descriptors [R, K, 32] uint8 — views of `records` ([R, stride] uint8, one allocation, the C layout); got [R], and per decoder
    current, kept, pic_id, kept_pic_id, lists of ints.  Slot indices are those of the point records"""

    def __init__(self, records, max_points, got, current, kept, pic_id, kept_pic_id):
        import torch
        w32 = records.view(torch.int32)
        K = max_points
        self.records, self.max_points = records, K
        self.kept_valid, self.current_valid, self.accepted, self.mutual, self.sum_dx, self.sum_dy = (w32[:, k] for k in range(6))
        self.j, self.best, self.second, self.flags = (w32[:, 8 + k:8 + 4 * K:4] for k in range(4))
        self.kept_descriptors = records[:, 32 + 16 * K:32 + 48 * K].unflatten(1, (K, 32))
        self.current_descriptors = records[:, 32 + 48 * K:32 + 80 * K].unflatten(1, (K, 32))
        self.got, self.current, self.kept, self.pic_id, self.kept_pic_id = got, current, kept, pic_id, kept_pic_id

    @staticmethod
    def _points(who, points, R, K):
        """x, y [R, K] of point records (a CornerPoints or a tensor of records) as host lists"""
        import torch
        rec = points.records if isinstance(points, CornerPoints) else points
        if tuple(rec.shape) != (R, 32 + 16 * K):
            raise ValueError(f"{who}: the point records are not those of the call ({tuple(rec.shape)} for {(R, 32 + 16 * K)})")
        w32 = rec.cpu().contiguous().view(torch.int32)
        return w32[:, 8:8 + 4 * K:4].tolist(), w32[:, 9:9 + 4 * K:4].tolist()

    def _accepted(self):
        """(j, best, flags) [R, K] as host lists: one copy of the slots"""
        import torch
        K = self.max_points
        w32 = self.records[:, :32 + 16 * K].cpu().contiguous().view(torch.int32)
        return w32[:, 8:8 + 4 * K:4].tolist(), w32[:, 9:9 + 4 * K:4].tolist(), w32[:, 11:11 + 4 * K:4].tolist()

    def pairs(self, r, kept_points, current_points):
        """the accepted slots of record r as a host list of (xk, yk, xc, yc, distance), in slot order; the point records are those of
        the call"""
        R, K = len(self.got), self.max_points
        xk, yk = self._points("PointMatches.pairs", kept_points, R, K)
        xc, yc = self._points("PointMatches.pairs", current_points, R, K)
        j, best, flags = self._accepted()
        return [(xk[r][i], yk[r][i], xc[r][j[r][i]], yc[r][j[r][i]], best[r][i]) for i in range(K) if flags[r][i] & MATCH_FLAGS["accepted"]]

    def moved(self, side, regions, current_points):
        """a side x side box around the matched current point of every accepted slot of every record with got: (decoder_index,
        x - side // 2, y - side // 2, side, side), ready for pull_shift / pull_regions / pull_stats; regions as for CornerPoints.regions"""
        if regions is None:
            raise ValueError("PointMatches.moved: pass the regions of the call; after regions=None, the windows as [(i, 0, 0, W, H), ...]")
        if not isinstance(side, int) or isinstance(side, bool) or side < 1:
            raise ValueError(f"PointMatches.moved: side is a positive int, not {side}")
        regions = [tuple(r) for r in regions]
        if len(regions) != len(self.got):
            raise ValueError(f"PointMatches.moved: {len(regions)} regions for {len(self.got)} records")
        K = self.max_points
        xc, yc = self._points("PointMatches.moved", current_points, len(self.got), K)
        j, _, flags = self._accepted()
        return [(reg[0], xc[r][j[r][i]] - side // 2, yc[r][j[r][i]] - side // 2, side, side)
                for r, reg in enumerate(regions) if self.got[r] for i in range(K) if flags[r][i] & MATCH_FLAGS["accepted"]]


def _point_records(who, points, K_regions):
    """the point records of pull_matches, checked: (the tensor [R, 32 + 16 K], K)"""
    if isinstance(points, CornerPoints):
        rec, K = points.records, points.max_points
    else:
        rec = points
        import torch
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda or rec.dtype != torch.uint8 or rec.dim() != 2 or not rec.is_contiguous() or \
                rec.data_ptr() % 8 or rec.shape[1] < 48 or (rec.shape[1] - 32) % 16:
            raise ValueError(f"{who}: point records are a CornerPoints or a contiguous, 8-byte aligned CUDA uint8 tensor [R, 32 + 16 K]")
        K = (rec.shape[1] - 32) // 16
    if not 1 <= K <= MATCHES_MAX_POINTS or tuple(rec.shape) != (K_regions, 32 + 16 * K) or not rec.is_contiguous() or rec.data_ptr() % 8:
        raise ValueError(f"{who}: point records of shape {tuple(rec.shape)} for {K_regions} regions (K in 1..{MATCHES_MAX_POINTS}, contiguous, 8-byte aligned)")
    return rec, K


def pull_matches(decoders, kept_points, current_points, regions=None, max_distance=64, ratio=205, max_move=0, mutual=True, crop=True,
                 keep=False, out=None, stream=None):
    """h264bsdmiOutputPointMatches: where the corner points of the decoders' KEPT pictures (keep_pictures) lie in their CURRENT pictures,
    at any distance — a 256-bit binary descriptor per point (comparisons of 5 x 5 box sums around it, a fixed pattern:
    descriptor_pattern()) on either picture and the Hamming matching of the two sets, by two kernel launches where the pictures lie;
    nothing is popped and no pixel is pulled.  kept_points, current_points: the CornerPoints of two pull_corners calls over the same
    regions (on the picture that was then kept, and on the current one) at the same max_points, or their records as CUDA uint8 tensors
    [R, 32 + 16 K].  regions, crop, out and stream as for pull_shift (out: [R, matches_record_bytes(K)]).  A kept slot is matched to the
    current slot of the smallest Hamming distance (then the smallest index) among those within max_move (Chebyshev; 0: anywhere), and
    accepted when that distance is <= max_distance (0..256), below ratio / 256 of the second smallest (ratio 1..256; 256: no test) and,
    with mutual=True, the best among the kept slots for that current slot as well.  got[r] = 1 only where the decoder has a current AND
    a kept picture: other records are left untouched.  keep=True: behind the matching the current pictures become the kept ones.
    Returns a PointMatches; the loop: c0 = pull_corners(decs); keep_pictures(decs); then per picture c1 = pull_corners(decs);
    m = pull_matches(decs, c0, c1, keep=True); c0 = c1."""
    import torch
    n = len(decoders)
    ints = lambda *vs: all(isinstance(v, int) and not isinstance(v, bool) for v in vs)
    if not ints(max_distance, ratio, max_move) or not 0 <= max_distance <= 256 or not 1 <= ratio <= 256 or not 0 <= max_move <= 65535:
        raise ValueError(f"pull_matches: max_distance is an int in 0..256, ratio in 1..256, max_move in 0..65535, not {max_distance} {ratio} {max_move}")
    K, regs = _regions_arg("pull_matches", n, regions)
    if regs is not None and any(r.w > SHIFT_MAX_SIDE or r.h > SHIFT_MAX_SIDE for r in regs[:K]):
        raise ValueError(f"pull_matches: a region is at most {SHIFT_MAX_SIDE} x {SHIFT_MAX_SIDE}")
    krec, P = _point_records("pull_matches", kept_points, K)
    crec, Pc = _point_records("pull_matches", current_points, K)
    if P != Pc:
        raise ValueError(f"pull_matches: the two point records have max_points {P} and {Pc}")
    shape = (K, matches_record_bytes(P))
    out, stream = _out_and_stream("pull_matches", out, shape, torch.uint8, stream, aligned=True)
    spec = MatchesSpec(out.data_ptr(), krec.data_ptr(), crec.data_ptr(), P, max_distance, ratio, max_move, 1 if mutual else 0,
                       1 if crop else 0, 1 if keep else 0, 0)
    return PointMatches(out, P, *_kept_pull("h264bsdmiOutputPointMatches", decoders, K, regs, (ctypes.byref(spec),), stream, n > 0 and K > 0))


def model_record_bytes(max_points):
    """the stride of one record of h264bsdmiOutputPointModel: 128 + 4 K bytes, K = max_points"""
    if not isinstance(max_points, int) or isinstance(max_points, bool) or not 1 <= max_points <= MATCHES_MAX_POINTS:
        raise ValueError(f"model_record_bytes: max_points is an int in 1..{MATCHES_MAX_POINTS}, not {max_points}")
    return 128 + 4 * max_points


class PointModel:
    """what pull_model returns: usable, hypotheses, inliers, found, a, b [R] int32 (a, b: the slots that span the best hypothesis, -1
    where not found, b = -1 for a translation); sums [R, 12] int64 over the inliers, (x, y) the kept and (u, v) the current point:
    Σx, Σy, Σu, Σv, Σxx, Σxy, Σyy, Σxu, Σyu, Σxv, Σyv, Σ(uu + vv); flags [R, K] int32 (MODEL_FLAGS) — usable .. flags are views of
    `records` ([R, 128 + 4 K] uint8, one allocation, the C layout), sums a copy made when it is read (a record is 4-byte aligned only).
    Slot indices are those of the point records; `matches` is the records tensor of the matches the call was given"""

    def __init__(self, records, max_points, model, matches=None):
        import torch
        w32 = records.view(torch.int32)
        self.records, self.max_points, self.model, self.matches = records, max_points, model, matches
        self.usable, self.hypotheses, self.inliers, self.found, self.a, self.b = (w32[:, k] for k in range(6))
        self.flags = w32[:, 32:32 + max_points]

    @property
    def sums(self):
        import torch
        packed = torch.empty((self.records.shape[0], 96), dtype=torch.uint8, device=self.records.device)
        return packed.copy_(self.records[:, 32:128]).view(torch.int64)

    def inlier_slots(self, r):
        """the slots of record r with the inlier flag, ascending, as a host list"""
        return [i for i, f in enumerate(self.flags[r].tolist()) if f & MODEL_FLAGS["inlier"]]

    def pairs(self, r, kept_points, current_points, inliers=True):
        """the matched coordinates (xk, yk, xc, yc) of the inliers of record r — inliers=False: of its usable pairs that are not — as a
        host list in slot order; the point records are those of the call"""
        import torch
        if self.matches is None:
            raise ValueError("PointModel.pairs: this PointModel was not made by pull_model (no matches)")
        R, K = self.records.shape[0], self.max_points
        xk, yk = PointMatches._points("PointModel.pairs", kept_points, R, K)
        xc, yc = PointMatches._points("PointModel.pairs", current_points, R, K)
        j = self.matches[r, 32:32 + 16 * K].cpu().contiguous().view(torch.int32)[0::4].tolist()
        want = MODEL_FLAGS["usable"] | MODEL_FLAGS["inlier"] if inliers else MODEL_FLAGS["usable"]
        return [(xk[r][i], yk[r][i], xc[r][j[i]], yc[r][j[i]]) for i, f in enumerate(self.flags[r].tolist()) if f == want]

    def theta(self, kind="similarity"):
        """the least-squares transform kept -> current of every record's inliers, from `sums` in closed form: float64 numpy [R, 2, 3],
        (u, v) = theta @ (x, y, 1) in window samples, ready for affine_maps.  kind "translation", "similarity" (rotation, uniform
        scale, translation: no reflection) or "affine", whatever the model of the call.  The moments are centred exactly in integers
        (N Σxx - Σx Σx, ...), the normal equations solved in float64.  A row is NaN where nothing was found or the centred moments are
        singular for the kind: a similarity needs two distinct kept points among the inliers, an affine transform three that are not
        collinear"""
        if kind not in ("translation", "similarity", "affine"):
            raise ValueError(f"PointModel.theta: kind is 'translation', 'similarity' or 'affine', not {kind!r}")
        sums, counts, found = self.sums.tolist(), self.inliers.tolist(), self.found.tolist()
        out = np.full((len(sums), 2, 3), np.nan, np.float64)
        for r, (s, N) in enumerate(zip(sums, counts)):
            if not found[r] or N < 1:
                continue
            sx, sy, su, sv, sxx, sxy, syy, sxu, syu, sxv, syv, _ = s
            cxx, cxy, cyy = N * sxx - sx * sx, N * sxy - sx * sy, N * syy - sy * sy        # N^2 x the centred moments, exact
            cxu, cyu, cxv, cyv = N * sxu - sx * su, N * syu - sy * su, N * sxv - sx * sv, N * syv - sy * sv
            if kind == "translation":
                A = ((1.0, 0.0), (0.0, 1.0))
            elif kind == "similarity":
                if cxx + cyy == 0:
                    continue
                re, im = float(cxu + cyv) / float(cxx + cyy), float(cxv - cyu) / float(cxx + cyy)
                A = ((re, -im), (im, re))
            else:
                det = cxx * cyy - cxy * cxy
                if det == 0:
                    continue
                det = float(det)
                A = ((float(cxu * cyy - cyu * cxy) / det, float(cyu * cxx - cxu * cxy) / det),
                     (float(cxv * cyy - cyv * cxy) / det, float(cyv * cxx - cxv * cxy) / det))
            mx, my, mu, mv = sx / N, sy / N, su / N, sv / N
            out[r] = ((A[0][0], A[0][1], mu - A[0][0] * mx - A[0][1] * my), (A[1][0], A[1][1], mv - A[1][0] * mx - A[1][1] * my))
        return out


def pull_model(decoders, matches, kept_points, current_points, model="similarity", tolerance=2, max_scale=0, min_inliers=None, out=None,
               stream=None):
    """h264bsdmiOutputPointModel: which motion the accepted matches of every region agree on — an exhaustive, deterministic, all-integer
    consensus fit of a translation or a similarity (rotation + uniform scale + translation), one kernel launch where the records lie;
    no picture is read and nothing crosses to the host.  decoders: at least one, they only name the device.  matches: the PointMatches
    of pull_matches or its records tensor [R, 32 + 80 K]; kept_points, current_points: the two point arguments that call was given
    (CornerPoints or records [R, 32 + 16 K]).  model "translation" (a hypothesis is one match) or "similarity" (a pair of matches);
    a match is an inlier within `tolerance` (0..255) luma samples of where the hypothesis sends its kept point; max_scale (similarity:
    0, or 256..4096 in 256ths) bounds the scale of a hypothesis and its inverse; found needs min_inliers (None: 1 for a translation, 2
    for a similarity; up to 256).  The best hypothesis has the most inliers, then the smallest slots.  out: [R, model_record_bytes(K)]
    uint8; out and stream as for pull_matches.  Returns a PointModel; the loop:
        c1 = pull_corners(decs)
        m = pull_matches(decs, c0, c1)
        g = pull_model(decs, m, c0, c1)
        maps = affine_maps(g.theta(), (H, W))
        pull_remap(decs, maps)
    gives the current pictures registered on the kept ones."""
    import torch
    n = len(decoders)
    ints = lambda *vs: all(isinstance(v, int) and not isinstance(v, bool) for v in vs)
    if model not in MODEL_KINDS:
        raise ValueError(f"pull_model: model is 'translation' or 'similarity', not {model!r}")
    kind = MODEL_KINDS[model]
    if min_inliers is None:
        min_inliers = 1 + kind
    if not ints(tolerance, max_scale, min_inliers) or not 0 <= tolerance <= 255 or not 1 + kind <= min_inliers <= 256:
        raise ValueError(f"pull_model: tolerance is an int in 0..255 and min_inliers in {1 + kind}..256, not {tolerance} {min_inliers}")
    if max_scale != 0 and (kind == 0 or not 256 <= max_scale <= 4096):
        raise ValueError(f"pull_model: max_scale is 0, or for a similarity an int in 256..4096, not {max_scale}")
    if n < 1 or len({id(d) for d in decoders}) != n or any(not isinstance(d, Decoder) or not d._st for d in decoders):
        raise ValueError("pull_model: decoders are at least one open Decoder, each once")
    mrec = matches.records if isinstance(matches, PointMatches) else matches
    if not isinstance(mrec, torch.Tensor) or not mrec.is_cuda or mrec.dtype != torch.uint8 or mrec.dim() != 2 or not mrec.is_contiguous() or \
            mrec.data_ptr() % 8 or mrec.shape[1] < 112 or (mrec.shape[1] - 32) % 80 or (mrec.shape[1] - 32) // 80 > MATCHES_MAX_POINTS:
        raise ValueError("pull_model: matches are a PointMatches or a contiguous, 8-byte aligned CUDA uint8 tensor [R, 32 + 80 K]")
    R, K = mrec.shape[0], (mrec.shape[1] - 32) // 80
    if R > 65535:
        raise ValueError("pull_model: at most 65535 records per call")
    krec, Pk = _point_records("pull_model", kept_points, R)
    crec, Pc = _point_records("pull_model", current_points, R)
    if Pk != K or Pc != K:
        raise ValueError(f"pull_model: the matches have max_points {K}, the point records {Pk} and {Pc}")
    out, stream = _out_and_stream("pull_model", out, (R, model_record_bytes(K)), torch.uint8, stream, aligned=True)
    spec = ModelSpec(out.data_ptr(), mrec.data_ptr(), krec.data_ptr(), crec.data_ptr(), K, kind, tolerance, max_scale, min_inliers, (ctypes.c_uint32 * 3)())
    _model_call(decoders, R, spec, stream)
    return PointModel(out, K, model, mrec)


def _model_call(decoders, R, spec, stream):
    """the C call of pull_model: what it refuses is a ValueError as well"""
    n = len(decoders)
    rc = api_lib().h264bsdmiOutputPointModel(n, (ctypes.c_void_p * n)(*[d._st for d in decoders]), R, ctypes.byref(spec), stream.cuda_stream)
    if rc == -1:
        raise ValueError("pull_model: h264bsdmiOutputPointModel refused the call (a decoder in capture mode, decoders on several devices)")
    if rc != 0:
        raise RuntimeError(f"h264bsdmiOutputPointModel failed ({rc})")


class CellBoxes:
    """what pull_boxes returns: cells, the CellMaps of the same call; boxes [R, 1 + M, 8] int32, the C layout, with the views header
    [R, 8] (found, written, foreground_cells, dropped, 0, 0, 0, 0) and records [R, M, 8] (x, y, w, h, cells, peak, sum_lo, sum_hi; zero
    beyond `written`); sums() the 64-bit sums; regions() and found, which make ONE small copy of boxes to the host, kept for both"""

    def __init__(self, cells, boxes, instances, stream=None):
        self.cells, self.boxes, self.instances, self.stream = cells, boxes, instances, stream
        self.header, self.records = boxes[:, 0], boxes[:, 1:]
        self._host = None

    def sums(self):
        """[R, M] int64: sum_lo | sum_hi << 32"""
        import torch
        lo, hi = self.records[..., 6].to(torch.int64), self.records[..., 7].to(torch.int64)
        return (lo & 0xFFFFFFFF) | (hi << 32)

    def host(self):
        """boxes as a host int64 array [R, 1 + M, 8] of the unsigned words: copied once, behind the call's stream"""
        if self._host is None:
            import numpy as np
            if self.stream is not None:
                self.stream.synchronize()
            self._host = self.boxes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        return self._host

    @property
    def found(self):
        """per region: the components that remain (0 where got is 0); more than M of them are not all written"""
        return [int(h[0, 0]) if g else 0 for h, g in zip(self.host(), self.cells.got)]

    def regions(self, pad=0):
        """[(decoder_index, x, y, w, h)] of all written boxes in slice order, each grown by pad luma samples a side: regions for
        pull_regions, pull_stats, pull_change, pull_cells (boxes may leave the window: those calls allow it)"""
        import numpy as np
        out = []
        for r, (slice_, g) in enumerate(zip(self.host(), self.cells.got)):
            if not g:
                continue
            rec = slice_[1:1 + int(slice_[0, 1]), :4]
            rows = np.column_stack([np.full(len(rec), self.instances[r]), rec[:, 0] - pad, rec[:, 1] - pad, rec[:, 2] + 2 * pad, rec[:, 3] + 2 * pad])
            out += map(tuple, rows.tolist())
        return out


def pull_boxes(decoders, regions=None, cell=16, grid=None, source="y", planes=("sad",), against="kept", threshold=0,
               plane=None, channel=0, level=0, sense="above", connectivity=8, min_cells=1, max_boxes=64,
               crop=True, keep=False, out=None, boxes_out=None, stream=None):
    """h264bsdmiOutputCellBoxes: pull_cells, and behind it, on the device, the bounding boxes of the connected groups of cells whose
    value in one of the maps passes a level.  decoders ... planes, against, threshold, crop, keep, out and stream as for pull_cells
    (here against defaults to "kept" and planes to ("sad",): where did the picture change).  plane: the map that is thresholded, one of
    planes but not "dsum" (None: the first of planes that is not "count", or "count"); channel: of source (count: 0); sense "above":
    foreground is value > level, "below": value < level, as unsigned 32-bit; cells the box or the window do not reach are never
    foreground.  connectivity 4 or 8; components of fewer than min_cells cells are dropped; the rest are numbered by their first cell
    in raster order and the first max_boxes (1..512) are written.  The grid has at most 16384 cells.  boxes_out: a contiguous CUDA
    int32 tensor [R, 1 + max_boxes, 8] to write into; slices of regions with got[r] = 0 are left untouched.  Returns a CellBoxes."""
    import torch
    n = len(decoders)
    mode, src, C, bits, thr, K, regs, grid = _cells_args("pull_boxes", decoders, regions, cell, grid, source, planes, against, threshold, crop, keep)
    names = (planes,) if isinstance(planes, str) else tuple(planes)
    if plane is None:
        plane = next((p for p in names if p != "count"), "count")
    if plane not in names or plane == "dsum":
        raise ValueError(f"pull_boxes: plane is one of planes and not 'dsum', not {plane}")
    if not isinstance(channel, int) or not 0 <= channel < (1 if plane == "count" else C):
        raise ValueError(f"pull_boxes: channel is 0..{(1 if plane == 'count' else C) - 1} for {plane} of {source}, not {channel}")
    if sense not in BOXES_SENSES or connectivity not in (4, 8):
        raise ValueError(f"pull_boxes: sense is 'above' or 'below' and connectivity 4 or 8, not {sense} {connectivity}")
    if not all(isinstance(v, int) for v in (level, min_cells, max_boxes)) or not 0 <= level < 2 ** 32 or not 1 <= min_cells < 2 ** 32 or \
            not 1 <= max_boxes <= BOXES_MAX_BOXES:
        raise ValueError(f"pull_boxes: level is 0..2^32 - 1, min_cells at least 1, max_boxes 1..{BOXES_MAX_BOXES}, not {level} {min_cells} {max_boxes}")
    if grid[0] * grid[1] > BOXES_MAX_CELLS:
        raise ValueError(f"pull_boxes: a grid of {grid[0]} x {grid[1]} cells is above the cap of {BOXES_MAX_CELLS} cells; use a larger cell or smaller regions")
    P = (bits & 1) + C * bin(bits >> 1).count("1")
    out, stream = _out_and_stream("pull_boxes", out, (K, P, grid[0], grid[1]), torch.int32, stream)
    boxes_out, _ = _out_and_stream("pull_boxes", boxes_out, (K, 1 + max_boxes, 8), torch.int32, stream)
    if boxes_out.device != out.device:
        raise ValueError("pull_boxes: out and boxes_out must be on the same device")
    spec = CellsSpec(out.data_ptr(), grid[1], grid[0], cell, src, 1 if crop else 0, mode, bits, (ctypes.c_uint32 * 3)(*thr), 1 if keep else 0)
    bspec = BoxesSpec(boxes_out.data_ptr(), max_boxes, CELL_MODE_PLANES[mode][plane], channel, BOXES_SENSES[sense], level, connectivity, min_cells)
    res = _kept_pull("h264bsdmiOutputCellBoxes", decoders, K, regs, (ctypes.byref(spec), ctypes.byref(bspec)), stream, n > 0 and K > 0)
    instances = [r.instance for r in regs[:K]] if regs is not None else list(range(K))
    return CellBoxes(CellMaps(out, mode, C, bits, *res), boxes_out, instances, stream)


def job_header(blob):
    """Decode the FjHeader of a frame job (h264bsd_amd/csrc/framejob.h)."""
    import struct
    (magic, total, wmb, hmb, n_mbs, cur, is_idr, n_slots, any_dbk, rec_off, mv_off, lvl_off, idx_off, coef_off,
     n_intra, n_levels, n_coef, n_inter, pic_seq, copy_off, n_copy, gen_off, n_gen, dbk_off, n_dbk, n_gen_uniform, ghost,
     dbk_only, _down, n_gen_quad, mvx_off, n_mvx) = struct.unpack_from("<IIHHIBBBBIIIIIIIIIIIIIIIIIIIIIII", blob, 0)
    if magic != 0x314A4648:
        raise ValueError("not a frame job")
    # FjCopy entries are 8 bytes {u16 mb, u8 slot, u8 count, i16 dx, i16 dy}: macroblocks moved by k_copy
    n_copy_mbs = sum(blob[copy_off + 8 * i + 3] for i in range(n_copy))
    return dict(total_bytes=total, width_mbs=wmb, height_mbs=hmb, n_mbs=n_mbs, cur_slot=cur, is_idr=is_idr,
                n_slots=n_slots, any_deblock=any_dbk, rec_off=rec_off, mv_off=mv_off, lvl_off=lvl_off,
                idx_off=idx_off, coef_off=coef_off, n_intra=n_intra, n_intra_levels=n_levels,
                n_coef_blocks=n_coef, n_inter=n_inter, pic_seq=pic_seq, copy_off=copy_off, n_copy=n_copy,
                gen_off=gen_off, n_gen=n_gen, dbk_off=dbk_off, n_dbk=n_dbk, n_copy_mbs=n_copy_mbs,
                n_gen_uniform=n_gen_uniform, n_gen_quad=n_gen_quad, ghost=ghost, dbk_only=dbk_only, mvx_off=mvx_off, n_mvx=n_mvx)


def job_mvs(blob):
    """The motion vectors of a FINISHED frame job as a dense int16 array [n_mbs][16][2] (raster 4x4 order, quarter samples):
    a macroblock with FJ_PRED_UNIFORM_MV (pred bit 6) carries its one vector in the record (bytes 24..27), the other inter
    macroblocks have sixteen in the sparse section at mvx_off, entry = u32 at bytes 28..31 of the record (framejob.h)."""
    h = job_header(blob)
    n = h["n_mbs"]
    rec = np.frombuffer(blob, dtype=np.uint8, count=n * 32, offset=h["rec_off"]).reshape(n, 32)
    mvx = np.frombuffer(blob, dtype=np.int16, count=h["n_mvx"] * 32, offset=h["mvx_off"]).reshape(h["n_mvx"], 16, 2)
    out = np.zeros((n, 16, 2), dtype=np.int16)
    inter = rec[:, 0] == 0
    one = inter & ((rec[:, 4] & 0x40) != 0)
    mv1 = np.frombuffer(rec[:, 24:28].tobytes(), dtype=np.int16).reshape(n, 2)
    idx = np.frombuffer(rec[:, 28:32].tobytes(), dtype=np.uint32)
    out[one] = mv1[one][:, None, :]
    many = inter & ~one
    out[many] = mvx[idx[many]]
    return out


def capture_stream(data, copy_elision=False):
    """Parse a byte stream on the host only.  Returns (jobs, trace, info): the packed frame job of every
    picture in decode order, the h264bsdDecode call trace, and stream geometry.  copy_elision: leave out the copies that
    would rewrite what the destination frame buffer holds, like a decoder bound to a device does — such jobs are only
    good for an in-order replay from an IDR picture onto persistent frames (Replay), not for rendering a picture alone."""
    jobs = []
    dec = Decoder(capture=jobs.append, copy_elision=copy_elision)
    trace = dec.decode_stream(data, drain=False)
    info = dict(width_mbs=dec.pic_width(), height_mbs=dec.pic_height(), cropping=dec.cropping_params(),
                video_range=dec.video_range(), matrix_coefficients=dec.matrix_coefficients(),
                profile=dec.profile(), sar=dec.sample_aspect_ratio())
    dec.close()
    return jobs, trace, info


def convert(fmt, width, height, yuv):
    """h264bsdConvertToRGBA/BGRA/YCbCrA (fmt 0/1/2) of one host I420 frame, computed on the GPU."""
    if device_count() <= 0:
        raise RuntimeError("h264bsdConvertTo*: no HIP device (no CPU pixel path exists)")
    L = api_lib()
    fn = (L.h264bsdConvertToRGBA, L.h264bsdConvertToBGRA, L.h264bsdConvertToYCbCrA)[fmt]
    src = np.ascontiguousarray(yuv, dtype=np.uint8)
    out = np.zeros(width * height, dtype=np.uint32)
    fn(width, height, src.ctypes.data, out.ctypes.data)
    return out


class Replay:
    """HBM-resident replay set: n_streams private copies of one captured stream (kernels only)."""

    def __init__(self, jobs, n_streams, odd_offset=0, offsets=None, heavy_lanes=0, heavy_delay=4, groups=1):
        """odd_offset: odd-numbered streams run picture (k + odd_offset) % n_pics in tick k ("staggered").
        offsets: first picture of every stream (desynchronised streams); heavy_lanes > 0: mostly intra-coded pictures
        run on extra HIP streams and rejoin heavy_delay ticks later (run() then always runs one whole lap); groups > 1
        (with heavy_lanes > 0): the streams are split into groups that run their own ticks on their own HIP streams."""
        L = lib()
        self._L = L
        self._keep = [ctypes.create_string_buffer(j, len(j)) for j in jobs]
        ptrs = (ctypes.c_void_p * len(jobs))(*[ctypes.addressof(b) for b in self._keep])
        sizes = (ctypes.c_uint32 * len(jobs))(*[len(j) for j in jobs])
        self.n_pics, self.n_streams = len(jobs), n_streams
        self.odd_offset = odd_offset
        if offsets is None:
            offsets = [odd_offset if s & 1 else 0 for s in range(n_streams)]
        self.offsets = [int(o) for o in offsets]
        offs = (ctypes.c_uint32 * n_streams)(*self.offsets)
        self._h = L.h264bsdmiReplayCreateSched(ptrs, sizes, len(jobs), n_streams, offs, heavy_lanes, heavy_delay, groups)
        if not self._h:
            raise RuntimeError("h264bsdmiReplayCreate failed (no HIP device or out of memory)")
        self.frame_bytes = int(L.h264bsdmiReplayFrameBytes(self._h))
        self.job_bytes = int(L.h264bsdmiReplayJobBytes(self._h))

    def reschedule(self, odd_offset=0, offsets=None, heavy_lanes=0, heavy_delay=4, groups=1):
        """Another schedule for the same resident jobs (arguments as in __init__): no second allocation and upload.
        Frame buffers start from zero again."""
        if offsets is None:
            offsets = [odd_offset if s & 1 else 0 for s in range(self.n_streams)]
        self.odd_offset = odd_offset
        self.offsets = [int(o) for o in offsets]
        offs = (ctypes.c_uint32 * self.n_streams)(*self.offsets)
        if self._L.h264bsdmiReplayReschedule(self._h, offs, heavy_lanes, heavy_delay, groups) != 0:
            raise RuntimeError("h264bsdmiReplayReschedule failed")

    def close(self):
        if self._h:
            self._L.h264bsdmiReplayDestroy(self._h)
            self._h = None

    __del__ = close

    def run(self, first=0, count=None):
        count = self.n_pics - first if count is None else count
        if self._L.h264bsdmiReplayRun(self._h, first, count) != 0:
            raise RuntimeError("h264bsdmiReplayRun failed")

    def sync(self):
        if self._L.h264bsdmiReplaySync(self._h) != 0:
            raise RuntimeError("h264bsdmiReplaySync failed")

    def fetch(self, stream, slot):
        out = np.empty(self.frame_bytes, dtype=np.uint8)
        if self._L.h264bsdmiReplayFetch(self._h, stream, slot, out.ctypes.data) != 0:
            raise RuntimeError("h264bsdmiReplayFetch failed")
        return out

    def dbk_records(self, picture, stream):
        """k_dbk alone for tick `picture`: (records [n_mbs, 48], flag bytes [n_mbs]) of `stream` (h264bsdmiReplayDbkRecords)"""
        n = self.frame_bytes // 384
        out = np.empty(n * 48 + ((n + 3) & ~3), dtype=np.uint8)
        if self._L.h264bsdmiReplayDbkRecords(self._h, picture, stream, out.ctypes.data, out.size) != 0:
            raise RuntimeError("h264bsdmiReplayDbkRecords failed")
        return out[:n * 48].reshape(n, 48), out[n * 48:n * 48 + n]

    def checksums(self, slot):
        out = np.empty(self.n_streams, dtype=np.uint64)
        if self._L.h264bsdmiReplayChecksums(self._h, slot, out.ctypes.data) != 0:
            raise RuntimeError("h264bsdmiReplayChecksums failed")
        return out

    def set_convert(self, fmt, trailing=True, hosting=True, conv_waves=0):
        """fmt 0..2: every picture run() produces is converted (hosted by the next tick's k_frame_dbk where possible, a launch of
        its own otherwise); -1: off.  trailing=False: no launch behind the last tick of a run; hosting=False: launches only;
        conv_waves: conversion wavefronts per k_frame_dbk workgroup (0 = the default)."""
        if fmt >= 0:
            fmt |= (0 if trailing else 0x100) | (0 if hosting else 0x200) | ((conv_waves & 15) << 16)
        if self._L.h264bsdmiReplaySetConvert(self._h, fmt) != 0:
            raise RuntimeError("h264bsdmiReplaySetConvert failed")

    def convert_timings(self):
        ms, n = ctypes.c_float(0), ctypes.c_uint32(0)
        if self._L.h264bsdmiReplayConvertTimings(self._h, ctypes.byref(ms), ctypes.byref(n)) != 0:
            raise RuntimeError("h264bsdmiReplayConvertTimings failed")
        return ms.value, n.value

    def convert(self, slot, fmt):
        if self._L.h264bsdmiReplayConvert(self._h, slot, fmt) != 0:
            raise RuntimeError("h264bsdmiReplayConvert failed")

    def fetch_converted(self, stream, n_pixels):
        out = np.empty(n_pixels, dtype=np.uint32)
        if self._L.h264bsdmiReplayFetchConverted(self._h, stream, out.ctypes.data) != 0:
            raise RuntimeError("h264bsdmiReplayFetchConverted failed")
        return out

    def set_groups(self, n):
        if self._L.h264bsdmiReplaySetGroups(self._h, n) != 0:
            raise RuntimeError('h264bsdmiReplaySetGroups failed')

    def set_stages(self, mask):
        self._L.h264bsdmiReplaySetStages(self._h, mask)

    def set_timed_kernels(self, mask):
        """bit k: KERNELS[k] is bracketed by HIP events in the following run() calls (default all)"""
        self._timed_mask = mask & 31
        self._L.h264bsdmiReplaySetTimedKernels(self._h, mask)

    KERNELS = ("k_copy", "k_recon_inter", "k_dbk", "k_frame_intra", "k_frame_dbk")

    def timings(self):
        """HIP-event times of the last run(): {kernel: (ms, launches)} + total_ms"""
        ms = (ctypes.c_float * 6)()
        n = (ctypes.c_uint32 * 5)()
        if self._L.h264bsdmiReplayTimings(self._h, ms, n) != 0:
            raise RuntimeError("h264bsdmiReplayTimings failed")
        tm = getattr(self, "_timed_mask", 31)
        out = {k: (float(ms[i]) if (tm >> i) & 1 else None, int(n[i])) for i, k in enumerate(self.KERNELS)}
        out["total_ms"] = float(ms[5])
        return out
