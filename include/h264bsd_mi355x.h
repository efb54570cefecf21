/*
 * h264bsd_mi355x.h — extensions of the drop-in API that only exist because the pixel path runs on
 * an MI355X: frame-job capture, explicit batching, device-resident output.  Plain C ABI: pointers and sizes only.
 * (The HBM-resident replay sets used for throughput measurement and kernel tests are NOT part of the product library:
 * include/h264bsd_mi355x_bench.h, libh264bsd_mi355x_bench.so.)
 *
 * None of these has a counterpart in the reference (it has no device, no batching: SURVEY.md §2);
 * the seams they expose are the reference's internal ones:
 *   frame job  = input of h264bsdDecodeMacroblock (src/h264bsd_macroblock_layer.c:965) for every
 *                macroblock of a picture + input of h264bsdFilterPicture (src/h264bsd_deblocking.c:575)
 */
#ifndef H264BSD_MI355X_EXT_H
#define H264BSD_MI355X_EXT_H

#include "h264bsd_decoder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- capture: run only the host parser, hand every finished picture's packed frame job to cb ----
 * No GPU is touched.  h264bsdDecode()'s return codes are unchanged; h264bsdNextOutputPicture*()
 * return NULL (there are no pixels).  cb's blob pointer is valid only during the call. */
typedef void (*h264bsdmi_job_cb)(void *user, const u8 *blob, u32 bytes);
u32 h264bsdmiInitCapture(storage_t *pStorage, u32 noOutputReordering, h264bsdmi_job_cb cb, void *user);
/* Pop the next picture of the output queue like h264bsdNextOutputPicture() (reference
 * src/h264bsd_decoder.c:1045-1066 -> h264bsdDpbOutputPicture, src/h264bsd_dpb.c:1415), but return the DPB
 * slot that holds it (the FjHeader.cur_slot of the job that wrote it) instead of pixels; -1 when the queue
 * is empty.  Works in capture mode, where it is the only way to observe the output order. */
int h264bsdmiNextOutputInfo(storage_t *pStorage, u32 *picId, u32 *isIdrPic, u32 *numErrMbs);


/* ---- device-resident output ----
 * The reference hands pictures over as host pointers (h264bsdNextOutputPicture*, src/h264bsd_decoder.c:1045-1161)
 * and leaves cropping to the application (h264bsdCroppingParams, :970-1001).  On an MI355X box the consumer of
 * decoded video is normally another GPU program, so this variant pops the next output picture like
 * h264bsdNextOutputPicture() but leaves it in HBM: 3.13 MB per 1080p frame never cross PCIe. */
#define H264BSDMI_FMT_RGBA   0   /* bytes R,G,B,A   (h264bsdConvertToRGBA)   */
#define H264BSDMI_FMT_BGRA   1
#define H264BSDMI_FMT_YCBCRA 2
#define H264BSDMI_FMT_I420   3   /* planar Y, Cb, Cr as the reference's u8* picture */
typedef struct h264bsdmi_device_picture {
    void *data;               /* DEVICE pointer; valid until the next h264bsdDecode()/h264bsdShutdown() of this instance */
    u32   width, height;      /* in samples, after cropping when requested                               */
    u32   pitch;              /* bytes per row: width for I420 luma (chroma planes: width/2), 4*width otherwise */
    u32   format;
    u32   picId, isIdrPic, numErrMbs;
    void *stream;             /* hipStream_t the producing work ran on; it has been synchronised on return */
} h264bsdmi_device_picture;
/* format: H264BSDMI_FMT_*; crop != 0 applies the SPS frame-cropping rectangle on the device.
 * Frames live in HBM as macroblock tiles, so every picture that is handed out is laid out by one kernel into a
 * per-instance HBM buffer (planar I420 by k_detile, windows and conversions by k_output).  Returns 1 = picture, 0 = no picture, <0 = error. */
int h264bsdmiNextOutputPictureDevice(storage_t *pStorage, int format, int crop, h264bsdmi_device_picture *out);

/* ---- batched device-resident output: the next pictures of n instances as one dense tensor ----
 * What a GPU consumer of many streams (normally a neural network) takes in: the next picture of every instance, colour
 * converted, optionally resized (bilinear) and normalised, written into ONE caller-owned device buffer by ONE kernel launch. */
#define H264BSDMI_LAYOUT_NCHW 0
#define H264BSDMI_LAYOUT_NHWC 1
#define H264BSDMI_DTYPE_U8    0
#define H264BSDMI_DTYPE_F16   1
#define H264BSDMI_DTYPE_F32   2
#define H264BSDMI_CH_RGB  0   /* 3 channels */
#define H264BSDMI_CH_BGR  1   /* 3 channels */
#define H264BSDMI_CH_RGBA 2   /* 4 channels, NHWC only, alpha = 255 (U8) / 1.0 (float, not normalised) */
#define H264BSDMI_CH_BGRA 3   /* 4 channels, NHWC only */
#define H264BSDMI_CH_Y    4   /* 1 channel: the decoded luma sample itself, no colour conversion */
typedef struct h264bsdmi_tensor_spec {
    void *data;                 /* DEVICE pointer, caller-owned, dense: picture i at data + i * C*H*W elements */
    u32   width, height;        /* output size of every picture */
    u32   layout, dtype, channels;
    u32   crop;                 /* 1: the SPS frame-cropping window is the source; 0: the whole coded frame */
    u32   resize;               /* 0: every source window must be width x height exactly; 1: bilinear (align_corners = false, no antialiasing) */
    float mean[3], std[3];      /* float dtypes: out = (v / 255 - mean[c]) / std[c], c = OUTPUT channel; U8: must be 0 / 1 */
} h264bsdmi_tensor_spec;
/* Pop the next output picture of each of n distinct instances, as h264bsdNextOutputPicture() would, and write all of
 * them into spec->data with ONE kernel launch.  Colour: the integer BT.601 conversion of h264bsdNextOutputPictureRGBA, per
 * source pixel, to 8-bit R, G, B; resizing interpolates those 8-bit values in fp32 (h264bsdmiNextOutputTensorBatchColour: the
 * stream's own colour space).
 * stream != NULL: enqueued on that hipStream_t (which must not be capturing), returns without waiting — the data are valid
 * as soon as work on that stream is, and later decoding of these instances waits for the kernel, not for the caller.
 * stream == NULL: on the library's own stream, returns when the data are there.
 * got[i] = 1 when instance i gave a picture (its slice is written), 0 otherwise (its slice is left untouched); picId /
 * isIdrPic / numErrMbs may be NULL.  0 = ok.  <0 = error; nothing was popped and nothing was enqueued.  Errors: an instance
 * in capture mode, repeated instances, data == NULL, a size of 0, a layout / dtype / channels value out of range, RGBA / BGRA
 * with NCHW, U8 with mean != 0 or std != 1, a std of 0, resize == 0 with a source window other than width x height. */
int h264bsdmiNextOutputTensorBatch(u32 n, storage_t *const *pStorage, const h264bsdmi_tensor_spec *spec, void *stream,
                                   u32 *got, u32 *picId, u32 *isIdrPic, u32 *numErrMbs);

/* The colour space of a tensor pull (h264bsdmiNextOutputTensorBatchColour).  Matrices by Kr, Kb (H.264 Table E-5). */
#define H264BSDMI_MATRIX_REFERENCE 0  /* h264bsdNextOutputPictureRGBA's integer BT.601 (the default); other fields must be 0 */
#define H264BSDMI_MATRIX_AUTO      1  /* from the picture's SPS VUI, matrix_coefficients, as h264bsdMatrixCoefficients() reports it */
#define H264BSDMI_MATRIX_BT601     2  /* Kr 0.299,  Kb 0.114   (matrix_coefficients 5, 6) */
#define H264BSDMI_MATRIX_BT709     3  /* Kr 0.2126, Kb 0.0722  (1) */
#define H264BSDMI_MATRIX_BT2020    4  /* Kr 0.2627, Kb 0.0593  (9, non-constant luminance) */
#define H264BSDMI_MATRIX_FCC       5  /* Kr 0.30,   Kb 0.11    (4) */
#define H264BSDMI_MATRIX_SMPTE240  6  /* Kr 0.212,  Kb 0.087   (7) */
#define H264BSDMI_RANGE_AUTO    0     /* video_full_range_flag, as h264bsdVideoRange() reports it: limited when the VUI has no video_signal_type */
#define H264BSDMI_RANGE_LIMITED 1
#define H264BSDMI_RANGE_FULL    2
#define H264BSDMI_CHROMA_NEAREST  0   /* chroma sample (x >> 1, y >> 1), as the reference */
#define H264BSDMI_CHROMA_BILINEAR 1   /* chroma_sample_loc_type 0: co-sited with even luma columns, midway between luma rows */
typedef struct h264bsdmi_colour_spec {
    u32 matrix, range, chroma;
    u32 unspecified;   /* AUTO only: the matrix (BT601..SMPTE240) used when the VUI names none, or one not listed above (0, 2, 3, 8, 10+) */
} h264bsdmi_colour_spec;
/* h264bsdmiNextOutputTensorBatch with a colour space.  colour == NULL or matrix == REFERENCE: exactly h264bsdmiNextOutputTensorBatch.
 * Otherwise, per SOURCE pixel in fp32: limited range Y' = (Y - 16) / 219, Pb = (Cb - 128) / 224, Pr = (Cr - 128) / 224; full range
 * Y' = Y / 255, Pb = (Cb - 128) / 255, Pr = (Cr - 128) / 255; with Kg = 1 - Kr - Kb, R = Y' + 2(1 - Kr) Pr, B = Y' + 2(1 - Kb) Pb,
 * G = Y' - (2 Kb (1 - Kb) / Kg) Pb - (2 Kr (1 - Kr) / Kg) Pr, each clamped to [0, 1] (CH_Y: Y' clamped to [0, 1]).  Bilinear chroma:
 * the chroma of luma sample (x, y) is taken at (x / 2, y / 2 - 1/4), neighbours clamped to the chroma of the source window (the
 * cropping window when crop, as if it were the whole picture).  Resizing interpolates these values (unquantised); then float dtypes
 * write (v - mean[c]) / std[c], U8 rint(255 v).  AUTO matrix and range are resolved per instance from the SPS the window comes
 * from, so one call may mix colour spaces.  Refused as well, before anything is popped: a field out of range, REFERENCE with any
 * other field non-zero, unspecified other than 0 or BT601..SMPTE240, or other than BT601..SMPTE240 with AUTO.  Everything else
 * (stream, fence, got, errors) as h264bsdmiNextOutputTensorBatch. */
int h264bsdmiNextOutputTensorBatchColour(u32 n, storage_t *const *pStorage, const h264bsdmi_tensor_spec *spec,
                                         const h264bsdmi_colour_spec *colour, void *stream,
                                         u32 *got, u32 *picId, u32 *isIdrPic, u32 *numErrMbs);

/* How a source window becomes an output rectangle (h264bsdmiNextOutputTensorBatchResize). */
#define H264BSDMI_FILTER_BILINEAR    0  /* torch bilinear, align_corners=False, antialias=False (what resize = 1 does without a spec) */
#define H264BSDMI_FILTER_BILINEAR_AA 1  /* torch bilinear, antialias=True (triangle filter widened by the downscale factor)            */
#define H264BSDMI_FILTER_BICUBIC_AA  2  /* torch bicubic,  antialias=True (a = -0.5, as PIL)                                           */
#define H264BSDMI_FIT_STRETCH   0       /* the source window fills width x height                                                     */
#define H264BSDMI_FIT_LETTERBOX 1       /* aspect preserved, centred, the rest of the picture is pad                                  */
typedef struct h264bsdmi_resize_spec {
    u32   filter, fit;
    float pad[3];                       /* letterbox border per OUTPUT channel, in [0, 1] before mean / std (CH_Y: pad[0]) */
} h264bsdmi_resize_spec;
/* h264bsdmiNextOutputTensorBatchColour with a resampling filter and a fit.  resize == NULL, and {FILTER_BILINEAR, FIT_STRETCH},
 * are exactly h264bsdmiNextOutputTensorBatchColour; a non-NULL resize needs spec->resize == 1.
 * Weights are torch's (interpolate(..., antialias=True)), with the source window as the input and the inner size as the output: for
 * output index i, scale = in / out, center = scale (i + 0.5), support = (interp / 2) max(scale, 1) with interp 2 (bilinear) or 4
 * (bicubic), taps xmin = max((int)(center - support + 0.5), 0) .. xmax = min((int)(center + support + 0.5), in) (exclusive), tap j
 * weighted filter((j - center + 0.5) / max(scale, 1)) and normalised by the sum of the taps; filter 1 - |x| or Keys' cubic, a = -0.5.
 * FILTER_BILINEAR keeps the coordinates of resize = 1 (two taps per axis) at the inner size.  What is interpolated is what resize = 1
 * interpolates: with colour NULL / REFERENCE the reference's 8-bit R, G, B (or luma), otherwise the unquantised colour value.  Float
 * outputs are then (v - mean[c]) / std[c], unclamped (bicubic may overshoot, as in torch); U8 is clamped to [0, 255] and rounded as
 * resize = 1 rounds.
 * FIT_LETTERBOX, per picture of window w x h, in double: s = min(width / w, height / h), iw = clamp(floor(w s + 0.5), 1, width), ih
 * likewise, left = (width - iw) / 2, top = (height - ih) / 2 (integer division).  The inner iw x ih rectangle is the window resampled
 * to that size; every other pixel is pad[c] under the output's scale (U8 floor(255 pad + 0.5), floats (pad - mean[c]) / std[c]);
 * alpha is 255 / 1.0.  box (may be NULL): 4 u32 per instance, left, top, iw, ih; FIT_STRETCH (and resize == NULL) 0, 0, width,
 * height; an instance with got[i] = 0 leaves its slice untouched, border included, and gets a box of zeros.
 * Refused as well, before anything is popped: filter > 2, fit > 1, a pad that is not finite or lies outside [0, 1], and a non-NULL
 * resize with spec->resize != 1.  Everything else (stream, fence, got, errors) as h264bsdmiNextOutputTensorBatchColour. */
int h264bsdmiNextOutputTensorBatchResize(u32 n, storage_t *const *pStorage, const h264bsdmi_tensor_spec *spec,
                                         const h264bsdmi_colour_spec *colour, const h264bsdmi_resize_spec *resize,
                                         void *stream, u32 *got, u32 *picId, u32 *isIdrPic, u32 *numErrMbs,
                                         u32 *box);

/* Region pulls: boxes of pictures that HAVE BEEN POPPED, each resampled into its own slice of one tensor, with one launch — the
 * second stage of a detector / classifier pipeline, which learns where to look only after the picture has left the output queue.
 * The CURRENT PICTURE of an instance is the picture popped last by any output call (h264bsdNextOutputPicture*,
 * h264bsdmiNextOutputInfo, ...PictureDevice, ...PictureBatch, ...TensorBatch*).  Its frame buffer is intact until the instance
 * decodes again (a pop only advances the output queue; a decode call chooses the buffer of the next picture): it stops being
 * current at the next h264bsdDecode or h264bsdmi*Decode* call that feeds the instance, whatever that call returns (an instance
 * that h264bsdmiPullAndDecodePictureBatch does not feed keeps the picture the call popped), and at h264bsdFlushBuffer,
 * h264bsdShutdown and h264bsdInit — the reference's rule for the pointer h264bsdNextOutputPicture returns.  The call pops
 * nothing and may be repeated on the same picture.
 * Region r reads the current picture of pStorage[regions[r].instance] and fills slice r of spec->data (data + r * C*H*W elements,
 * spec->width x spec->height; layout, dtype, channels, mean, std as for every tensor pull; spec->resize must be 1).  An instance
 * may have any number of regions, or none.  got[r] = 1, or 0 (slice untouched, box of zeros) when that instance has no current
 * picture.  current[i] / picId[i] (each may be NULL): whether instance i has a current picture, and its picId.
 * (x, y) is the box's top-left corner in the instance's source window (the SPS cropping window when spec->crop, else the coded
 * frame), in luma samples, of any parity, and may be negative; the box may reach beyond the window on any side or lie outside it.
 * 1 <= w, h <= 16384, |x|, |y| <= 16384.
 * What is sampled is the w x h picture S: where (x + u, y + v) lies inside the window, S(u, v) is what a tensor pull of the WHOLE
 * window interpolates there (colour NULL / REFERENCE: the reference's 8-bit R, G, B or luma; otherwise the unquantised colour in
 * [0, 1], the neighbours of bilinear chroma clamped to the chroma of the window, not of the box); elsewhere S is the pad
 * (REFERENCE: floor(255 pad[c] + 0.5); otherwise pad[c]; c the output channel).  A region is "convert, pad, crop", in that order.
 * S is then resampled exactly as h264bsdmiNextOutputTensorBatchResize resamples a source window: the same filters and tap rule
 * with n_in = w or h, FIT_STRETCH / FIT_LETTERBOX with the rectangle arithmetic on (w, h), the same output scale, clamping and
 * rounding; box (may be NULL): 4 u32 per REGION.  resize == NULL is {FILTER_BILINEAR, FIT_STRETCH}, pad 0.
 * stream as for the other pulls (not capturing; NULL: the library's own stream, and the call waits).  Later decoding of the
 * sampled instances waits for the kernel, not for the caller.  -1, before anything is enqueued: everything
 * h264bsdmiNextOutputTensorBatchResize refuses in spec, colour and resize; spec->resize != 1; regions or got NULL with
 * nRegions > 0; nRegions > 65535; an instance index >= n; a w or h of 0 or above the limit, an x or y beyond it; an instance in
 * capture mode; repeated instances.  -2: the engine failed. */
typedef struct h264bsdmi_region { u32 instance; int x, y; u32 w, h; } h264bsdmi_region;
int h264bsdmiOutputTensorRegions(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                                 const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec *colour,
                                 const h264bsdmi_resize_spec *resize, void *stream,
                                 u32 *got, u32 *box, u32 *current, u32 *picId);

/* Remapped pulls: the CURRENT pictures (above) sampled through caller-supplied coordinate maps, map r into slice r of one tensor,
 * with one launch — lens undistortion (what cv2.initUndistortRectifyMap produces and cv2.remap consumes), rotated and
 * perspective-rectified crops, polar unwrapping: everything that is "output pixel (i, j) comes from source position (x, y)".  A
 * sibling of h264bsdmiOutputTensorRegions: the same current-picture rule and lifetime, the same got (per MAP) / current / picId
 * (per instance), the same stream rule and fence (one per distinct instance), the same colour handling (NULL / REFERENCE: the
 * reference's 8-bit values; otherwise the unquantised colour, bilinear chroma clamped to the window) and the same spec (layout,
 * dtype, channels, mean / std, crop; spec->resize must be 1).  It pops nothing and may be repeated.  remap == NULL is
 * {REMAP_BILINEAR, BORDER_CONSTANT, pad 0}.
 * maps[r].map is a DEVICE pointer to float32 [spec->height][spec->width][2], dense, x then y, 8-byte aligned.  The kernel reads
 * it on `stream`: it must be complete on that stream and stay valid until the kernel has run.  Several entries may name the same
 * map (one calibration for many pictures) or the same instance.  (mx, my) is a position in luma samples of the source window of
 * instance maps[r].instance (the SPS cropping window when spec->crop, else the coded frame), W x H; sample (u, v) sits AT (u, v):
 * cv2.remap's convention, and grid_sample(align_corners=True)'s after de-normalising, x = (gx + 1) (W - 1) / 2.
 * S(u, v), u, v integers: inside the window what a pull of the whole window interpolates there (as for a region); outside the pad
 * under the scale of the converted samples (REFERENCE floor(255 pad[c] + 0.5), otherwise pad[c]).
 * A non-finite mx or my gives the pad under the OUTPUT's scale (as the letterbox border is written) whatever the border mode; no
 * address is formed.  Otherwise, in fp32: BORDER_CONSTANT cx = min(max(mx, -1), W), BORDER_REPLICATE cx = min(max(mx, 0), W - 1);
 * cy likewise with H.
 * REMAP_BILINEAR: x0 = floor(cx), lx = cx - x0 (exact in fp32 for cx >= 0; for -1 < cx < 0 rounded to nearest, at most 2^-25
 * off), y0, ly likewise; the neighbours are (x0 | x0 + 1, y0 | y0 + 1);
 * one outside the window is the pad (CONSTANT; with REPLICATE such a neighbour only ever carries weight 0 and its index is
 * clamped).  The blend is resize = 1's for the same colour: REFERENCE hy (hx v00 + lx v01) + ly (hx v10 + lx v11), hx = 1 - lx,
 * hy = 1 - ly; otherwise a + l (b - a) along the rows, then between them.  The output encoding is resize = 1's too: REFERENCE U8
 * rounds halves up, REFERENCE floats are (v / 255 - mean) / std, otherwise U8 rint(v) and floats v; alpha is 255 / 1.0.
 * REMAP_NEAREST: xi = floor(cx + 0.5f), the sum rounded in fp32, yi likewise; the value is S(xi, yi) (CONSTANT: the pad outside;
 * REPLICATE: never outside), encoded the same way.
 * There is NO antialiasing: a map that shrinks the picture aliases exactly as cv2.remap does; shrink with
 * h264bsdmiNextOutputTensorBatchResize or a region pull instead, or supersample the map.
 * -1, before anything is enqueued: everything h264bsdmiOutputTensorRegions refuses in spec, colour, instances and stream; maps or
 * got NULL with nMaps > 0; nMaps > 65535; an instance index >= n; a NULL map or one that is not 8-byte aligned; filter > 1 or
 * border > 1; a pad that is not finite or lies outside [0, 1].  nMaps == 0 returns 0 and launches nothing.  -2: the engine failed. */
#define H264BSDMI_REMAP_NEAREST   0
#define H264BSDMI_REMAP_BILINEAR  1
#define H264BSDMI_BORDER_CONSTANT  0   /* outside the window: pad */
#define H264BSDMI_BORDER_REPLICATE 1   /* outside the window: the nearest sample of the window */
typedef struct h264bsdmi_remap      { u32 instance; const void *map; } h264bsdmi_remap;
typedef struct h264bsdmi_remap_spec { u32 filter, border; float pad[3]; } h264bsdmi_remap_spec;
int h264bsdmiOutputTensorRemap(u32 n, storage_t *const *pStorage, u32 nMaps, const h264bsdmi_remap *maps,
                               const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec *colour,
                               const h264bsdmi_remap_spec *remap, void *stream,
                               u32 *got, u32 *current, u32 *picId);

/* Motion-field tensors: the motion vectors the decoder resolved for a picture (P_Skip prediction included), resampled onto the
 * grid of a tensor pull — for carrying boxes across pictures, gating inference on motion, flow-conditioned networks.
 * Keep the motion side information of every picture of this instance beside its frame buffer (74 bytes per macroblock and frame
 * buffer).  Call before the first h264bsdDecode() (like h264bsdmiSetCopyElision).  Off by default: nothing is kept and nothing is
 * launched.  0 = ok, -1: capture mode, or the instance has decoded already. */
int h264bsdmiSetMotionExport(storage_t *pStorage, u32 on);
#define H264BSDMI_MOTION_NEAREST 0   /* the 4x4 block under the output pixel's centre */
#define H264BSDMI_MOTION_AREA    1   /* area-weighted mean over the output pixel's footprint */
#define H264BSDMI_MOTION_PLANE_MV    1u   /* 2 channels: dx, dy */
#define H264BSDMI_MOTION_PLANE_VALID 2u   /* 1 channel */
#define H264BSDMI_MOTION_PLANE_AGE   4u   /* 1 channel */
#define H264BSDMI_MOTION_PLANE_QP    8u   /* 1 channel */
#define H264BSDMI_MOTION_UNITS_SOURCE 0   /* luma samples of the source window */
#define H264BSDMI_MOTION_UNITS_OUTPUT 1   /* pixels of the output rectangle: dx * iw / w, dy * ih / h */
typedef struct h264bsdmi_motion_spec {
    void *data;                 /* DEVICE pointer, caller-owned, dense: region r at data + r * C*H*W elements */
    u32   width, height;        /* output size of every region */
    u32   layout, dtype;        /* H264BSDMI_LAYOUT_*; H264BSDMI_DTYPE_F16 / F32 (U8: refused) */
    u32   planes;               /* non-empty subset of H264BSDMI_MOTION_PLANE_*; channels in the order MV, VALID, AGE, QP */
    u32   crop, fit;            /* as h264bsdmi_tensor_spec.crop; H264BSDMI_FIT_* */
    u32   sampler, units;
    u32   per_picture;          /* 1: dx, dy divided by max(age, 1): displacement per decoded picture */
} h264bsdmi_motion_spec;
/* The motion side information of the instances' CURRENT pictures (above), region by region as h264bsdmiOutputTensorRegions reads
 * their pixels: the same region struct and limits, the same source window, the same rectangle arithmetic for FIT_LETTERBOX (on the
 * box's w, h), the same got / box / current / picId, the same stream rule and fence; it pops nothing and may be repeated.  Slice r
 * of a motion pull lies pixel for pixel over slice r of a region pull with the same regions, size, crop and fit.  regions == NULL
 * with nRegions == n: region i is the whole window of instance i.  The side information is valid exactly as long as the pixels are.
 * Per 4x4 luma block of the coded frame the decoder keeps: whether it is VALID — the block belongs to an inter macroblock (P_Skip
 * included) or to a lost macroblock of a P picture concealed by copying, and its reference is a frame buffer of the sequence;
 * intra, I_PCM, intra-concealed and undecoded macroblocks are invalid — its vector (mx, my) in quarter samples (0 when invalid, 0
 * for a concealed macroblock): the block's samples were predicted from the reference picture displaced by (mx / 4, my / 4) luma
 * samples, the direction as coded (negate for "where did it go"), dx = mx / 4, dy = my / 4; the AGE of its reference: the distance
 * in decoding order to the picture predicted from, clamped to [0, 255], 0 when invalid or unknown (the reference was not decoded
 * since the sequence began); and its macroblock's luma QP (valid or not).  Of a picture decoded from redundant slices, what the
 * reference decoder ends up with.
 * Values, for output pixel (i, j) of the inner rectangle (left, top, iw, ih) of a box (x, y, w, h) in a window W x H that starts at
 * luma sample (x0, y0) of the coded frame; everything outside the inner rectangle is 0 in every plane:
 * NEAREST, integers only: u = ((2 (i - left) + 1) w) / (2 iw), v likewise; window position (x + u, y + v); outside [0, W) x [0, H)
 * all planes 0; else the block ((x0 + x + u) >> 2, (y0 + y + v) >> 2): VALID 1 / 0, MV its vector, AGE its age, QP its QP.
 * AREA: the footprint [x + (i - left) w / iw, x + (i - left + 1) w / iw) x (the same in v), clipped to the window; a block weighs
 * by the area it shares with the clipped footprint.  VALID = weight of the valid blocks / area of the UNCLIPPED footprint
 * (w / iw) (h / ih); MV, AGE = weighted mean over the valid blocks (0 when there is none); QP = weighted mean over all blocks inside
 * the window (0 when the footprint misses the window).  Edges, weights and sums in double, the mean rounded to fp32 once.
 * Then per_picture (per block, before averaging: the fp32 vector component divided by max(age, 1)), then UNITS_OUTPUT (dx times
 * (float) iw / (float) w, dy times (float) ih / (float) h, in fp32), then the dtype (F16: round to nearest even).  No mean / std.
 * -1, before anything is enqueued: everything h264bsdmiOutputTensorRegions refuses in regions, instances and stream; an instance
 * without motion export; data NULL, width or height 0, layout out of range, a dtype other than F16 / F32, planes 0 or with unknown
 * bits, sampler, units, fit or per_picture out of range; regions == NULL with nRegions != n.  -2: the engine failed. */
int h264bsdmiOutputMotionRegions(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                                 const h264bsdmi_motion_spec *spec, void *stream,
                                 u32 *got, u32 *box, u32 *current, u32 *picId);

/* Region statistics: sums, extrema and histograms of boxes of the instances' CURRENT pictures (above), computed where the pictures
 * lie, with one launch — camera health (black, blown out, covered), exposure (the mean and spread to hand the next tensor pull as
 * mean / std), scene cuts (histogram distance between consecutive pictures), the colour of a detector's box — without pulling a
 * pixel.  A sibling of h264bsdmiOutputTensorRegions: the same region struct and limits (1 <= w, h <= 16384, |x|, |y| <= 16384,
 * negative origins, boxes that leave the source window or miss it), the same source window (the SPS cropping window when
 * spec->crop, else the coded frame), the same current-picture rule and lifetime, the same got (per REGION) / current / picId (per
 * instance, each may be NULL), the same stream rule (not capturing; NULL: the library's own stream, and the call waits) and the
 * same fence: later decoding of the instances waits for the kernel, not for the caller.  It pops nothing and may be repeated.
 * regions == NULL with nRegions == n: region i is the whole window of instance i, as in the motion pull.
 * Record r is written at spec->data + r * stride, stride = 8 + 24 C + 4 C B bytes, C = 1 (STATS_Y) or 3 channels in the order of
 * the source, B = spec->bins, little endian:
 *     u32 count; u32 zero;
 *     C x { u64 sum; u64 sumsq; u32 min; u32 max; }
 *     C x B x u32 hist                                   hist[c][b]
 * A record covers every luma position (x + u, y + v), 0 <= u < w, 0 <= v < h, that lies inside the window; count is their number,
 * the same for every channel, at most 2^28; sum and sumsq are over the 8-bit values at those positions (below 2^44), min and max
 * their extrema; hist[c][value >> (8 - log2 B)] counts them, so every hist[c] sums to count.  count == 0 (the box misses the
 * window): sums 0, min 255, max 0, histogram all zero.  Everything is an integer and exact: no order of summation shows.
 * The call writes the WHOLE record with plain stores: the caller does not clear it.  got[r] = 1, or 0 when that instance has no
 * current picture: record r is then untouched.
 * -1, before anything is enqueued: everything h264bsdmiOutputTensorRegions refuses in regions, instances and stream (got NULL
 * with nRegions > 0; nRegions > 65535; an instance index >= n; a w or h of 0 or above the limit, an x or y beyond it; an instance
 * in capture mode; repeated instances; a capturing stream); spec or data NULL, data not 8-byte aligned; source > 2; bins not one of
 * 0, 16, 32, 64, 128, 256; crop > 1; regions == NULL with nRegions != n.  nRegions == 0 returns 0 and launches nothing.  -2: the
 * engine failed. */
#define H264BSDMI_STATS_Y      0   /* 1 channel : the decoded luma sample */
#define H264BSDMI_STATS_YCBCR  1   /* 3 channels: Y, Cb, Cr as decoded; the chroma of luma sample (X, Y) of the coded frame is chroma sample (X >> 1, Y >> 1), as the reference's conversion pairs them */
#define H264BSDMI_STATS_RGB    2   /* 3 channels: R, G, B of h264bsdNextOutputPictureRGBA's integer BT.601 conversion, 8 bit */
typedef struct h264bsdmi_stats_spec {
    void *data;      /* DEVICE pointer, caller-owned, 8-byte aligned: record r at data + r * stride */
    u32   source;    /* H264BSDMI_STATS_* */
    u32   bins;      /* 0 (no histogram), 16, 32, 64, 128 or 256: bin = value >> (8 - log2 bins) */
    u32   crop;      /* as h264bsdmi_tensor_spec.crop */
} h264bsdmi_stats_spec;
int h264bsdmiOutputRegionStats(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                               const h264bsdmi_stats_spec *spec, void *stream,
                               u32 *got, u32 *current, u32 *picId);

/* Kept pictures: one picture per instance that the library holds on to, for h264bsdmiOutputRegionChange below.  A frame buffer stops
 * being current at the next decode call and is decoded into a few pictures later; this call copies the CURRENT picture (above) of
 * each of n distinct instances — the whole coded frame, as it lies on the device — into that instance's kept-picture buffer, with
 * one launch for the call.  The buffer is one frame, owned by the library, allocated at the instance's first keep: instances that never
 * keep pay nothing.  kept[i] = 1 when instance i had a current picture and it was copied, else 0: a picture kept earlier then stays
 * as it was.  picId (may be NULL): the picId of the picture instance i now keeps, or 0.
 * The kept picture survives decoding, popping and h264bsdFlushBuffer.  It is dropped at h264bsdShutdown / h264bsdInit and when a
 * sequence of another coded size is activated; a new sequence of the same coded size keeps it.
 * The stream rule and the fence are those of the pulls of current pictures: not capturing; NULL: the library's own stream, and the call
 * waits; the next decode into the source frame buffer waits for the copy, not for the caller.
 * -1, before anything is enqueued: pStorage NULL or kept NULL with n > 0, an instance in capture mode, repeated instances, a
 * capturing stream.  -2: the engine failed, nothing is marked kept and nothing is written.  n == 0 returns 0. */
int h264bsdmiKeepCurrentPictures(u32 n, storage_t *const *pStorage, void *stream, u32 *kept, u32 *picId);

/* Background model: the kept picture as a RUNNING AVERAGE of the current pictures, with a hold mask — a background that slow and
 * stopped objects do not vanish from after one picture, that movers leave no ghost in, and in which sensor noise is averaged away.  It
 * lives where the kept picture lives, so every consumer (h264bsdmiOutputRegionChange, h264bsdmiOutputRegionShift,
 * h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes in CHANGE mode) reads it as it reads a copied picture.
 * The state of a sample is 16-bit fixed point, S = hi * 256 + lo: hi is the kept picture, lo a second frame that the library allocates
 * at an instance's first blend.  With the current sample c, T = c * 256 + 128 and a shift k,
 *     S' = S + floor((T - S + 2^(k-1)) / 2^k)        k = 1 .. 7;        S' = T        k = 0
 * S' lies between S and T and S stays in [128, 65408]; for constant input hi reaches c and stays there for every k <= 7.
 * A luma sample is MOVING when |c - hi| > hold (strict: hold = 255 means nothing is moving; the test of h264bsdmiOutputRegionChange's
 * `above` with source Y and threshold = hold), a chroma sample when one of the four luma samples it covers is; the test uses the
 * values from before the update.  Still samples take `shift`, moving samples `moving_shift`: 0 copies the current value, 1 .. 7 blends
 * at that rate, H264BSDMI_BLEND_FROZEN leaves S as it is.  Everything is an integer and exact.
 * One launch for the call, the whole coded frame of each of n distinct instances.  kept[i] = 1 when instance i had a current picture,
 * as for h264bsdmiKeepCurrentPictures; blended[i] (may be NULL) = 1 when it was blended into an existing kept picture of the coded
 * size, 0 when the model started with a copy (S = T: what a plain keep leaves); picId (may be NULL): the picId the kept picture now
 * carries, the current picture's.  A plain keep (h264bsdmiKeepCurrentPictures, or any keep_after) stays what it is and resets the
 * fraction: lo reads as 0x80 everywhere until the next blend.
 * spec->moving: NULL, or a DEVICE pointer to u32[n]: word i receives the number of moving luma samples of the whole coded frame of
 * instance i (0 without a current picture, or where the model started); the words are zeroed on the stream ahead of the launch when
 * any instance of the call has a current picture, else untouched.
 * The stream rule, the fence and the ordering of launches that touch kept pictures are those of h264bsdmiKeepCurrentPictures.
 * -1, before anything is enqueued: what h264bsdmiKeepCurrentPictures refuses; spec NULL; shift > 7; hold > 255; a moving_shift that is
 * neither 0 .. 7 nor H264BSDMI_BLEND_FROZEN.  -2: the engine failed, nothing is marked kept and nothing is written.  n == 0 returns 0. */
#define H264BSDMI_BLEND_FROZEN 8u
typedef struct h264bsdmi_blend_spec {
    u32   shift;         /* 0 .. 7: still samples */
    u32   hold;          /* 0 .. 255 */
    u32   moving_shift;  /* 0 .. 7 or H264BSDMI_BLEND_FROZEN: moving samples */
    void *moving;        /* NULL, or DEVICE pointer to u32[n] */
} h264bsdmi_blend_spec;
int h264bsdmiBlendCurrentPictures(u32 n, storage_t *const *pStorage, const h264bsdmi_blend_spec *spec, void *stream,
                                  u32 *kept, u32 *blended, u32 *picId);

/* The kept pictures handed out, for viewing the background: picture[i], a DEVICE buffer of 384 * (macroblocks of the coded frame)
 * bytes, 16-byte aligned, receives the kept picture of instance i as the planar I420 coded frame (Y, Cb, Cr: what
 * h264bsdNextOutputPicture returns for a decoded one).  fraction (may be NULL, and so may fraction[i]): the same for lo, 0x80 where a
 * plain keep came last.  One launch for the call, inside the ordering of launches that touch kept pictures; the stream rule is that
 * of h264bsdmiKeepCurrentPictures.  got[i] = 1, or 0 where the instance has no kept picture of its coded size: its buffers are then
 * untouched.  keptPicId (may be NULL): the picId of the kept picture, or 0.
 * -1, before anything is enqueued: pStorage, picture or got NULL with n > 0; a picture[i] that is NULL or a buffer that is not 16-byte
 * aligned, for an instance that has a kept picture; an instance in capture mode; repeated instances; a capturing stream.  -2: the
 * engine failed, nothing is written by the host.  n == 0 returns 0. */
int h264bsdmiOutputKeptPictures(u32 n, storage_t *const *pStorage, void *const *picture, void *const *fraction, void *stream,
                                u32 *got, u32 *keptPicId);

/* Background spread: a per-sample NOISE LEVEL beside the kept picture.  One `hold` cannot serve a real camera: foliage, water, flicker
 * and noisy dark areas need a high threshold, the quiet wall beside them a low one.  The SPREAD V is a third frame per instance, one
 * byte per sample of the coded frame (luma, Cb, Cr) in the layout of the kept picture, that follows how much the sample usually differs
 * from its background; the moving test then uses it as the sample's threshold.  The library allocates it at an instance's first
 * h264bsdmiBlendCurrentPicturesSpread (instances that never ask pay nothing) and drops it wherever the kept picture is dropped.
 * h264bsdmiBlendCurrentPicturesSpread is h264bsdmiBlendCurrentPictures with one more argument, and everything not said here is that
 * call's.  Per sample, with the current sample c, the kept byte hi and the spread byte V, all read BEFORE the call, and d = |c - hi|:
 *     MOVING    a luma sample when d > max(hold, V); a chroma sample when one of the four luma samples it covers is (chroma V never gates)
 *     S         updated exactly as h264bsdmiBlendCurrentPictures does under that mask (shift, moving_shift, FROZEN)
 *     V         A = min(255, gain d);  V' = clamp(V + sign(A - V), lowest, highest): one step a call; chroma samples with their own d
 * update H264BSDMI_SPREAD_NONE: no byte of V changes; _ALL: the rule applies to every sample; _STILL: only to samples that are not
 * moving (a chroma sample counts as moving by the rule above).  Where an instance's spread is NOT VALID it reads as `lowest`, and where
 * the model starts (no kept picture of the coded size) S = T, V = lowest and nothing is moving.  spec->moving counts the moving luma
 * samples under the new test.  With lowest = highest = 0 the call is h264bsdmiBlendCurrentPictures byte for byte.  Everything is an
 * integer and exact, and independent of scheduling.
 * VALIDITY: the spread becomes valid at a spread blend.  A plain keep (h264bsdmiKeepCurrentPictures and every keep_after) invalidates
 * it without freeing the frame, as it resets the fraction; a plain h264bsdmiBlendCurrentPictures leaves it as it is.
 * h264bsdmiWarpKeptPictures leaves it WHERE IT LIES, unresampled and still valid: after a warp the spread is that of the samples'
 * old positions (registering it with the picture is not part of this interface yet).
 * kept, blended, picId, the stream rule, the fence and the ordering are those of the blend.
 * -1, before anything is enqueued: everything h264bsdmiBlendCurrentPictures refuses; spread NULL; gain outside 1 .. 8; lowest > highest
 * or either above 255; update > 2; an engine without the entry.  -2: the engine failed, nothing is marked.  n == 0 returns 0. */
#define H264BSDMI_SPREAD_NONE  0u
#define H264BSDMI_SPREAD_ALL   1u
#define H264BSDMI_SPREAD_STILL 2u
typedef struct h264bsdmi_spread_spec {
    u32 gain;      /* 1 .. 8 */
    u32 lowest;    /* 0 .. 255 */
    u32 highest;   /* lowest .. 255 */
    u32 update;    /* H264BSDMI_SPREAD_*: 0 none, 1 every sample, 2 still samples only */
} h264bsdmi_spread_spec;
int h264bsdmiBlendCurrentPicturesSpread(u32 n, storage_t *const *pStorage, const h264bsdmi_blend_spec *spec,
                                        const h264bsdmi_spread_spec *spread, void *stream, u32 *kept, u32 *blended, u32 *picId);

/* The spread handed out, for viewing where the scene is busy: spread[i], a DEVICE buffer of 384 * (macroblocks of the coded frame)
 * bytes, 16-byte aligned, receives V of instance i as a planar I420 coded frame, as h264bsdmiOutputKeptPictures hands out the kept
 * picture: one launch, the same ordering and stream rule.  got[i] = 1, or 0 where the instance has no kept picture of its coded size
 * or no valid spread: its buffer is then untouched.  keptPicId (may be NULL): the picId of the kept picture, or 0.
 * -1 and -2 as for h264bsdmiOutputKeptPictures (spread in the place of picture; there is no fraction); an engine without the entry. */
int h264bsdmiOutputKeptSpread(u32 n, storage_t *const *pStorage, void *const *spread, void *stream, u32 *got, u32 *keptPicId);

/* Warped kept pictures: the kept picture of each of n distinct instances RESAMPLED IN PLACE through an affine map, the picture (hi)
 * and, where the instance has one, the fraction (lo) — a background that follows a camera which shakes or pans.  Afterwards the kept
 * picture lies in the coordinates the map leads to, and every consumer (h264bsdmiOutputRegionChange, h264bsdmiOutputRegionShift,
 * h264bsdmiOutputCellMaps / CellBoxes in CHANGE mode, h264bsdmiOutputCellShift, h264bsdmiOutputPointMatches, the blend) reads it
 * unchanged.  maps[i]: six coefficients a b c d e f in 16.16 fixed point, the map from OUTPUT to SOURCE in luma samples of the window
 * (spec->crop as h264bsdmi_tensor_spec.crop: 1 the frame-cropping window, 0 the coded frame).  For the output luma sample (x, y) of a
 * window w x h, in 64-bit integers,
 *     X = a x + b y + c      Y = d x + e y + f                          (units of 2^-16 sample)
 *     outside = X < 0 || X > (w-1) << 16 || Y < 0 || Y > (h-1) << 16;   X, Y clamped to those ranges
 *     x0 = X >> 16, x1 = min(x0 + 1, w - 1), fx = (X >> 8) & 255;       y0, y1, fy likewise
 *     V = (S00 (256 - fx) + S01 fx)(256 - fy) + (S10 (256 - fx) + S11 fx) fy;     S' = (V + 32768) >> 16
 * with S = 256 hi + lo the state of h264bsdmiBlendCurrentPictures (lo reads as 128 where a plain keep came last).  S' is a rounded
 * convex combination of its four neighbours and stays in the blend's [128, 65408].  A chroma sample (cx, cy) sits at luma
 * (2 cx + 1/2, 2 cy + 1/2): in units of 2^-18 chroma sample U = 2 (a 2cx + b 2cy + c) + a + b - 65536, V' the same with d e f, both
 * clamped to the chroma window (w/2, h/2); index U >> 18, weight (U >> 10) & 255, the same blend; whether a chroma sample is outside is
 * decided on its own U, V' before the clamp.  The identity (a = e = 65536, the rest 0) changes no byte; a translation by an even number
 * of whole samples is an index shift on all three planes; a = e = -65536, c = (w-1) << 16, f = (h-1) << 16 is the exact half turn.
 * spec->outside: H264BSDMI_WARP_REPLICATE — the clamp decides; H264BSDMI_WARP_CURRENT — an output sample whose source was outside takes
 * T = 256 c + 128 of the CURRENT picture's sample at the output position, what a starting blend writes; an instance without a current
 * picture is then left alone.  Samples of the coded frame outside the window keep their state.  hi is always written, lo only where
 * the instance's lo is valid (after a plain keep none is allocated and it keeps reading as 0x80).  The kept picId does not change.
 * warped[i] = 1 when instance i's kept picture was resampled, 0 when it was left alone (no kept picture of its coded size, or none
 * current under CURRENT); keptPicId (may be NULL): the picId of the kept picture, or 0.
 * spec->count: NULL, or a DEVICE pointer to u32[n]: word i receives the number of luma samples of instance i's window whose source was
 * outside (0 where it was left alone); the words are zeroed on the stream ahead of the launch when any instance is warped.
 * Repeated bilinear resampling softens the picture: the 16-bit state delays the loss and does not remove it; whole-sample translations
 * are exact.  One launch for the call.  The stream rule and the ordering of launches that touch kept pictures are those of
 * h264bsdmiKeepCurrentPictures; under CURRENT the fence of a pull of current pictures applies.
 * -1, before anything is enqueued: what h264bsdmiKeepCurrentPictures refuses (warped NULL in place of kept); spec or spec->maps NULL;
 * outside > 1; crop > 1; |a|, |b|, |d| or |e| above 16 * 65536 (c, f: any int32).  -2: the engine failed, nothing is written by the
 * host.  n == 0 returns 0. */
#define H264BSDMI_WARP_REPLICATE 0u
#define H264BSDMI_WARP_CURRENT   1u
#define H264BSDMI_WARP_MAX_COEFFICIENT (16 * 65536)
typedef struct h264bsdmi_warp_map { int a, b, c, d, e, f; } h264bsdmi_warp_map;      /* 32-bit, 16.16 fixed point */
typedef struct h264bsdmi_warp_spec {
    const h264bsdmi_warp_map *maps;  /* HOST, n */
    u32   outside;       /* H264BSDMI_WARP_* */
    u32   crop;          /* 0, 1 */
    void *count;         /* NULL, or DEVICE pointer to u32[n] */
} h264bsdmi_warp_spec;
int h264bsdmiWarpKeptPictures(u32 n, storage_t *const *pStorage, const h264bsdmi_warp_spec *spec, void *stream,
                              u32 *warped, u32 *keptPicId);

/* Change statistics: integer statistics of (current picture - kept picture) over boxes, computed where the two pictures lie, with one
 * launch — did anything change since the last picture or since the background I stored, is the feed frozen, is this a cut or only a
 * brightness shift, what is the PSNR against the picture I kept — without pulling a pixel.  A sibling of h264bsdmiOutputRegionStats:
 * the same region struct and limits, the same source window (spec->crop), regions == NULL with nRegions == n meaning whole windows,
 * the same sources — the channels exactly as region statistics defines them; RGB is the reference conversion of each picture, then
 * the difference —, the same stream rule and fence, nRegions <= 65535.  It pops nothing and may be repeated.
 * Record r is written at spec->data + r * stride, stride = 8 + 32 C + 4 C B bytes, little endian; d = current - kept per channel at
 * every luma position of box ∩ window:
 *     u32 count; u32 zero;
 *     C x { u64 sad; u64 ssd; i64 sum; u32 max; u32 above; }     sum of |d|, of d * d, of d (signed); max |d|; #(|d| > threshold[c])
 *     C x B x u32 hist                                           of |d|: hist[c][|d| >> (8 - log2 B)]; every hist[c] sums to count
 * count == 0 (the box misses the window): all zeros.  Everything is an integer and exact.  The call writes the WHOLE record with plain
 * stores: the caller does not clear it.  got[r] = 1 only when the region's instance has a current picture AND a kept one; otherwise 0,
 * and record r is untouched.  current, kept, picId, keptPicId: per instance, each may be NULL; kept / keptPicId report what the
 * comparison saw.
 * keep_after = 1: behind the comparison, on the same stream, the current picture of every instance of the call that has one becomes
 * its kept picture (one more launch), whether or not it had a kept picture before: a per-tick loop starts itself, call t gives the
 * difference to the picture of call t - 1.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputRegionStats refuses in regions, instances, stream,
 * data and bins; source > 2; crop > 1; a threshold above 255; keep_after > 1.  -2: the engine failed: nothing is written by the
 * host and nothing is marked kept. */
typedef struct h264bsdmi_change_spec {
    void *data;          /* DEVICE pointer, caller-owned, 8-byte aligned: record r at data + r * stride */
    u32   source;        /* H264BSDMI_STATS_* */
    u32   bins;          /* 0 (no histogram), 16, 32, 64, 128 or 256: bin = |d| >> (8 - log2 bins) */
    u32   crop;          /* as h264bsdmi_tensor_spec.crop */
    u32   threshold[3];  /* per channel, 0..255 (STATS_Y: [0] only) */
    u32   keep_after;    /* 0 / 1 */
} h264bsdmi_change_spec;
int h264bsdmiOutputRegionChange(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                                const h264bsdmi_change_spec *spec, void *stream,
                                u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId);

/* Cell maps: WHERE did the picture change, where is it dark, flat or blown out — dense maps with one value per small square cell of a
 * box, computed where the pictures lie with one launch, small enough to threshold in torch and turn into the boxes of the calls above.
 * A sibling of h264bsdmiOutputRegionStats (mode PICTURE) and h264bsdmiOutputRegionChange (mode CHANGE): the same region struct and
 * limits, negative origins, boxes that leave the window or miss it, regions == NULL with nRegions == n meaning whole windows, the same
 * source window (spec->crop), the same channels, the current-picture rule, in CHANGE mode the kept-picture rule, got, current, kept,
 * picId and keptPicId (each may be NULL), the stream rule, the fence and keep_after.
 * Every region gets a grid of rows x cols cells of cell x cell luma samples laid over its box from the box's origin: cell (i, j),
 * 0 <= i < rows, 0 <= j < cols, covers the box-relative positions u in [j cell, (j + 1) cell), v in [i cell, (i + 1) cell), intersected
 * with the box [0, w) x [0, h) and with the window.  THE DEFINITION: cell (i, j) of region (x, y, w, h) holds what the record, at
 * bins = 0, of h264bsdmiOutputRegionStats (PICTURE) or h264bsdmiOutputRegionChange (CHANGE) holds for the box
 * (x + j cell, y + i cell, min(cell, w - j cell), min(cell, h - i cell)).  Cells of the box beyond the grid are not reported; cells of
 * the grid beyond the box or outside the window have count 0, and with count 0 PICTURE gives sum 0, sumsq 0, min 255, max 0 and CHANGE
 * all zeros.
 * Slice r is written at (u32 *)spec->data + r * P * rows * cols: P maps of rows x cols u32 each, row-major, in this order: COUNT if
 * asked, then per set bit of spec->planes in ascending order C maps, in the channel order of the source.  The call writes the WHOLE
 * slice with plain stores: the caller does not clear it.  Everything is exact: the largest value is 64 * 64 * 255^2 < 2^31, which
 * is why cell stops at 64 and why u32 (int32 in torch) suffices; DSUM is an i32 in two's complement.  got[r] = 0 (no current picture;
 * CHANGE: or no kept one): slice r is untouched.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputRegionStats refuses in regions, instances and stream;
 * spec or data NULL or data not 4-byte aligned; cols or rows 0 or above 4096; a cell not in {4, 8, 16, 32, 64}; source > 2; crop > 1;
 * mode > 1; planes 0 or with bits outside the mode's set; a threshold above 255; PICTURE with a non-zero threshold or keep_after;
 * keep_after > 1.  -2: the engine failed (also: more than 2^23 workgroups — 128 x 64 luma samples of grid each, times the regions —
 * in one call): nothing is written by the host and nothing is marked kept.  nRegions == 0 returns 0 and launches nothing.
 * MODE SPREAD (2) reads the current picture, the kept picture and the spread of h264bsdmiBlendCurrentPicturesSpread: per sample and
 * channel t = max(threshold[c], V) — threshold is the floor — and d = |current - kept|; the planes are COUNT, FORE = #(d > t),
 * EXCESS = sum of max(0, d - t) and SPREADSUM = sum of V (the map of where the scene is busy), C maps each, sources Y and YCbCr (the
 * chroma bytes of V lie under the luma positions as the chroma samples do); the largest value is 64 * 64 * 255.  got[r] = 0 and slice
 * r untouched where the instance lacks a current picture, a kept picture or a valid spread.  Refused with -1 beyond the above: source
 * RGB; plane bits outside 1 | 2 | 4 | 8; keep_after = 1 (a plain keep would invalidate what the call just read); an engine without
 * the spread entries.  h264bsdmiOutputCellBoxes takes any one plane of the mode: all are unsigned. */
#define H264BSDMI_CELLS_PICTURE 0      /* statistics of the current picture            */
#define H264BSDMI_CELLS_CHANGE  1      /* of d = current - kept, as region change      */
#define H264BSDMI_CELL_COUNT  1u       /* 1 map, both modes                            */
/* PICTURE, C maps each: */
#define H264BSDMI_CELL_SUM    2u
#define H264BSDMI_CELL_SUMSQ  4u
#define H264BSDMI_CELL_MIN    8u
#define H264BSDMI_CELL_MAX    16u
/* CHANGE, C maps each: */
#define H264BSDMI_CELL_SAD    2u       /* sum |d|  */
#define H264BSDMI_CELL_SSD    4u       /* sum d*d  */
#define H264BSDMI_CELL_DSUM   8u       /* sum d, i32 two's complement */
#define H264BSDMI_CELL_DMAX   16u      /* max |d|  */
#define H264BSDMI_CELL_ABOVE  32u      /* #(|d| > threshold[c]) */
/* SPREAD, C maps each: */
#define H264BSDMI_CELLS_SPREAD  2      /* of |current - kept| against t = max(threshold[c], V) */
#define H264BSDMI_CELL_FORE      2u    /* #(|d| > t) */
#define H264BSDMI_CELL_EXCESS    4u    /* sum max(0, |d| - t) */
#define H264BSDMI_CELL_SPREADSUM 8u    /* sum V */
typedef struct h264bsdmi_cells_spec {
    void *data;            /* DEVICE, caller-owned, 4-byte aligned: slice r at data + r * P*rows*cols u32 */
    u32 cols, rows;        /* grid of every slice, 1..4096 each */
    u32 cell;              /* 4, 8, 16, 32 or 64 luma samples a side */
    u32 source, crop;      /* H264BSDMI_STATS_*; as everywhere */
    u32 mode, planes;      /* planes: non-empty subset of the mode's bits */
    u32 threshold[3];      /* CHANGE, SPREAD: 0..255 per channel; PICTURE: must be 0 */
    u32 keep_after;        /* CHANGE: 0 / 1 as h264bsdmiOutputRegionChange; PICTURE, SPREAD: must be 0 */
} h264bsdmi_cells_spec;
int h264bsdmiOutputCellMaps(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                            const h264bsdmi_cells_spec *spec, void *stream,
                            u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId);

/* Cell boxes: the step from a cell map to the boxes of the calls above — threshold, connected regions, bounding boxes — made where the
 * map lies, so that a few hundred bytes per region cross to the host instead of the map.
 * THE MAPS: the call does everything h264bsdmiOutputCellMaps(..., cells, ...) does, with the same result in cells->data, byte for byte,
 * keep_after and all the output arrays included.  Behind that launch, on the same stream, it fills the boxes slices.
 * FOREGROUND: cell (i, j) of region r is foreground iff box ∩ window reaches it (its count is above 0: decided from the geometry,
 * whether or not COUNT was asked for) and its value in map `plane`, channel `channel`, passes the level: value > level (ABOVE) or
 * value < level (BELOW), both as u32.  Cells the box or the window do not reach are never foreground, under BELOW too, where their sum
 * of 0 would pass.
 * COMPONENTS: a component is a maximal set of foreground cells connected through 4 (left, right, up, down) or 8 (the diagonals too)
 * neighbours within the slice's grid.  Components of fewer than min_cells cells are dropped.  NUMBERING: the rest are numbered by the
 * raster index (i * cols + j) of their first cell in raster order, ascending.
 * SLICE LAYOUT: slice r, at (u32 *)boxes->data + r * (1 + M) * 8 with M = max_boxes, is (1 + M) records of 8 u32, and the call writes
 * the WHOLE slice with plain stores: the caller does not clear it.
 *     record 0           found, written, foreground_cells, dropped, 0, 0, 0, 0
 *                        found: the components that remain; written = min(found, M); dropped: the components removed by min_cells
 *     records 1..written x, y, w, h, cells, peak, sum_lo, sum_hi        the first `written` components in that order
 *     the records beyond all zero
 * x, y, w, h: the bounding rectangle of the component's cells, (x_r + jmin cell, y_r + imin cell) to (x_r + (jmax + 1) cell,
 * y_r + (imax + 1) cell), intersected with the box and with the window, in the coordinates regions use: { instance, x, y, w, h } is a
 * valid h264bsdmi_region of the same instance, w, h >= 1.  cells: the number of cells; peak: the largest value under ABOVE, the smallest
 * under BELOW; sum: the 64-bit sum of the values (16384 cells x 64 * 64 * 255^2 passes 2^32: two words, low first).  Everything is an
 * integer and exact, and no result depends on scheduling.  got[r] = 0: neither slice r of the maps nor slice r of the boxes is touched.
 * THE CAP: rows * cols of the grid is at most H264BSDMI_BOXES_MAX_CELLS, so that the labels and the per-component counters of a slice
 * live in one workgroup's LDS as plain 32-bit words: 1080p fits at cell 16 (68 x 120 = 8160), 32 and 64; 1080p at cell 8 and 4K at
 * cell 16 do not and are refused.  Larger grids are not part of this interface yet.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputCellMaps refuses; boxes or boxes->data NULL or data not
 * 4-byte aligned; max_boxes 0 or above 512; plane not exactly one bit of cells->planes, or DSUM in CHANGE mode (signed); channel not
 * below the channels of cells->source (COUNT: not 0); sense > 1; connectivity not 4 or 8; min_cells 0; cells->rows * cells->cols above
 * 16384.  -2: the engine failed, as for the siblings: nothing is written by the host and nothing is marked kept.  nRegions == 0 returns
 * 0 and launches nothing. */
#define H264BSDMI_BOXES_MAX_CELLS 16384u   /* rows * cols of a slice that can be labelled */
#define H264BSDMI_BOXES_MAX_BOXES 512u
#define H264BSDMI_BOXES_ABOVE 0u           /* foreground: value >  level */
#define H264BSDMI_BOXES_BELOW 1u           /* foreground: value <  level */
typedef struct h264bsdmi_boxes_spec {
    void *data;          /* DEVICE, caller-owned, 4-byte aligned: slice r at (u32 *)data + r * (1 + max_boxes) * 8 */
    u32 max_boxes;       /* M, 1..512 */
    u32 plane;           /* ONE H264BSDMI_CELL_* bit, contained in cells->planes; not DSUM (signed) */
    u32 channel;         /* 0 .. C-1 of cells->source (COUNT: 0) */
    u32 sense, level;    /* ABOVE / BELOW; unsigned comparison with the u32 of the cell */
    u32 connectivity;    /* 4 or 8 */
    u32 min_cells;       /* >= 1: components of fewer cells are dropped before numbering */
} h264bsdmi_boxes_spec;
int h264bsdmiOutputCellBoxes(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                             const h264bsdmi_cells_spec *cells, const h264bsdmi_boxes_spec *boxes, void *stream,
                             u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId);

/* Region shift: WHERE did a box go — a block-matching search of boxes of the instances' KEPT pictures in their CURRENT pictures, luma
 * only, computed where the two pictures lie, with one launch: boxes that follow the content between two runs of a detector, a camera that
 * was knocked or shakes (the whole window moved by (dx, dy), which h264bsdmiOutputRegionChange cannot tell from a scene change), crops
 * stabilised before h264bsdmiOutputTensorRegions — without pulling a pixel.  A sibling of h264bsdmiOutputRegionChange, and everything not
 * said here is that call's, word for word: the region struct and its limits, negative origins, boxes that leave the source window or miss
 * it, regions == NULL with nRegions == n meaning whole windows, the source window (spec->crop: W x H, coordinates relative to it), the
 * current-picture and the kept-picture rule, got (per REGION), current, kept, picId, keptPicId (per instance, each may be NULL), the stream
 * rule, the fence, the ordering of launches that touch kept pictures, keep_after, nRegions <= 65535.  It pops nothing and may be repeated.
 * THE QUANTITY: the region's box lies in the KEPT picture and is the template, T = box ∩ window; it is searched in the CURRENT picture.
 * For every displacement (dx, dy), |dx|, |dy| <= R = spec->radius, D = 2 R + 1:
 *     SAD(dx, dy) = sum over (u, v) in T of | kept(u, v) - current(clamp(u + dx, 0, W - 1), clamp(v + dy, 0, H - 1)) |
 * DIRECTION: (dx, dy) is where the content of the box lies in the current picture relative to where it lay in the kept one: content that
 * moved 3 samples right and 2 up answers (3, -2), and the box to use from now on is (x + dx, y + dy, w, h).
 * BORDER: the current picture is replicated at the border of the WINDOW, not of the coded frame, so every displacement sums over the same
 * count = |T| samples and the SADs are comparable.
 * TIES: the answer is the displacement of the smallest SAD; among equal SADs the smallest dx^2 + dy^2, then the smallest dy, then the
 * smallest dx: a flat or unchanged box answers (0, 0).
 * Record r is written at spec->data + r * stride, little endian; stride = 32 without the surface, 32 + 4 (D D + 1) with it (the last u32
 * is a zero pad that keeps records 8-byte aligned):
 *     u32 count; u32 D; i32 dx; i32 dy; u32 best; u32 still; u32 ties; u32 zero;
 *     [ D x D x u32 sad;   sad[(dy + R) * D + (dx + R)];   u32 zero ]
 * best = SAD(dx, dy); still = SAD(0, 0), which is h264bsdmiOutputRegionChange's luma sad of the same box; ties = the number of
 * displacements whose SAD equals best (1: a unique minimum).  count == 0 (the box misses the window): dx = dy = best = still = 0, ties =
 * D D, the surface all zero — the formula applied to nothing.  w, h <= H264BSDMI_SHIFT_MAX_SIDE keeps count <= 2^24, so every SAD fits 32
 * bits (4096^2 * 255 < 2^32).  Everything is an integer and exact.  The call writes the WHOLE record with plain stores: the caller does
 * not clear it.  got[r] = 0 (no current picture, or no kept one): record r is untouched.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputRegionChange refuses in regions, instances, stream and data;
 * radius > 16; surface > 1; crop > 1; keep_after > 1; a region with w or h above 4096.  -2: the engine failed: nothing is written by the
 * host and nothing is marked kept.  nRegions == 0 returns 0 and launches nothing. */
#define H264BSDMI_SHIFT_MAX_RADIUS 16
#define H264BSDMI_SHIFT_MAX_SIDE   4096     /* w, h of a region: count <= 2^24, so every SAD fits 32 bits (4096^2 * 255 < 2^32) */
typedef struct h264bsdmi_shift_spec {
    void *data;        /* DEVICE pointer, caller-owned, 8-byte aligned: record r at data + r * stride */
    u32   radius;      /* R, 0 .. 16; D = 2R + 1 */
    u32   surface;     /* 0 / 1: the D x D SADs behind the header */
    u32   crop;        /* as h264bsdmi_tensor_spec.crop */
    u32   keep_after;  /* 0 / 1, as h264bsdmi_change_spec.keep_after */
} h264bsdmi_shift_spec;
int h264bsdmiOutputRegionShift(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                               const h264bsdmi_shift_spec *spec, void *stream,
                               u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId);

/* Cell shift: WHERE did every cell go — the dense sibling of h264bsdmiOutputRegionShift, as h264bsdmiOutputCellMaps is the dense sibling
 * of h264bsdmiOutputRegionChange: one block-matching search per cell of a grid, all in one launch, the answers as maps with one integer
 * per cell: motion segmentation against the kept picture (a frame from a second ago, or the background model of
 * h264bsdmiBlendCurrentPictures), a camera shift as the mode of the map, objects as the cells that leave it, and per cell the gain
 * still - best that tells motion from noise.  Nothing is pulled.
 * A sibling of h264bsdmiOutputCellMaps in CHANGE mode, and everything about regions, grids and instances is that call's, word for word:
 * the region struct and its limits, negative origins, boxes that leave the window or miss it, regions == NULL with nRegions == n
 * meaning whole windows, the source window (spec->crop), the grid of rows x cols cells of cell x cell luma samples laid over the box
 * from its origin, the current-picture and the kept-picture rule (got[r] = 0 when either is missing: slice r is untouched), got,
 * current, kept, picId, keptPicId (each may be NULL), the stream rule, the fence, the ordering of launches that touch kept pictures,
 * keep_after, nRegions <= 65535.  A sibling of h264bsdmiOutputRegionShift for the arithmetic.
 * THE DEFINITION: cell (i, j) of region (x, y, w, h) holds the fields count, dx, dy, best, still, ties of the record that
 * h264bsdmiOutputRegionShift, at the same radius and crop, writes for the box
 * (x + j cell, y + i cell, min(cell, w - j cell), min(cell, h - i cell)): the template is that box ∩ window in the KEPT picture; the
 * CURRENT picture is clamped at the WINDOW, not at the cell or the box, so a cell searches into its neighbours' samples; the same tie
 * rule (smallest SAD, then smallest dx^2 + dy^2, then smallest dy, then smallest dx).  Cells of the grid beyond the box or outside the
 * window are the formula applied to nothing: count 0, dx = dy = best = still = 0, ties = D D, D = 2 radius + 1.  Cells of the box beyond
 * the grid are not reported.
 * Slice r is written at (u32 *)spec->data + r * P * rows * cols: P maps of rows x cols u32 each, row-major, one per set bit of
 * spec->planes in ascending order (dx and dy are i32 in two's complement).  The call writes the WHOLE slice with plain stores: the
 * caller does not clear it.  Everything is an integer and exact, and no result depends on scheduling.  A cell's SAD is at most
 * 64 * 64 * 255 < 2^20, so u32 (int32 in torch) suffices, and regions need no H264BSDMI_SHIFT_MAX_SIDE cap: no sum spans more than a
 * cell.  Cell 4 is left out on purpose: sixteen samples are no template, and D D displacements per 16 samples is the worst ratio of
 * argmin to search.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputCellMaps refuses in regions, instances and stream; spec
 * or data NULL or data not 4-byte aligned; cols or rows 0 or above 4096; a cell not in {8, 16, 32, 64}; radius > 16; planes 0 or with
 * bits outside the set; crop > 1; keep_after > 1.  -2: the engine failed (also: more than 2^23 workgroups — 64 x 64 luma samples of grid
 * each, times the regions — in one call): nothing is written by the host and nothing is marked kept.  nRegions == 0 returns 0 and
 * launches nothing. */
#define H264BSDMI_FLOW_COUNT 1u
#define H264BSDMI_FLOW_DX    2u    /* i32 */
#define H264BSDMI_FLOW_DY    4u    /* i32 */
#define H264BSDMI_FLOW_BEST  8u
#define H264BSDMI_FLOW_STILL 16u
#define H264BSDMI_FLOW_TIES  32u
typedef struct h264bsdmi_cell_shift_spec {
    void *data;        /* DEVICE, caller-owned, 4-byte aligned: slice r at (u32 *)data + r * P * rows * cols */
    u32 cols, rows;    /* 1..4096 each */
    u32 cell;          /* 8, 16, 32 or 64 */
    u32 radius;        /* 0..16 */
    u32 planes;        /* non-empty subset of the bits above; P = their number */
    u32 crop, keep_after;
} h264bsdmi_cell_shift_spec;
int h264bsdmiOutputCellShift(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                             const h264bsdmi_cell_shift_spec *spec, void *stream,
                             u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId);

/* Corner points: WHICH boxes are worth following — Shi-Tomasi (minimum eigenvalue) or Harris corner points of boxes of the instances'
 * CURRENT pictures, luma only, computed where the pictures lie with one launch: gradients, the structure tensor, a corner score,
 * non-maximum suppression, the strongest K — the good-features-to-track step ahead of h264bsdmiOutputRegionShift, whose search means
 * something on textured templates only — and a focus measure (the gradient energy) from the same pass.  A sibling of
 * h264bsdmiOutputRegionStats, and everything not said here is that call's, word for word: the region struct and its limits, negative
 * origins, boxes that leave the source window or miss it, regions == NULL with nRegions == n meaning whole windows, the source window
 * (spec->crop: W x H, coordinates relative to it), the current-picture rule, got (per REGION), current, picId (per instance, each may be
 * NULL), the stream rule, the fence, nRegions <= 65535.  It needs no kept picture, pops nothing and may be repeated.
 * THE QUANTITY, all integers, T = box ∩ window:
 *     replicated luma   L~(u, v) = L(clamp(u, 0, W - 1), clamp(v, 0, H - 1)): the clamp is at the WINDOW, as for the region shift, and
 *                       it is the only border rule
 *     gradients         at any (u, v): gx = [L~(u+1, v-1) + 2 L~(u+1, v) + L~(u+1, v+1)] - [the same at u-1], gy the same transposed
 *                       (Sobel); |g| <= 1020
 *     structure tensor  b = spec->block, 3 or 5: A = sum gx gx, B = sum gy gy, C = sum gx gy over the b x b samples centred on (u, v),
 *                       taken from the replicated picture as well; A, B, |C| <= 25 * 1020^2 < 2^25
 *     score S(u, v)     for (u, v) in the window.  MIN_EIGEN: A + B - isqrt((A - B)^2 + 4 C^2), isqrt the exact floor square root:
 *                       about twice the smaller eigenvalue, 0 <= S < 2^26.  HARRIS: 16 (A B - C^2) - (A + B)^2, k = 1 / 16, signed,
 *                       |S| < 2^54
 *     candidates        a window sample p with S(p) > min_score (strictly) that no OTHER window sample q within Chebyshev distance
 *                       spec->nms beats: q beats p when S(q) > S(p), or S(q) == S(p) and q comes earlier in raster order (smaller y,
 *                       then smaller x).  Samples outside the window do not compete.  Candidacy does not depend on the box:
 *                       candidates(box) = candidates(whole window) ∩ box
 *     points            the candidates inside T, sorted by (score descending, y ascending, x ascending); the first K = max_points
 *     energy            the sum over T of gx^2 + gy^2 (the Tenengrad focus measure), at most 2^28 * 2^21
 * Record r is written at spec->data + r * stride, little endian, stride = 32 + 16 K:
 *     u32 count; u32 found; u32 written; u32 zero; u64 energy; u64 zero;
 *     K x { i32 x; i32 y; i64 score; }       x, y in the regions' own coordinates (the source window's); slots >= written all zero
 * count = |T|, found = the candidates in T, written = min(found, K).  count == 0 (the box misses the window): everything zero.
 * Everything is an integer and exact, and no result depends on scheduling.  The call writes the WHOLE record with plain stores: the
 * caller does not clear it.  got[r] = 0 (no current picture): record r is untouched.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputRegionStats refuses in regions, instances and stream;
 * spec or data NULL or data not 8-byte aligned; score > 1; block not 3 or 5; nms outside 1 .. 7; max_points outside 1 .. 256; crop > 1;
 * zero != 0; HARRIS with min_score >= 2^63.  -2: the engine failed: nothing is written by the host.  nRegions == 0 returns 0 and
 * launches nothing. */
#define H264BSDMI_CORNERS_MIN_EIGEN  0u
#define H264BSDMI_CORNERS_HARRIS     1u
#define H264BSDMI_CORNERS_MAX_NMS    7u
#define H264BSDMI_CORNERS_MAX_POINTS 256u
typedef struct h264bsdmi_corners_spec {
    void *data;        /* DEVICE pointer, caller-owned, 8-byte aligned: record r at data + r * (32 + 16 * max_points) */
    u32   score;       /* H264BSDMI_CORNERS_* */
    u32   block;       /* b: 3 or 5 */
    u32   nms;         /* 1 .. 7, Chebyshev distance */
    u32   max_points;  /* K, 1 .. 256 */
    u32   crop;        /* as h264bsdmi_tensor_spec.crop */
    u32   zero;        /* must be 0 */
    unsigned long long min_score;   /* a candidate has S > min_score */
} h264bsdmi_corners_spec;
int h264bsdmiOutputCornerPoints(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                                const h264bsdmi_corners_spec *spec, void *stream,
                                u32 *got, u32 *current, u32 *picId);

/* Point matches: WHERE did the points go, at any distance — a 256-bit binary descriptor of every corner point of the KEPT and of the
 * CURRENT picture and the Hamming matching of the two sets, computed where the pictures lie: what h264bsdmiOutputRegionShift cannot
 * answer beyond its radius of 16 (a camera that pans or was knocked, an object that crosses the picture between two detector runs, a
 * point that reappears, a scene reference from a minute ago), because distance in the picture does not enter.  The inputs are the records
 * of two h264bsdmiOutputCornerPoints calls at the same max_points and the two pictures.  Nothing is pulled.
 * A sibling of h264bsdmiOutputRegionShift, and everything about the following is that call's, word for word: the region struct and its
 * limits, regions == NULL with nRegions == n meaning whole windows, the source window (spec->crop), the current-and-kept-picture rule
 * (got[r] = 0 when either is missing: record r is untouched), got, current, kept, picId, keptPicId (each may be NULL), the stream rule,
 * the fence, the ordering of launches that touch kept pictures, keep_after, nRegions <= 65535.
 * THE DEFINITION, all integers, T = box ∩ window, L~ the luma replicated at the WINDOW (h264bsdmiOutputCornerPoints' clamp, the only
 * border rule):
 *     pattern           256 tests (px, py, qx, qy), every coordinate in -12 .. 12, from this generator, fixed forever: xorshift32 with
 *                       state s = 0x9E3779B9; one draw is s ^= s << 13; s ^= s >> 17; s ^= s << 5 (mod 2^32) and gives s; one
 *                       coordinate is ((draw >> 8) % 13 - 6) + ((draw >> 8) % 13 - 6), from two draws; one test is four coordinates in
 *                       the order px, py, qx, qy; a test with p == q, or one equal to an earlier test or its swap, is dropped and drawn
 *                       again (none occurs in the first 256).  The first three tests are (-6, 5, 4, -1), (0, -10, -10, -4) and
 *                       (-7, -10, -6, 1), the last is (-2, -2, -4, -11), the sum of all 1024 numbers is 86 and of their absolute values
 *                       4464.  h264bsdmiDescriptorPattern() gives the 1024 numbers, test after test; it is host-only, needs no device.
 *     smoothed sample   B(u, v) = the sum of L~ over the 5 x 5 samples centred on (u, v), 0 .. 6375: a descriptor reads L~ within 14
 *                       samples of its point, a 29 x 29 patch
 *     descriptor        of a point (x, y): bit t is 1 iff B(x + px_t, y + py_t) < B(x + qx_t, y + qy_t); bit t is bit t % 32 of
 *                       little-endian dword t / 32: 32 bytes.  Upright, no orientation: fixed cameras are the use
 *     valid slots       slot i of a point record is valid iff i < min(written, K) and (x, y) in T, `written` the u32 at byte 8 of the
 *                       record, read as it is and clamped.  The records are caller memory: garbage in them leads to no access outside
 *                       the picture or the record.  Kept slots are described on the KEPT picture, current slots on the CURRENT one;
 *                       the descriptor of an invalid slot is 32 zero bytes
 *     candidates        of kept slot i: the valid current slots j, with max_move > 0 those with max(|xk - xc|, |yk - yc|) <= max_move;
 *                       d(i, j) = popcount(Dk[i] xor Dc[j]), 0 .. 256
 *     best match        of i: the candidate j of smallest d, then smallest j; best = that d; second = the smallest d among the OTHER
 *                       candidates, 257 if there is none; with no candidates j = -1 and best = second = 257
 *     mutual            i is mutual iff, among the valid kept slots that have best(i) as a candidate, i has the smallest d to it,
 *                       then the smallest i
 *     accepted          i is valid and has a candidate, best <= max_distance, ratio == 256 or best * 256 < ratio * second, and
 *                       !mutual_only or i is mutual
 * Record r is written at spec->data + r * stride, little endian, stride = 32 + 80 K:
 *     u32 kept_valid; u32 current_valid; u32 accepted; u32 mutual; i32 sum_dx; i32 sum_dy; u32 zero[2];
 *     K x { i32 j; u32 best; u32 second; u32 flags; }      flags: H264BSDMI_MATCH_*; an invalid kept slot holds -1, 257, 257, 0
 *     K x 32 bytes of kept descriptors; K x 32 bytes of current descriptors
 * Slot indices are those of the point records, not compacted.  kept_valid, current_valid, accepted and mutual count the slots of each
 * kind; sum_dx, sum_dy are the sums of xc - xk, yc - yk over the accepted slots: the mean displacement, a camera shift, without a host
 * loop.  Everything is an integer and exact, and no result depends on scheduling.  The call writes the WHOLE record with plain stores:
 * the caller does not clear it.  data must not overlap the point records (undefined, not checked); kept_points == current_points is
 * allowed.
 * -1, before anything is enqueued, nothing written: everything h264bsdmiOutputRegionShift refuses in regions, instances and stream;
 * spec NULL; data, kept_points or current_points NULL or not 8-byte aligned; max_points outside 1 .. 256; max_distance > 256; ratio
 * outside 1 .. 256; max_move > 65535; mutual_only, crop or keep_after > 1; zero != 0; a sink without the entry or one that cannot keep
 * pictures.  -2: the engine failed: nothing is written by the host and nothing is marked kept.  nRegions == 0 returns 0 and launches
 * nothing. */
#define H264BSDMI_MATCH_VALID    1u
#define H264BSDMI_MATCH_MUTUAL   2u
#define H264BSDMI_MATCH_ACCEPTED 4u
#define H264BSDMI_MATCHES_MAX_POINTS 256u
typedef struct h264bsdmi_matches_spec {
    void       *data;            /* DEVICE, caller-owned, 8-byte aligned: record r at data + r * (32 + 80 K) */
    const void *kept_points;     /* DEVICE, 8-byte aligned: records of h264bsdmiOutputCornerPoints at max_points == K, */
    const void *current_points;  /*   record r at + r * (32 + 16 K); r's points belong to region r's picture (kept / current) */
    u32 max_points;              /* K, 1 .. 256 */
    u32 max_distance;            /* 0 .. 256 */
    u32 ratio;                   /* 1 .. 256, in 256ths; 256: no ratio test */
    u32 max_move;                /* 0: no gate; else 1 .. 65535, Chebyshev */
    u32 mutual_only;             /* 0 / 1 */
    u32 crop, keep_after, zero;  /* zero must be 0 */
} h264bsdmi_matches_spec;
int h264bsdmiOutputPointMatches(u32 n, storage_t *const *pStorage, u32 nRegions, const h264bsdmi_region *regions,
                                const h264bsdmi_matches_spec *spec, void *stream,
                                u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId);
const signed char *h264bsdmiDescriptorPattern(void);

/* Point model: WHICH motion do the matches agree on — an exhaustive, deterministic, all-integer consensus fit of a translation or of a
 * similarity (rotation + uniform scale + translation) to the accepted matches of every region, computed where the records lie: the step
 * behind h264bsdmiOutputPointMatches, whose sum_dx, sum_dy is a translation only and is pulled by every mismatch and every object that
 * moves.  Not random-sample consensus: EVERY hypothesis is tried, which K <= 256 allows.  The output is the inlier set, the two slots that
 * span the best hypothesis and the exact integer moment sums of the inliers, from which a least-squares translation, similarity or affine
 * transform kept -> current follows on the host in closed form; the inlier and outlier flags separate "the camera" from "what moved in
 * front of it".
 * The call needs NO PICTURE: the instances only name the device.  n >= 1 instances, each non-NULL and distinct, each on a sink of this
 * engine that has the entry, all on one device; no instance needs a current or a kept picture or to have been fed anything; nothing is
 * popped or marked.  There are no `got` arrays: every record r < nRecords is written WHOLE with plain stores, the caller does not clear
 * it.  nRecords == 0 returns 0 and launches nothing; nRecords <= 65535.  The stream rule is the siblings': with a stream the call is
 * enqueued there and returns; with NULL it runs on the engine's stream and returns after completion, the device's error words folded; a
 * capturing stream is refused.
 * The three inputs are caller memory, read as they are: record r of `matches` at + r * (32 + 80 K) (h264bsdmiOutputPointMatches at K), of
 * kept_points and current_points at + r * (32 + 16 K) (h264bsdmiOutputCornerPoints at K).  Garbage in them leads to no access outside
 * the three records of that r and to no arithmetic overflow.  data must not overlap the inputs (undefined, not checked).
 * THE DEFINITION, all integers:
 *     pair of slot i    slot i (0 <= i < K) gives a USABLE PAIR iff the matches slot's flags have H264BSDMI_MATCH_ACCEPTED, its j
 *                       satisfies 0 <= j < K, i < min(kept `written`, K) and j < min(current `written`, K), and all four coordinates
 *                       p = (xk, yk) (kept slot i) and q = (xc, yc) (current slot j) lie in 0 .. 16383.  That bound makes every
 *                       quantity below fit 64 bits: differences are < 2^14, components of complex products of differences < 2^30,
 *                       their squared norm < 2^61
 *     TRANSLATION       a hypothesis is one usable slot a, with t = q_a - p_a; slot i is an inlier iff |q_i - p_i - t|^2 <= tolerance^2
 *     SIMILARITY        a hypothesis is a pair of usable slots a < b with p_a != p_b and q_a != q_b; with max_scale = S > 0 the pair
 *                       must also satisfy 65536 |q_b - q_a|^2 <= S^2 |p_b - p_a|^2 and 65536 |p_b - p_a|^2 <= S^2 |q_b - q_a|^2.
 *                       Points are read as complex numbers x + iy; slot i is an inlier iff
 *                           |(q_i - q_a)(p_b - p_a) - (q_b - q_a)(p_i - p_a)|^2 <= tolerance^2 |p_b - p_a|^2
 *                       which is |q_i - (q_a + s (p_i - p_a))| <= tolerance for s = (q_b - q_a) / (p_b - p_a), without a division.
 *                       It preserves orientation: no reflections
 *     best hypothesis   the one with the most inliers, then the smallest a, then the smallest b
 *     found             iff a hypothesis exists and its inlier count >= min_inliers
 * Record r is written at spec->data + r * stride, little endian, stride = 128 + 4 K:
 *     u32 usable; u32 hypotheses; u32 inliers; u32 found; i32 a; i32 b; u32 zero[2];
 *     i64 sum[12]         over the inliers, with (x, y) = p and (u, v) = q:
 *                         Σx, Σy, Σu, Σv, Σxx, Σxy, Σyy, Σxu, Σyu, Σxv, Σyv, Σ(uu + vv)
 *     K x u32 flags       H264BSDMI_MODEL_USABLE, H264BSDMI_MODEL_INLIER
 * usable counts the usable pairs, hypotheses those that passed the gates (TRANSLATION: the usable slots); b = -1 for TRANSLATION; not
 * found gives inliers = 0, a = b = -1, all sums 0 and no inlier bit.  Slot indices are those of the point records.  Everything is an
 * integer and exact, and no result depends on scheduling.  (With K odd a record is 4-byte aligned only: read the sums accordingly.)
 * -1, before anything is enqueued, nothing written: spec NULL; data, matches, kept_points or current_points NULL or not 8-byte aligned;
 * max_points outside 1 .. 256; model > 1; tolerance > 255; max_scale neither 0 nor in 256 .. 4096, or not 0 for TRANSLATION; min_inliers
 * outside 1 .. 256, or 1 for SIMILARITY; zero != 0; n == 0 with nRecords > 0; a NULL or repeated instance; nRecords > 65535; a
 * capture-mode instance; a sink without the entry; instances on more than one device.  -2: the engine failed, or refused a capturing
 * stream: nothing was enqueued. */
#define H264BSDMI_MODEL_TRANSLATION 0u
#define H264BSDMI_MODEL_SIMILARITY  1u
#define H264BSDMI_MODEL_USABLE 1u
#define H264BSDMI_MODEL_INLIER 2u
#define H264BSDMI_MODEL_MAX_POINTS 256u
typedef struct h264bsdmi_model_spec {
    void       *data;            /* DEVICE, caller-owned, 8-byte aligned: record r at data + r * (128 + 4 K) */
    const void *matches;         /* DEVICE, 8-byte aligned: records of h264bsdmiOutputPointMatches at max_points == K, stride 32 + 80 K */
    const void *kept_points;     /* DEVICE, 8-byte aligned: records of h264bsdmiOutputCornerPoints at max_points == K, */
    const void *current_points;  /*   stride 32 + 16 K: the two the matches were made from */
    u32 max_points;              /* K, 1 .. 256 */
    u32 model;                   /* H264BSDMI_MODEL_TRANSLATION / _SIMILARITY */
    u32 tolerance;               /* 0 .. 255, whole luma samples */
    u32 max_scale;               /* in 256ths: 0 = no gate, else 256 .. 4096; SIMILARITY only, 0 for TRANSLATION */
    u32 min_inliers;             /* 1 .. 256; SIMILARITY: 2 .. 256 */
    u32 zero[3];                 /* must be 0 */
} h264bsdmi_model_spec;
int h264bsdmiOutputPointModel(u32 n, storage_t *const *pStorage, u32 nRecords, const h264bsdmi_model_spec *spec, void *stream);

/* ---- host parse pipeline at scale ----
 * h264bsdDecode() consumes one NAL unit of one stream per call; a caller that feeds hundreds of streams needs the
 * loop of posix/test_h264bsd.c:146-177 for each of them and its own threading.  These entry points move both into
 * the library. */
/* Feed NAL units of one instance until a picture is complete: calls h264bsdDecode() on buf, buf+readBytes, ...
 * and stops after H264BSD_PIC_RDY or when the buffer is used up.  H264BSD_RDY / H264BSD_HDRS_RDY continue, errors
 * are counted in *nErrors (may be NULL) and skipped like the reference harness does.  Returns the last status
 * (H264BSD_PIC_RDY, or H264BSD_RDY at the end of the buffer); *consumed = bytes to advance. */
u32 h264bsdmiDecodePicture(storage_t *pStorage, u8 *buf, u32 len, u32 picId, u32 *consumed, u32 *nErrors);
/* The same for n independent instances at once, on the library's parser threads (the caller's thread helps).
 * status[i] / consumed[i] / nErrors[i] (nErrors may be NULL) as above.  Instances must be distinct. */
int h264bsdmiDecodePictureBatch(u32 n, storage_t *const *pStorage, u8 *const *buf, const u32 *len, const u32 *picId,
                                u32 *status, u32 *consumed, u32 *nErrors);
/* h264bsdNextOutputPicture() (src/h264bsd_decoder.c:599-646) of n distinct instances at once, on the same threads: every thread
 * enqueues its instances' pictures on their way out (layout kernel + copy into pinned host memory) and waits for ITS copies
 * only — the engine's lock is held while enqueueing, never while waiting — so the 3.1 MB transfers of the instances overlap.
 * pictures[i] = NULL when instance i has no picture to give; picId / isIdrPic / numErrMbs may be NULL.  0 = ok. */
int h264bsdmiNextOutputPictureBatch(u32 n, storage_t *const *pStorage, u8 **pictures, u32 *picId, u32 *isIdrPic, u32 *numErrMbs);
/* Both in one call — one round of the reference harness's per-stream loop (posix/test_h264bsd.c:146-177: take the pictures that are
 * ready, then decode on) for n distinct instances: every thread FIRST pulls its instance's next output picture (as above:
 * pictures[i], outPicId[i], outIsIdrPic[i], outNumErrMbs[i]; the last three may be NULL) and THEN parses that instance's next
 * picture (as h264bsdmiDecodePicture: buf / len / picId -> status / consumed / nErrors).  The pictures of some instances cross the
 * link while other instances are parsed; with the two calls above the CPUs wait for the link and the link for the CPUs.
 * An instance that still has FURTHER pictures waiting in its output queue is not fed — the next slice would discard them, as in the
 * reference (src/h264bsd_dpb.c:1260-1261): status[i] = H264BSD_RDY, consumed[i] = 0, call again.  len[i] = 0: pull only.
 * pictures[i] stays valid until the next pull from instance i (it is the pinned host mirror of the picture's DPB slot, which the
 * parsing of later pictures does not touch, and which survives the activation of a new sequence parameter set) — longer than the
 * reference's "until the next h264bsdDecode()"; its dimensions are those the instance reported BEFORE the call.  0 = ok. */
int h264bsdmiPullAndDecodePictureBatch(u32 n, storage_t *const *pStorage, u8 **pictures, u32 *outPicId, u32 *outIsIdrPic, u32 *outNumErrMbs,
                                       u8 *const *buf, const u32 *len, const u32 *picId, u32 *status, u32 *consumed, u32 *nErrors);
/* Number of parser threads (default: the CPUs the process may use — affinity mask, cgroup quota + a quarter — divided by H264BSDMI_HOST_SHARE,
 * at most 64; env H264BSDMI_THREADS).  Returns the value in use.  With the default, batches that PULL pictures run on at most as many of
 * these threads as the process may have running at once (the quota itself); a count named here or in the environment is used as it is. */
int h264bsdmiSetParserThreads(int n);
/* INPUT BUFFERS ARE MODIFIED by h264bsdDecode() and by the two calls above, exactly as by the reference: the emulation-
 * prevention bytes of the NAL unit just parsed are removed IN the caller's buffer (src/h264bsd_byte_stream.c), so that a
 * caller who feeds the same bytes again sees what the reference's caller sees.  Consequences: every decoder instance needs
 * its own private, writable copy of the stream (never hand one buffer to several instances of a batch, never a read-only
 * mapping).  on != 0 switches the write-back off for this instance: the buffer may then be shared and read-only; pictures are
 * the same, the h264bsdDecode() call trace can differ from the reference's only where a NAL unit that contains emulation-
 * prevention bytes is fed a second time.  Returns 0. */
int h264bsdmiSetInputReadOnly(storage_t *pStorage, u32 on);
/* Copy elision.  The parser knows what every macroblock tile of every frame buffer holds: a P macroblock that copies the
 * co-located macroblock of its reference (zero motion, no residual) and that no deblocking edge touches leaves its tile
 * equal to the reference's, and frame buffers are reused in rotation — so the buffer a picture is decoded into often holds
 * exactly those bytes already (a region that has not changed since the buffer's previous picture).  Such copies are left out
 * of the frame job: nothing is read, nothing is written, the picture is bit-identical.  ON by default for decoders bound
 * to a device (env H264BSDMI_COPY_ELISION=0 switches it off for the process), OFF by default in capture mode, where a
 * frame job is then a pure function of its picture; a capture that is replayed IN ORDER from an IDR picture onto frames
 * that persist (the bench harness's replay sets) may switch it on.  Call before the first h264bsdDecode().  Returns 0. */
int h264bsdmiSetCopyElision(storage_t *pStorage, u32 on);

/* ---- device engine ---- */
/* Number of usable GPUs (0 when the HIP runtime finds none); selects the device for this process. */
int  h264bsdmiDeviceCount(void);
int  h264bsdmiSetDevice(int device);
/* Run every queued frame job of every decoder instance of this process now (they are otherwise run
 * lazily, when the first picture is pulled).  Returns 0 on success. */
int  h264bsdmiFlush(void);
/* Sticky device error bits (0 = none): 1 a residual outside [-512,511] reached the kernels (the host parser finds this
 * decode error while it parses, so the kernels' check is a tripwire), 2 / 4 the intra / deblocking scheduler of a
 * picture gave up.  Any bit means that pixels were produced that cannot be trusted; the library also says so on stderr. */
unsigned h264bsdmiDeviceErrors(void);
/* Like h264bsdmiFlush() but returns as soon as the copies and kernels are enqueued, so that parsing the next
 * pictures overlaps the reconstruction of these.  Any call that needs pixels (h264bsdNextOutputPicture*,
 * h264bsdmiFlush) waits for the outstanding work first. */
int  h264bsdmiFlushAsync(void);

#ifdef __cplusplus
}
#endif
#endif
