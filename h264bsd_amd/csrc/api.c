/*
 * api.c — the exported h264bsd* C API (include/h264bsd_decoder.h) on top of the host parser and
 * the HIP engine.  Mirrors the reference's public functions one to one
 * (src/h264bsd_decoder.c:90-1370); see the header for the per-function citations.
 *
 * There is no CPU pixel path in this library: h264bsdInit() binds the instance to the HIP engine
 * and fails loudly (stderr + HANTRO_NOK) when no gfx950 device is usable.  The only GPU-less mode is
 * h264bsdmiInitCapture(), which produces frame jobs and never pixels.
 */
#define _GNU_SOURCE
#include <pthread.h>
#include <sched.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "../../include/h264bsd_mi355x_bench.h"
#include "hostdec.h"
#include "engine.h"
#include "descriptor_pattern.h"
#pragma weak eng_sink_entries     /* an engine without it (a device stand-in of the tests) gives NULL: the calls that need an entry of it refuse */
static const EngSinkEntries *sink_entries(const JobSink *k) { return eng_sink_entries ? eng_sink_entries(k) : NULL; }

HostDec *hd_create(int no_output_reordering);
void hd_destroy(HostDec *d);
int hd_decode(HostDec *d, uint8_t *stream, uint32_t len, uint32_t pic_id, uint32_t *read_bytes);

typedef struct ApiDec {
    HostDec *hd;
    h264bsdmi_job_cb cb;
    void *cb_user;
    /* the current picture: the one popped last (pop_output), until the instance decodes again or is flushed (drop_current) —
     * what h264bsdmiOutputTensorRegions samples.  A copy: the output queue is rewritten by the decode calls only, but so is this. */
    OutPic cur;
    int has_cur;
    int fed;        /* h264bsdDecode has been called: too late for h264bsdmiSetMotionExport */
    int motion;     /* motion export is on (h264bsdmiSetMotionExport) */
    /* the kept picture (h264bsdmiKeepCurrentPictures): the engine holds its bytes, this is what is known about it without asking.  It
     * counts only while kept_wmb x kept_hmb is the HostDec's coded size (has_kept_picture): the engine frees the buffer when a sequence
     * of another size is configured, and h264bsdDecode forgets it for good when it sees the size change */
    int has_kept;
    u32 kept_id, kept_wmb, kept_hmb;
    /* the spread beside it (h264bsdmiBlendCurrentPicturesSpread): valid from a spread blend to the next plain keep, and only while the
     * kept picture counts (has_spread) */
    int spread_valid;
} ApiDec;

/* Every H264BSDMI_* variable this library reads (tests/test_abi.py compares the list with the sources and INTEGRATION.md).  A
 * variable of that family that is NOT in the list — a typing error, or a switch of an earlier release — is named on stderr when
 * the library is loaded instead of being silently ignored. */
extern char **environ;
__attribute__((constructor)) static void report_unknown_switches(void)
{
    static const char *const known[] = { "H264BSDMI_LANES", "H264BSDMI_TAIL", "H264BSDMI_BAND_BUDGET", "H264BSDMI_HEAVY_BUDGET", "H264BSDMI_TRACE_LANES",
                                         "H264BSDMI_COPY_ELISION", "H264BSDMI_THREADS", "H264BSDMI_HOST_SHARE", "H264BSDMI_PIN", NULL };
    for (char **e = environ; e && *e; e++) {
        if (strncmp(*e, "H264BSDMI_", 10) != 0) continue;
        const char *eq = strchr(*e, '=');
        const size_t len = eq ? (size_t)(eq - *e) : strlen(*e);
        int ok = 0;
        for (int k = 0; known[k] && !ok; k++) ok = strlen(known[k]) == len && strncmp(known[k], *e, len) == 0;
        if (!ok) fprintf(stderr, "h264bsd-mi355x: unknown environment switch %.*s ignored (INTEGRATION.md lists the ones this library reads)\n", (int)len, *e);
    }
}

static ApiDec *dec_of(storage_t *s) { return s ? (ApiDec *)s->opaque : NULL; }
static void drop_current(ApiDec *a) { if (a) a->has_cur = 0; }
static int has_kept_picture(const ApiDec *a) { return a->has_kept && a->kept_wmb == a->hd->width_mbs && a->kept_hmb == a->hd->height_mbs; }
static int has_spread(const ApiDec *a) { return has_kept_picture(a) && a->spread_valid; }

/* ---- capture sink ---- */
static int cap_configure(void *u, uint32_t w, uint32_t h, uint32_t n) { (void)u; (void)w; (void)h; (void)n; return 0; }
static int cap_submit(void *u, const uint8_t *blob, uint32_t bytes)
{
    ApiDec *a = (ApiDec *)u;
    if (a->cb) a->cb(a->cb_user, blob, bytes);
    return 0;
}

static u32 init_common(storage_t *s, u32 no_reorder, h264bsdmi_job_cb cb, void *user, int capture)
{
    if (!s) return HANTRO_NOK;
    memset(s, 0, sizeof(*s));
    ApiDec *a = (ApiDec *)calloc(1, sizeof(ApiDec));
    if (!a) return HANTRO_NOK;
    a->hd = hd_create((int)no_reorder);
    if (!a->hd) { free(a); return HANTRO_NOK; }
    if (capture) {
        a->cb = cb;
        a->cb_user = user;
        a->hd->sink.user = a;
        a->hd->sink.configure = cap_configure;
        a->hd->sink.submit = cap_submit;
    } else if (eng_attach(&a->hd->sink)) {
        fprintf(stderr, "h264bsd-mi355x: h264bsdInit failed: no usable HIP device (this library has no CPU pixel path)\n");
        hd_destroy(a->hd);
        free(a);
        return HANTRO_NOK;
    } else {
        /* bound to a device: the frames live from job to job, copies that would rewrite what a tile holds are left out
         * (hostdec.h, copy elision).  H264BSDMI_COPY_ELISION=0 switches it off for the process. */
        const char *e = getenv("H264BSDMI_COPY_ELISION");
        a->hd->copy_elision = !(e && *e == '0');
        a->hd->sink_errors_at_start = a->hd->sink.errors ? a->hd->sink.errors(a->hd->sink.user) : 0;
    }
    s->opaque = a;
    return HANTRO_OK;
}

u32 h264bsdInit(storage_t *s, u32 noOutputReordering) { return init_common(s, noOutputReordering, NULL, NULL, 0); }
u32 h264bsdmiInitCapture(storage_t *s, u32 noOutputReordering, h264bsdmi_job_cb cb, void *user)
{
    return init_common(s, noOutputReordering, cb, user, 1);
}

void h264bsdShutdown(storage_t *s)
{
    ApiDec *a = dec_of(s);
    if (!a) return;
    hd_destroy(a->hd);
    free(a);
    s->opaque = NULL;
}

storage_t *h264bsdAlloc(void) { return (storage_t *)calloc(1, sizeof(storage_t)); }
void h264bsdFree(storage_t *s) { free(s); }

u32 h264bsdDecode(storage_t *s, u8 *byteStrm, u32 len, u32 picId, u32 *readBytes)
{
    ApiDec *a = dec_of(s);
    drop_current(a);
    if (!a || !byteStrm || !len || !readBytes) return H264BSD_ERROR;
    a->fed = 1;
    const u32 r = (u32)hd_decode(a->hd, byteStrm, len, picId, readBytes);
    if (a->has_kept && !has_kept_picture(a)) a->has_kept = a->spread_valid = 0;      /* a sequence of another coded size: the kept picture is gone, and its spread */
    return r;
}

static const OutPic *pop_output(ApiDec *a, u32 *picId, u32 *isIdrPic, u32 *numErrMbs)
{
    const OutPic *o = hd_dpb_next_output(&a->hd->dpb);
    if (!o) return NULL;
    a->cur = *o;
    a->has_cur = 1;
    if (picId) *picId = o->pic_id;
    if (isIdrPic) *isIdrPic = o->is_idr;
    if (numErrMbs) *numErrMbs = o->num_err_mbs;
    return o;
}

u8 *h264bsdNextOutputPicture(storage_t *s, u32 *picId, u32 *isIdrPic, u32 *numErrMbs)
{
    ApiDec *a = dec_of(s);
    if (!a) return NULL;
    const OutPic *o = pop_output(a, picId, isIdrPic, numErrMbs);
    if (!o || !a->hd->sink.fetch) return NULL;
    return a->hd->sink.fetch(a->hd->sink.user, o->slot);
}

int h264bsdmiSetInputReadOnly(storage_t *s, u32 on)
{
    ApiDec *a = dec_of(s);
    if (!a) return -1;
    a->hd->input_readonly = on ? 1 : 0;
    return 0;
}

int h264bsdmiSetCopyElision(storage_t *s, u32 on)
{
    ApiDec *a = dec_of(s);
    if (!a) return -1;
    a->hd->copy_elision = on ? 1 : 0;
    return 0;
}

int h264bsdmiSetMotionExport(storage_t *s, u32 on)
{
    ApiDec *a = dec_of(s);
    if (!a || a->fed || !a->hd->sink.set_motion) return -1;               /* capture mode: there is no device to keep it on */
    if (a->hd->sink.set_motion(a->hd->sink.user, on ? 1 : 0)) return -1;
    a->motion = on ? 1 : 0;
    return 0;
}

int h264bsdmiNextOutputInfo(storage_t *s, u32 *picId, u32 *isIdrPic, u32 *numErrMbs)
{
    ApiDec *a = dec_of(s);
    if (!a) return -1;
    const OutPic *o = pop_output(a, picId, isIdrPic, numErrMbs);
    return o ? (int)o->slot : -1;
}

/* The source window of an SPS in luma samples: the coded frame, or (crop) its frame-cropping window where it has one */
static void sps_window(const Sps *sps, int crop, u32 *x0, u32 *y0, u32 *w, u32 *h)
{
    *x0 = *y0 = 0;
    *w = 16 * sps->width_mbs;
    *h = 16 * sps->height_mbs;
    if (crop && sps->cropping) {
        *x0 = 2 * sps->crop_left;
        *y0 = 2 * sps->crop_top;
        *w -= 2 * (sps->crop_left + sps->crop_right);
        *h -= 2 * (sps->crop_top + sps->crop_bottom);
    }
}

int h264bsdmiNextOutputPictureDevice(storage_t *s, int format, int crop, h264bsdmi_device_picture *out)
{
    ApiDec *a = dec_of(s);
    if (!a || !out || format < 0 || format > 3) return -1;
    if (!a->hd->sink.fetch_device) return -1;               /* capture mode: there are no pixels */
    const Sps *sps = a->hd->active_sps;
    if (!sps) return 0;
    u32 id = 0, idr = 0, nerr = 0;
    const OutPic *o = pop_output(a, &id, &idr, &nerr);
    if (!o) return 0;
    u32 x0, y0, w, h;
    sps_window(sps, crop, &x0, &y0, &w, &h);
    void *stream = NULL;
    void *p = a->hd->sink.fetch_device(a->hd->sink.user, o->slot, format, x0, y0, w, h, &stream);
    if (!p) return -2;
    out->data = p;
    out->width = w;
    out->height = h;
    out->pitch = format == H264BSDMI_FMT_I420 ? w : 4 * w;
    out->format = (u32)format;
    out->picId = id;
    out->isIdrPic = idr;
    out->numErrMbs = nerr;
    out->stream = stream;
    return 1;
}

/* The next pictures of n instances into one caller-owned device tensor.  Everything that can be refused is refused before the first
 * pop: the spec, the instances (bound to a device, distinct), every source window against the output size; the pictures are only
 * popped once the engine has enqueued their layout. */
static int sps_full_range(const Sps *p) { return p && p->vui_present && p->video_signal_type_present && p->video_full_range; }
static u32 sps_matrix_coefficients(const Sps *p)
{
    if (p && p->vui_present && p->video_signal_type_present && p->colour_description_present) return p->matrix_coefficients;
    return 2;   /* unspecified */
}
/* H264BSDMI_MATRIX_* of matrix_coefficients (H.264 Table E-5); `unspecified` for 2 and the ones without a Kr / Kb matrix here */
static u32 matrix_of(u32 mc, u32 unspecified)
{
    switch (mc) {
    case 1: return H264BSDMI_MATRIX_BT709;
    case 4: return H264BSDMI_MATRIX_FCC;
    case 5: case 6: return H264BSDMI_MATRIX_BT601;
    case 7: return H264BSDMI_MATRIX_SMPTE240;
    case 9: return H264BSDMI_MATRIX_BT2020;
    }
    return unspecified;
}

int h264bsdmiNextOutputTensorBatch(u32 n, storage_t *const *dec, const h264bsdmi_tensor_spec *spec, void *stream,
                                   u32 *got, u32 *picId, u32 *isIdrPic, u32 *numErrMbs)
{
    return h264bsdmiNextOutputTensorBatchColour(n, dec, spec, NULL, stream, got, picId, isIdrPic, numErrMbs);
}

int h264bsdmiNextOutputTensorBatchColour(u32 n, storage_t *const *dec, const h264bsdmi_tensor_spec *spec,
                                         const h264bsdmi_colour_spec *colour, void *stream,
                                         u32 *got, u32 *picId, u32 *isIdrPic, u32 *numErrMbs)
{
    return h264bsdmiNextOutputTensorBatchResize(n, dec, spec, colour, NULL, stream, got, picId, isIdrPic, numErrMbs, NULL);
}

/* The letterbox rectangle of a w x h window in a W x H output (include/h264bsd_mi355x.h), in double (the truncations are floors:
 * every operand is positive) */
static u32 lb_side(u32 n, double s, u32 N)
{
    const u32 v = (u32)(n * s + 0.5);
    return v < 1 ? 1 : v > N ? N : v;
}
static void letterbox(u32 W, u32 H, u32 w, u32 h, u32 *box)
{
    const double sw = (double)W / w, sh = (double)H / h, s = sw < sh ? sw : sh;
    box[2] = lb_side(w, s, W);
    box[3] = lb_side(h, s, H);
    box[0] = (W - box[2]) / 2;
    box[1] = (H - box[3]) / 2;
}

/* What every tensor pull refuses in its three specs (1 = refused).  *colour == NULL becomes REFERENCE, the reference's conversion. */
static const h264bsdmi_colour_spec REFERENCE_COLOUR = { H264BSDMI_MATRIX_REFERENCE, 0, 0, 0 };
static int tensor_specs_refused(const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec **pcolour, const h264bsdmi_resize_spec *resize)
{
    if (!spec || !spec->data || !spec->width || !spec->height) return 1;
    if (resize) {
        if (resize->filter > H264BSDMI_FILTER_BICUBIC_AA || resize->fit > H264BSDMI_FIT_LETTERBOX || spec->resize != 1) return 1;
        for (int c = 0; c < 3; c++)
            if (!(resize->pad[c] >= 0.0f && resize->pad[c] <= 1.0f)) return 1;        /* NaN and the infinities too */
    }
    if (!*pcolour) *pcolour = &REFERENCE_COLOUR;
    const h264bsdmi_colour_spec *colour = *pcolour;
    if (colour->matrix > H264BSDMI_MATRIX_SMPTE240 || colour->range > H264BSDMI_RANGE_FULL || colour->chroma > H264BSDMI_CHROMA_BILINEAR)
        return 1;
    if (colour->unspecified && (colour->unspecified < H264BSDMI_MATRIX_BT601 || colour->unspecified > H264BSDMI_MATRIX_SMPTE240)) return 1;
    if (colour->matrix == H264BSDMI_MATRIX_AUTO && !colour->unspecified) return 1;
    if (colour->matrix == H264BSDMI_MATRIX_REFERENCE && (colour->range || colour->chroma || colour->unspecified)) return 1;
    if (spec->layout > H264BSDMI_LAYOUT_NHWC || spec->dtype > H264BSDMI_DTYPE_F32 || spec->channels > H264BSDMI_CH_Y) return 1;
    if (spec->layout == H264BSDMI_LAYOUT_NCHW && (spec->channels == H264BSDMI_CH_RGBA || spec->channels == H264BSDMI_CH_BGRA)) return 1;
    for (int c = 0; c < 3; c++) {
        if (spec->std[c] == 0.0f) return 1;
        if (spec->dtype == H264BSDMI_DTYPE_U8 && (spec->mean[c] != 0.0f || spec->std[c] != 1.0f)) return 1;
    }
    return 0;
}

/* The picture in frame buffer `slot` of instance a (which has an active SPS) as slice `index` of a tensor pull: its source window,
 * AUTO matrix and range resolved from the SPS the window comes from; the box is the whole output */
static void tensor_pic(SinkTensorPic *p, const ApiDec *a, u32 slot, u32 index, const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec *colour)
{
    const Sps *sps = a->hd->active_sps;
    u32 x0, y0, w, h;
    sps_window(sps, spec->crop != 0, &x0, &y0, &w, &h);
    u32 matrix = colour->matrix, range = colour->range;
    if (matrix == H264BSDMI_MATRIX_AUTO) matrix = matrix_of(sps_matrix_coefficients(sps), colour->unspecified);
    if (matrix != H264BSDMI_MATRIX_REFERENCE && range == H264BSDMI_RANGE_AUTO) range = sps_full_range(sps) ? H264BSDMI_RANGE_FULL : H264BSDMI_RANGE_LIMITED;
    *p = (SinkTensorPic){ &a->hd->sink, slot, index, x0, y0, w, h, matrix, range, { 0, 0, spec->width, spec->height } };
}

/* colour == NULL: REFERENCE, the reference's conversion.  Otherwise AUTO matrix and range are resolved here, per instance, from the
 * active SPS the window comes from (the conditions of h264bsdMatrixCoefficients / h264bsdVideoRange).  resize == NULL: stretch with
 * resize = 1's bilinear; the engine keeps {FILTER_BILINEAR, FIT_STRETCH} on that path too. */
int h264bsdmiNextOutputTensorBatchResize(u32 n, storage_t *const *dec, const h264bsdmi_tensor_spec *spec,
                                         const h264bsdmi_colour_spec *colour, const h264bsdmi_resize_spec *resize,
                                         void *stream, u32 *got, u32 *picId, u32 *isIdrPic, u32 *numErrMbs,
                                         u32 *box)
{
    if (!dec || !got || tensor_specs_refused(spec, &colour, resize)) return -1;
    if (!n) return 0;
    SinkTensorPic *pics = (SinkTensorPic *)malloc(n * sizeof(SinkTensorPic));
    if (!pics) return -1;
    u32 m = 0;
    int rc = 0;
    for (u32 i = 0; i < n && !rc; i++) {
        ApiDec *a = dec_of(dec[i]);
        if (!a || !a->hd->sink.tensor_out) { rc = -1; break; }              /* capture mode: there are no pixels */
        for (u32 k = 0; k < i; k++)
            if (dec[k] == dec[i]) rc = -1;
        const Dpb *d = &a->hd->dpb;
        const Sps *sps = a->hd->active_sps;
        if (rc || !sps || d->out_idx >= d->n_out) continue;                  /* nothing to give: got[i] = 0 */
        SinkTensorPic *p = &pics[m++];
        tensor_pic(p, a, d->out[d->out_idx].slot, i, spec, colour);
        if (!spec->resize && (p->w != spec->width || p->h != spec->height)) { rc = -1; break; }
        if (resize && resize->fit == H264BSDMI_FIT_LETTERBOX) letterbox(spec->width, spec->height, p->w, p->h, p->box);
    }
    if (!rc && m && pics[0].sink->tensor_out(m, pics, spec, colour->chroma, resize, stream)) rc = -2;
    if (!rc && box) {
        memset(box, 0, 4 * sizeof(u32) * n);
        for (u32 k = 0; k < m; k++) memcpy(box + 4 * pics[k].index, pics[k].box, sizeof(pics[k].box));
    }
    free(pics);
    if (rc) return rc;
    for (u32 i = 0; i < n; i++) {
        u32 id = 0, idr = 0, nerr = 0;
        ApiDec *a = dec_of(dec[i]);
        got[i] = a->hd->active_sps && pop_output(a, &id, &idr, &nerr) ? 1 : 0;
        if (picId) picId[i] = id;
        if (isIdrPic) isIdrPic[i] = idr;
        if (numErrMbs) numErrMbs[i] = nerr;
    }
    return 0;
}

/* ---- The pulls of CURRENT pictures (pop_output, drop_current): h264bsdmiOutputTensorRegions, h264bsdmiOutputTensorRemap,
 * h264bsdmiOutputMotionRegions, h264bsdmiOutputRegionStats, h264bsdmiOutputCornerPoints, h264bsdmiOutputRegionChange and h264bsdmiOutputRegionShift (which need the kept picture as well),
 * h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes (which need it in CHANGE mode), and their small siblings h264bsdmiKeepCurrentPictures and h264bsdmiBlendCurrentPictures (the picture list only).  Each checks its own spec; everything else is one path:
 *   regions_refused   got, the count and the range of every region — before the instances are looked at
 *   pull_begin        dec and the instances (of this library, with the sink entry the call needs, distinct), then the lists
 *   pull_pic          an instance's current picture in the picture list, appended at its first use
 *   pull_regions      the regions (or one whole window per instance) of the pictures that exist, each with its rectangle
 *   pull_finish       after the sink: got, box, current and picId — unless the sink failed (-2 writes nothing) — and the lists freed
 * A refused call returns -1 and has called no sink, written nothing; no call pops anything. */
enum { PULL_REGIONS, PULL_REMAP, PULL_MOTION, PULL_STATS, PULL_CHANGE, PULL_KEEP, PULL_CELLS, PULL_BOXES, PULL_SHIFT, PULL_CORNERS, PULL_FLOW, PULL_MATCHES };
#define NO_PIC 0xFFFFFFFFu
typedef struct CurrentPull {
    u32 n, m, k;                /* instances; pictures and items gathered so far */
    storage_t *const *dec;
    SinkTensorPic *pics;        /* one per instance that has a current picture and at least one item, in the order of first use */
    u32 *pic_of;                /* per instance: its index in pics, NO_PIC before its first use */
    SinkRegion *regs;           /* the items for the sink: regions, or (PULL_REMAP) maps */
    SinkRemap *maps;
    int kind;                   /* PULL_* */
    int vs_kept;                /* only instances that have a kept picture too: PULL_CHANGE, PULL_SHIFT, PULL_FLOW, PULL_MATCHES, and PULL_CELLS / PULL_BOXES in CHANGE mode */
    int vs_spread;              /* ... and a valid spread: PULL_CELLS / PULL_BOXES in SPREAD mode */
} CurrentPull;

/* regions == NULL: no regions at all, or (whole: one whole window per instance) exactly n */
static int regions_refused(u32 n, u32 nRegions, const h264bsdmi_region *regions, const u32 *got, int whole)
{
    const int LIMIT = 16384;
    if (nRegions && !got) return 1;
    if (nRegions > 65535u) return 1;
    if (!regions) return nRegions != (whole ? n : 0u);
    for (u32 r = 0; r < nRegions; r++) {
        const h264bsdmi_region *g = &regions[r];
        if (g->instance >= n || !g->w || !g->h || g->w > (u32)LIMIT || g->h > (u32)LIMIT) return 1;
        if (g->x > LIMIT || g->x < -LIMIT || g->y > LIMIT || g->y < -LIMIT) return 1;
    }
    return 0;
}
/* 1 when the sink has what a pull of `kind` calls (capture mode has none of it: there are no pixels) */
static int sink_pulls(const ApiDec *a, int kind)
{
    const JobSink *k = &a->hd->sink;
    switch (kind) {
    case PULL_REMAP:  return k->tensor_remap != NULL;
    case PULL_MOTION: return k->motion_regions != NULL && a->motion;          /* ... and motion export is on */
    case PULL_STATS:  return k->tensor_regions != NULL && k->region_stats != NULL;
    case PULL_CORNERS: return k->tensor_regions != NULL && k->corner_points != NULL;
    case PULL_CHANGE: return k->tensor_regions != NULL && k->region_change != NULL && k->keep_pictures != NULL;
    case PULL_SHIFT:  return k->tensor_regions != NULL && k->region_shift != NULL && k->keep_pictures != NULL;
    case PULL_KEEP:   return k->tensor_regions != NULL && k->keep_pictures != NULL;
    case PULL_CELLS:  return k->tensor_regions != NULL && k->cell_maps != NULL;      /* CHANGE mode: keep_pictures too (the entry asks) */
    case PULL_BOXES:  return k->tensor_regions != NULL && k->cell_maps != NULL && k->cell_boxes != NULL;
    case PULL_FLOW:   return k->tensor_regions != NULL && k->keep_pictures != NULL && sink_entries(k) && sink_entries(k)->cell_shift != NULL;      /* (engine.h) */
    case PULL_MATCHES: return k->tensor_regions != NULL && k->keep_pictures != NULL && sink_entries(k) && sink_entries(k)->point_matches != NULL;
    }
    return k->tensor_regions != NULL;
}
static void pull_free(CurrentPull *c) { free(c->pics); free(c->pic_of); free(c->regs); free(c->maps); }
static int pull_begin(CurrentPull *c, u32 n, storage_t *const *dec, u32 n_items, int kind)
{
    if (n && !dec) return -1;
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        if (!a || !sink_pulls(a, kind)) return -1;
        for (u32 k = 0; k < i; k++)
            if (dec[k] == dec[i]) return -1;
    }
    *c = (CurrentPull){ n, 0, 0, dec, (SinkTensorPic *)malloc((n ? n : 1) * sizeof(SinkTensorPic)), (u32 *)malloc((n ? n : 1) * sizeof(u32)),
                        kind == PULL_REMAP ? NULL : (SinkRegion *)malloc((n_items ? n_items : 1) * sizeof(SinkRegion)),
                        kind == PULL_REMAP ? (SinkRemap *)malloc((n_items ? n_items : 1) * sizeof(SinkRemap)) : NULL, kind, kind == PULL_CHANGE || kind == PULL_SHIFT, 0 };
    if (!c->pics || !c->pic_of || !(c->regs || c->maps)) { pull_free(c); return -1; }
    for (u32 i = 0; i < n; i++) c->pic_of[i] = NO_PIC;
    return 0;
}
/* the index in pics of instance inst's current picture, NO_PIC when it has none (got = 0 for what names it); vs_kept: when it has
 * no kept picture either */
static u32 pull_pic(CurrentPull *c, u32 inst, const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec *colour)
{
    const ApiDec *a = dec_of(c->dec[inst]);
    if (!a->has_cur || !a->hd->active_sps) return NO_PIC;
    if (c->vs_kept && !has_kept_picture(a)) return NO_PIC;
    if (c->vs_spread && !has_spread(a)) return NO_PIC;
    if (c->pic_of[inst] == NO_PIC) {
        c->pic_of[inst] = c->m;
        tensor_pic(&c->pics[c->m++], a, a->cur.slot, inst, spec, colour);
    }
    return c->pic_of[inst];
}
/* regions (NULL: instance r's whole window is region r) into the rectangle a W x H output gives each: all of it, or its letterbox */
static void pull_regions(CurrentPull *c, u32 nRegions, const h264bsdmi_region *regions, const h264bsdmi_tensor_spec *spec,
                         const h264bsdmi_colour_spec *colour, u32 W, u32 H, int letterboxed)
{
    for (u32 r = 0; r < nRegions; r++) {
        const u32 pic = pull_pic(c, regions ? regions[r].instance : r, spec, colour);
        if (pic == NO_PIC) continue;
        SinkRegion *q = &c->regs[c->k++];
        if (regions) *q = (SinkRegion){ pic, r, regions[r].x, regions[r].y, regions[r].w, regions[r].h, { 0, 0, W, H } };
        else *q = (SinkRegion){ pic, r, 0, 0, c->pics[pic].w, c->pics[pic].h, { 0, 0, W, H } };
        if (letterboxed) letterbox(W, H, q->w, q->h, q->box);
    }
}
/* failed: what the sink returned.  got[0 .. n_items), box (NULL, or 4 per item: regions only), current / picId (each may be NULL) */
static int pull_finish(CurrentPull *c, int failed, u32 n_items, u32 *got, u32 *box, u32 *current, u32 *picId)
{
    if (!failed) {
        for (u32 r = 0; r < n_items; r++) got[r] = 0;
        if (box) memset(box, 0, 4 * sizeof(u32) * n_items);
        for (u32 j = 0; j < c->k; j++) {
            const u32 index = c->regs ? c->regs[j].index : c->maps[j].index;
            got[index] = 1;
            if (box) memcpy(box + 4 * index, c->regs[j].box, sizeof(c->regs[j].box));
        }
        for (u32 i = 0; i < c->n; i++) {
            const ApiDec *a = dec_of(c->dec[i]);
            const int cur = a->has_cur && a->hd->active_sps;
            if (current) current[i] = cur ? 1 : 0;
            if (picId) picId[i] = cur ? a->cur.pic_id : 0;
        }
    }
    pull_free(c);
    return failed ? -2 : 0;
}

/* Boxes of the instances' current pictures, each into its own slice */
int h264bsdmiOutputTensorRegions(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                                 const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec *colour,
                                 const h264bsdmi_resize_spec *resize, void *stream,
                                 u32 *got, u32 *box, u32 *current, u32 *picId)
{
    static const h264bsdmi_resize_spec stretch = { H264BSDMI_FILTER_BILINEAR, H264BSDMI_FIT_STRETCH, { 0.0f, 0.0f, 0.0f } };
    CurrentPull c;
    if (tensor_specs_refused(spec, &colour, resize) || spec->resize != 1) return -1;
    if (!resize) resize = &stretch;
    if (regions_refused(n, nRegions, regions, got, 0) || pull_begin(&c, n, dec, nRegions, PULL_REGIONS)) return -1;
    pull_regions(&c, nRegions, regions, spec, colour, spec->width, spec->height, resize->fit == H264BSDMI_FIT_LETTERBOX);
    const int failed = c.k && c.pics[0].sink->tensor_regions(c.m, c.pics, c.k, c.regs, spec, colour->chroma, resize, stream);
    return pull_finish(&c, failed, nRegions, got, box, current, picId);
}

/* The instances' current pictures through coordinate maps, each map into its own slice */
int h264bsdmiOutputTensorRemap(u32 n, storage_t *const *dec, u32 nMaps, const h264bsdmi_remap *maps,
                               const h264bsdmi_tensor_spec *spec, const h264bsdmi_colour_spec *colour,
                               const h264bsdmi_remap_spec *remap, void *stream,
                               u32 *got, u32 *current, u32 *picId)
{
    static const h264bsdmi_remap_spec plain = { H264BSDMI_REMAP_BILINEAR, H264BSDMI_BORDER_CONSTANT, { 0.0f, 0.0f, 0.0f } };
    CurrentPull c;
    if (tensor_specs_refused(spec, &colour, NULL) || spec->resize != 1) return -1;
    if (!remap) remap = &plain;
    if (remap->filter > H264BSDMI_REMAP_BILINEAR || remap->border > H264BSDMI_BORDER_REPLICATE) return -1;
    for (int ch = 0; ch < 3; ch++)
        if (!(remap->pad[ch] >= 0.0f && remap->pad[ch] <= 1.0f)) return -1;    /* NaN and the infinities too */
    if (nMaps && (!maps || !got)) return -1;
    if (nMaps > 65535u) return -1;
    for (u32 r = 0; r < nMaps; r++)
        if (maps[r].instance >= n || !maps[r].map || ((uintptr_t)maps[r].map & 7u)) return -1;
    if (pull_begin(&c, n, dec, nMaps, PULL_REMAP)) return -1;
    for (u32 r = 0; r < nMaps; r++) {
        const u32 pic = pull_pic(&c, maps[r].instance, spec, colour);
        if (pic != NO_PIC) c.maps[c.k++] = (SinkRemap){ pic, r, maps[r].map };
    }
    const int failed = c.k && c.pics[0].sink->tensor_remap(c.m, c.pics, c.k, c.maps, spec, colour->chroma, remap, stream);
    return pull_finish(&c, failed, nMaps, got, NULL, current, picId);
}

/* h264bsdmiOutputTensorRegions' regions over the motion side information of the current pictures: the same windows and rectangles */
int h264bsdmiOutputMotionRegions(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                                 const h264bsdmi_motion_spec *spec, void *stream,
                                 u32 *got, u32 *box, u32 *current, u32 *picId)
{
    const u32 planes = H264BSDMI_MOTION_PLANE_MV | H264BSDMI_MOTION_PLANE_VALID | H264BSDMI_MOTION_PLANE_AGE | H264BSDMI_MOTION_PLANE_QP;
    CurrentPull c;
    if (!spec || !spec->data || !spec->width || !spec->height || spec->layout > H264BSDMI_LAYOUT_NHWC) return -1;
    if (spec->dtype != H264BSDMI_DTYPE_F16 && spec->dtype != H264BSDMI_DTYPE_F32) return -1;
    if (!spec->planes || (spec->planes & ~planes) || spec->fit > H264BSDMI_FIT_LETTERBOX || spec->sampler > H264BSDMI_MOTION_AREA ||
        spec->units > H264BSDMI_MOTION_UNITS_OUTPUT || spec->per_picture > 1) return -1;
    if (regions_refused(n, nRegions, regions, got, 1) || pull_begin(&c, n, dec, nRegions, PULL_MOTION)) return -1;
    const h264bsdmi_tensor_spec window = { spec->data, spec->width, spec->height, spec->layout, spec->dtype, 0, spec->crop, 1, { 0, 0, 0 }, { 1, 1, 1 } };
    pull_regions(&c, nRegions, regions, &window, &REFERENCE_COLOUR, spec->width, spec->height, spec->fit == H264BSDMI_FIT_LETTERBOX);
    const int failed = c.k && c.pics[0].sink->motion_regions(c.m, c.pics, c.k, c.regs, spec, stream);
    return pull_finish(&c, failed, nRegions, got, box, current, picId);
}

/* a histogram of `bins` bins: none, or a power of two from 16 to 256 */
static int bins_refused(u32 bins) { return bins != 0 && bins != 16 && bins != 32 && bins != 64 && bins != 128 && bins != 256; }

/* Integer statistics of h264bsdmiOutputTensorRegions' regions over the current pictures: the same windows, no rectangles */
int h264bsdmiOutputRegionStats(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                               const h264bsdmi_stats_spec *spec, void *stream,
                               u32 *got, u32 *current, u32 *picId)
{
    CurrentPull c;
    if (!spec || !spec->data || ((uintptr_t)spec->data & 7u) || spec->source > H264BSDMI_STATS_RGB || spec->crop > 1) return -1;
    if (bins_refused(spec->bins)) return -1;
    if (regions_refused(n, nRegions, regions, got, 1) || pull_begin(&c, n, dec, nRegions, PULL_STATS)) return -1;
    const h264bsdmi_tensor_spec window = { spec->data, 1, 1, 0, 0, 0, spec->crop, 1, { 0, 0, 0 }, { 1, 1, 1 } };
    pull_regions(&c, nRegions, regions, &window, &REFERENCE_COLOUR, 1, 1, 0);
    const int failed = c.k && c.pics[0].sink->region_stats(c.m, c.pics, c.k, c.regs, spec, stream);
    return pull_finish(&c, failed, nRegions, got, NULL, current, picId);
}

/* Corner points of h264bsdmiOutputRegionStats' regions over the current pictures: the same windows and path, no kept picture */
int h264bsdmiOutputCornerPoints(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                                const h264bsdmi_corners_spec *spec, void *stream,
                                u32 *got, u32 *current, u32 *picId)
{
    CurrentPull c;
    if (!spec || !spec->data || ((uintptr_t)spec->data & 7u) || spec->score > H264BSDMI_CORNERS_HARRIS || (spec->block != 3 && spec->block != 5)) return -1;
    if (spec->nms < 1 || spec->nms > H264BSDMI_CORNERS_MAX_NMS || spec->max_points < 1 || spec->max_points > H264BSDMI_CORNERS_MAX_POINTS) return -1;
    if (spec->crop > 1 || spec->zero || (spec->score == H264BSDMI_CORNERS_HARRIS && spec->min_score >> 63)) return -1;
    if (regions_refused(n, nRegions, regions, got, 1) || pull_begin(&c, n, dec, nRegions, PULL_CORNERS)) return -1;
    const h264bsdmi_tensor_spec window = { spec->data, 1, 1, 0, 0, 0, spec->crop, 1, { 0, 0, 0 }, { 1, 1, 1 } };
    pull_regions(&c, nRegions, regions, &window, &REFERENCE_COLOUR, 1, 1, 0);
    const int failed = c.k && c.pics[0].sink->corner_points(c.m, c.pics, c.k, c.regs, spec, stream);
    return pull_finish(&c, failed, nRegions, got, NULL, current, picId);
}

/* The current pictures of the instances as the sink's keep_pictures takes them: whole coded frames, one per instance that has one.
 * mark_kept: after the sink has taken them */
static const h264bsdmi_tensor_spec KEEP_WINDOW = { NULL, 1, 1, 0, 0, 0, 0, 1, { 0, 0, 0 }, { 1, 1, 1 } };
static int keep_begin(CurrentPull *c, u32 n, storage_t *const *dec)
{
    if (pull_begin(c, n, dec, 0, PULL_KEEP)) return -1;
    for (u32 i = 0; i < n; i++) (void)pull_pic(c, i, &KEEP_WINDOW, &REFERENCE_COLOUR);
    return 0;
}
/* plain: a copy (the keep call, a keep_after), which invalidates the spread as it resets the fraction; a blend leaves it */
static void mark_kept(const CurrentPull *c, int plain)
{
    for (u32 i = 0; i < c->n; i++) {
        ApiDec *a = dec_of(c->dec[i]);
        if (c->pic_of[i] == NO_PIC) continue;
        if (plain) a->spread_valid = 0;
        a->has_kept = 1;
        a->kept_id = a->cur.pic_id;
        a->kept_wmb = a->hd->width_mbs;
        a->kept_hmb = a->hd->height_mbs;
    }
}

/* The current picture of each instance becomes its kept picture */
int h264bsdmiKeepCurrentPictures(u32 n, storage_t *const *dec, void *stream, u32 *kept, u32 *picId)
{
    CurrentPull c;
    if (!n) return 0;
    if (!kept || keep_begin(&c, n, dec)) return -1;
    const int failed = c.m && c.pics[0].sink->keep_pictures(c.m, c.pics, stream);
    if (!failed) {
        mark_kept(&c, 1);
        for (u32 i = 0; i < n; i++) {
            const ApiDec *a = dec_of(dec[i]);
            kept[i] = c.pic_of[i] != NO_PIC;
            if (picId) picId[i] = has_kept_picture(a) ? a->kept_id : 0;
        }
    }
    pull_free(&c);
    return failed ? -2 : 0;
}

/* The current picture of each instance blended into its kept picture (the background model); where it has none, the model starts as a
 * copy.  keep_begin and mark_kept are the keep call's; flags: per picture, what the sink is told of the instance's kept picture
 * (ENG_SPREAD_FRESH: there is none) and, with a spread spec, of its spread (ENG_SPREAD_UNSET: none that is valid).  spread NULL: the
 * plain blend through the sink's blend_pictures; else the engine's blend_spread entry (engine.h), behind which the spread is valid */
static int blend_call(u32 n, storage_t *const *dec, const h264bsdmi_blend_spec *spec, const h264bsdmi_spread_spec *spread, void *stream,
                      u32 *kept, u32 *blended, u32 *picId)
{
    CurrentPull c;
    if (!spec || spec->shift > 7 || spec->hold > 255 || (spec->moving_shift > 7 && spec->moving_shift != H264BSDMI_BLEND_FROZEN)) return -1;
    if (!kept || keep_begin(&c, n, dec)) return -1;
    u32 *flags = (u32 *)malloc(n * sizeof(u32));
    int refused = !flags;
    for (u32 i = 0; i < n && !refused; i++) {
        const ApiDec *a = dec_of(dec[i]);
        const EngSinkEntries *entries = spread ? sink_entries(&a->hd->sink) : NULL;
        refused = spread ? !entries || !entries->blend_spread : !a->hd->sink.blend_pictures;
        if (c.pic_of[i] != NO_PIC)
            flags[c.pic_of[i]] = (has_kept_picture(a) ? 0u : ENG_SPREAD_FRESH) | (spread && !has_spread(a) ? ENG_SPREAD_UNSET : 0u);
    }
    if (refused) { free(flags); pull_free(&c); return -1; }
    const int failed = c.m && (spread ? sink_entries(c.pics[0].sink)->blend_spread(c.m, c.pics, flags, spec, spread, n, stream)
                                      : c.pics[0].sink->blend_pictures(c.m, c.pics, flags, spec, n, stream));
    if (!failed) {
        for (u32 i = 0; i < n; i++) {
            kept[i] = c.pic_of[i] != NO_PIC;
            if (blended) blended[i] = kept[i] && !(flags[c.pic_of[i]] & ENG_SPREAD_FRESH);
        }
        mark_kept(&c, 0);
        for (u32 i = 0; i < n; i++) {
            ApiDec *a = dec_of(dec[i]);
            if (spread && c.pic_of[i] != NO_PIC) a->spread_valid = 1;
            if (picId) picId[i] = has_kept_picture(a) ? a->kept_id : 0;
        }
    }
    free(flags);
    pull_free(&c);
    return failed ? -2 : 0;
}
int h264bsdmiBlendCurrentPictures(u32 n, storage_t *const *dec, const h264bsdmi_blend_spec *spec, void *stream,
                                  u32 *kept, u32 *blended, u32 *picId)
{
    if (!n) return 0;
    return blend_call(n, dec, spec, NULL, stream, kept, blended, picId);
}
/* ... and with the spread beside the kept picture: the moving test d > max(hold, V), V stepped towards gain d */
int h264bsdmiBlendCurrentPicturesSpread(u32 n, storage_t *const *dec, const h264bsdmi_blend_spec *spec, const h264bsdmi_spread_spec *spread,
                                        void *stream, u32 *kept, u32 *blended, u32 *picId)
{
    if (!n) return 0;
    if (!spread || spread->gain < 1 || spread->gain > 8 || spread->highest > 255 || spread->lowest > spread->highest ||
        spread->update > H264BSDMI_SPREAD_STILL) return -1;
    return blend_call(n, dec, spec, spread, stream, kept, blended, picId);
}

/* The kept pictures of the instances that have one, as planar I420 coded frames, and their fractions; or (spread_only) the spreads of
 * the instances that have a valid one, through the engine's kept_spread_out entry */
static int kept_out_call(u32 n, storage_t *const *dec, void *const *picture, void *const *fraction, int spread_only, void *stream,
                         u32 *got, u32 *keptPicId)
{
    if (!n) return 0;
    if (!dec || !picture || !got) return -1;
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        if (!a || !a->hd->sink.kept_pictures_out) return -1;
        if (spread_only && (!sink_entries(&a->hd->sink) || !sink_entries(&a->hd->sink)->kept_spread_out)) return -1;
        for (u32 k = 0; k < i; k++)
            if (dec[k] == dec[i]) return -1;
        if (!(spread_only ? has_spread(a) : has_kept_picture(a))) continue;
        if (!picture[i] || ((uintptr_t)picture[i] & 15u) || (fraction && ((uintptr_t)fraction[i] & 15u))) return -1;
    }
    SinkTensorPic *pics = (SinkTensorPic *)calloc(n, sizeof(SinkTensorPic));
    void **bufs = (void **)malloc(2 * (size_t)n * sizeof(void *));
    if (!pics || !bufs) { free(pics); free(bufs); return -1; }
    u32 m = 0;
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        if (!(spread_only ? has_spread(a) : has_kept_picture(a))) continue;
        pics[m].sink = &a->hd->sink;
        pics[m].index = i;
        bufs[m] = picture[i];
        bufs[n + m] = fraction ? fraction[i] : NULL;
        m++;
    }
    const int failed = m && (spread_only ? sink_entries(pics[0].sink)->kept_spread_out(m, pics, bufs, stream)
                                         : pics[0].sink->kept_pictures_out(m, pics, bufs, bufs + n, stream));
    for (u32 i = 0; !failed && i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        got[i] = (spread_only ? has_spread(a) : has_kept_picture(a)) ? 1 : 0;
        if (keptPicId) keptPicId[i] = has_kept_picture(a) ? a->kept_id : 0;
    }
    free(pics); free(bufs);
    return failed ? -2 : 0;
}
int h264bsdmiOutputKeptPictures(u32 n, storage_t *const *dec, void *const *picture, void *const *fraction, void *stream,
                                u32 *got, u32 *keptPicId)
{
    return kept_out_call(n, dec, picture, fraction, 0, stream, got, keptPicId);
}
int h264bsdmiOutputKeptSpread(u32 n, storage_t *const *dec, void *const *spread, void *stream, u32 *got, u32 *keptPicId)
{
    return kept_out_call(n, dec, spread, NULL, 1, stream, got, keptPicId);
}

/* The kept pictures of the instances that have one resampled in place through an affine map each.  The checks in the keep call's order
 * behind the spec's; then one picture per instance that is warped — its window, and under CURRENT its current picture's slot — with
 * its map beside it, through the engine's warp_kept entry (engine.h) */
static int warp_map_refused(const h264bsdmi_warp_map *m)
{
    const int top = H264BSDMI_WARP_MAX_COEFFICIENT;
    return m->a > top || m->a < -top || m->b > top || m->b < -top || m->d > top || m->d < -top || m->e > top || m->e < -top;
}
int h264bsdmiWarpKeptPictures(u32 n, storage_t *const *dec, const h264bsdmi_warp_spec *spec, void *stream, u32 *warped, u32 *keptPicId)
{
    if (!n) return 0;
    if (!spec || !spec->maps || spec->outside > H264BSDMI_WARP_CURRENT || spec->crop > 1) return -1;
    for (u32 i = 0; i < n; i++)
        if (warp_map_refused(&spec->maps[i])) return -1;
    if (!dec || !warped) return -1;
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        if (!a || !sink_pulls(a, PULL_KEEP)) return -1;
        const EngSinkEntries *entries = sink_entries(&a->hd->sink);
        if (!entries || !entries->warp_kept) return -1;
        for (u32 k = 0; k < i; k++)
            if (dec[k] == dec[i]) return -1;
    }
    SinkTensorPic *pics = (SinkTensorPic *)malloc(n * sizeof(SinkTensorPic));
    h264bsdmi_warp_map *maps = (h264bsdmi_warp_map *)malloc(n * sizeof(h264bsdmi_warp_map));
    u32 *took = (u32 *)calloc(n, sizeof(u32));
    if (!pics || !maps || !took) { free(pics); free(maps); free(took); return -1; }
    const h264bsdmi_tensor_spec window = { NULL, 1, 1, 0, 0, 0, spec->crop, 1, { 0, 0, 0 }, { 1, 1, 1 } };
    u32 m = 0;
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        const int cur = a->has_cur && a->hd->active_sps;
        if (!has_kept_picture(a) || !a->hd->active_sps || (spec->outside == H264BSDMI_WARP_CURRENT && !cur)) continue;
        tensor_pic(&pics[m], a, cur ? a->cur.slot : 0, i, &window, &REFERENCE_COLOUR);
        maps[m++] = spec->maps[i];
        took[i] = 1;
    }
    const int failed = m && sink_entries(pics[0].sink)->warp_kept(m, pics, maps, spec, n, stream);
    for (u32 i = 0; !failed && i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        warped[i] = took[i];
        if (keptPicId) keptPicId[i] = has_kept_picture(a) ? a->kept_id : 0;
    }
    free(pics); free(maps); free(took);
    return failed ? -2 : 0;
}

/* The host path of the pulls that may compare against kept pictures and may keep afterwards, behind their own spec checks:
 * h264bsdmiOutputRegionChange (PULL_CHANGE), h264bsdmiOutputRegionShift (PULL_SHIFT), h264bsdmiOutputCellMaps (PULL_CELLS) and
 * h264bsdmiOutputCellBoxes (PULL_BOXES, spec2 its boxes spec), h264bsdmiOutputCellShift (PULL_FLOW), h264bsdmiOutputPointMatches (PULL_MATCHES).  vs_kept: only instances that have a kept picture too (2: and a valid spread); max_side: the
 * longest side a region may have (0: whatever regions_refused allows); keep_after: behind the sink's entry the keep call's launch for
 * every instance with a current picture.  kept / keptPicId are what the comparison saw; -2 writes nothing, marks nothing */
static int kept_pull(int kind, int vs_kept, u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions, u32 max_side,
                     const void *spec, const void *spec2, u32 crop, u32 keep_after, void *stream,
                     u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    CurrentPull c, k;
    if (regions_refused(n, nRegions, regions, got, 1)) return -1;
    for (u32 r = 0; max_side && regions && r < nRegions; r++)
        if (regions[r].w > max_side || regions[r].h > max_side) return -1;
    if (pull_begin(&c, n, dec, nRegions, kind)) return -1;
    c.vs_kept = vs_kept != 0;       /* (pull_begin knows it of PULL_CHANGE and PULL_SHIFT; the cells have it from their mode) */
    c.vs_spread = vs_kept == 2;
    for (u32 i = 0; vs_kept && i < n; i++)
        if (!dec_of(dec[i])->hd->sink.keep_pictures) { pull_free(&c); return -1; }
    if (keep_after && keep_begin(&k, n, dec)) { pull_free(&c); return -1; }
    const h264bsdmi_tensor_spec window = { NULL, 1, 1, 0, 0, 0, crop, 1, { 0, 0, 0 }, { 1, 1, 1 } };
    pull_regions(&c, nRegions, regions, &window, &REFERENCE_COLOUR, 1, 1, 0);
    int failed = 0;
    if (c.k) {
        const JobSink *sink = c.pics[0].sink;
        switch (kind) {
        case PULL_CHANGE: failed = sink->region_change(c.m, c.pics, c.k, c.regs, (const h264bsdmi_change_spec *)spec, stream); break;
        case PULL_SHIFT:  failed = sink->region_shift(c.m, c.pics, c.k, c.regs, (const h264bsdmi_shift_spec *)spec, stream); break;
        case PULL_CELLS:  failed = sink->cell_maps(c.m, c.pics, c.k, c.regs, (const h264bsdmi_cells_spec *)spec, stream); break;
        case PULL_FLOW:   failed = sink_entries(sink)->cell_shift(c.m, c.pics, c.k, c.regs, (const h264bsdmi_cell_shift_spec *)spec, stream); break;
        case PULL_MATCHES: failed = sink_entries(sink)->point_matches(c.m, c.pics, c.k, c.regs, (const h264bsdmi_matches_spec *)spec, stream); break;
        default:          failed = sink->cell_boxes(c.m, c.pics, c.k, c.regs, (const h264bsdmi_cells_spec *)spec, (const h264bsdmi_boxes_spec *)spec2, stream);
        }
    }
    if (keep_after && !failed) failed = k.m && k.pics[0].sink->keep_pictures(k.m, k.pics, stream);
    if (!failed) {
        for (u32 i = 0; i < n; i++) {
            const ApiDec *a = dec_of(dec[i]);
            if (kept) kept[i] = has_kept_picture(a) ? 1 : 0;
            if (keptPicId) keptPicId[i] = has_kept_picture(a) ? a->kept_id : 0;
        }
        if (keep_after) mark_kept(&k, 1);
    }
    if (keep_after) pull_free(&k);
    return pull_finish(&c, failed, nRegions, got, NULL, current, picId);
}

/* Integer statistics of (current picture - kept picture) over h264bsdmiOutputRegionStats' regions */
int h264bsdmiOutputRegionChange(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                                const h264bsdmi_change_spec *spec, void *stream,
                                u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    if (!spec || !spec->data || ((uintptr_t)spec->data & 7u) || spec->source > H264BSDMI_STATS_RGB || spec->crop > 1 || spec->keep_after > 1) return -1;
    if (bins_refused(spec->bins)) return -1;
    if (spec->threshold[0] > 255 || spec->threshold[1] > 255 || spec->threshold[2] > 255) return -1;
    return kept_pull(PULL_CHANGE, 1, n, dec, nRegions, regions, 0, spec, NULL, spec->crop, spec->keep_after, stream, got, current, kept, picId, keptPicId);
}

/* Where the boxes of the kept pictures lie in the current ones */
int h264bsdmiOutputRegionShift(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                               const h264bsdmi_shift_spec *spec, void *stream,
                               u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    if (!spec || !spec->data || ((uintptr_t)spec->data & 7u) || spec->radius > H264BSDMI_SHIFT_MAX_RADIUS || spec->surface > 1 || spec->crop > 1 ||
        spec->keep_after > 1) return -1;
    return kept_pull(PULL_SHIFT, 1, n, dec, nRegions, regions, H264BSDMI_SHIFT_MAX_SIDE, spec, NULL, spec->crop, spec->keep_after, stream,
                     got, current, kept, picId, keptPicId);
}

/* Dense per-cell maps of h264bsdmiOutputRegionStats' (PICTURE) or h264bsdmiOutputRegionChange's (CHANGE) quantities over the same
 * regions: the host path of the one or of the other, the mode carried by CurrentPull.vs_kept */
static int cells_spec_refused(const h264bsdmi_cells_spec *s)
{
    const u32 allowed = s && s->mode == H264BSDMI_CELLS_SPREAD
        ? H264BSDMI_CELL_COUNT | H264BSDMI_CELL_FORE | H264BSDMI_CELL_EXCESS | H264BSDMI_CELL_SPREADSUM
        : s && s->mode == H264BSDMI_CELLS_CHANGE
        ? H264BSDMI_CELL_COUNT | H264BSDMI_CELL_SAD | H264BSDMI_CELL_SSD | H264BSDMI_CELL_DSUM | H264BSDMI_CELL_DMAX | H264BSDMI_CELL_ABOVE
        : H264BSDMI_CELL_COUNT | H264BSDMI_CELL_SUM | H264BSDMI_CELL_SUMSQ | H264BSDMI_CELL_MIN | H264BSDMI_CELL_MAX;
    if (!s || !s->data || ((uintptr_t)s->data & 3u)) return 1;
    if (!s->cols || s->cols > 4096u || !s->rows || s->rows > 4096u) return 1;
    if (s->cell != 4 && s->cell != 8 && s->cell != 16 && s->cell != 32 && s->cell != 64) return 1;
    if (s->source > H264BSDMI_STATS_RGB || s->crop > 1 || s->mode > H264BSDMI_CELLS_SPREAD || s->keep_after > 1) return 1;
    if (s->mode == H264BSDMI_CELLS_SPREAD && (s->source == H264BSDMI_STATS_RGB || s->keep_after)) return 1;     /* (a plain keep would invalidate what was just read) */
    if (!s->planes || (s->planes & ~allowed)) return 1;
    if (s->threshold[0] > 255 || s->threshold[1] > 255 || s->threshold[2] > 255) return 1;
    if (s->mode == H264BSDMI_CELLS_PICTURE && (s->threshold[0] || s->threshold[1] || s->threshold[2] || s->keep_after)) return 1;
    return 0;
}
/* The boxes spec against the cells spec it labels a map of (which has passed cells_spec_refused) */
static int boxes_spec_refused(const h264bsdmi_cells_spec *c, const h264bsdmi_boxes_spec *b)
{
    if (!b || !b->data || ((uintptr_t)b->data & 3u)) return 1;
    if (!b->max_boxes || b->max_boxes > H264BSDMI_BOXES_MAX_BOXES) return 1;
    if (!b->plane || (b->plane & (b->plane - 1u)) || !(b->plane & c->planes)) return 1;
    if (c->mode == H264BSDMI_CELLS_CHANGE && b->plane == H264BSDMI_CELL_DSUM) return 1;
    if (b->channel >= (b->plane == H264BSDMI_CELL_COUNT || c->source == H264BSDMI_STATS_Y ? 1u : 3u)) return 1;
    if (b->sense > H264BSDMI_BOXES_BELOW || (b->connectivity != 4 && b->connectivity != 8) || !b->min_cells) return 1;
    return c->rows * c->cols > H264BSDMI_BOXES_MAX_CELLS;                   /* (4096 each at the most: no overflow) */
}
/* The host path of both is kept_pull's: kind PULL_CELLS calls the sink's cell_maps, PULL_BOXES its cell_boxes with the boxes spec */
static int cells_pull(int kind, u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                      const h264bsdmi_cells_spec *spec, const h264bsdmi_boxes_spec *boxes, void *stream,
                      u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    if (cells_spec_refused(spec) || (kind == PULL_BOXES && boxes_spec_refused(spec, boxes))) return -1;
    /* SPREAD: CHANGE's path, for the instances that have a valid spread too (vs_kept 2), on an engine that has the spread entries */
    for (u32 i = 0; spec->mode == H264BSDMI_CELLS_SPREAD && dec && i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        if (a && (!sink_entries(&a->hd->sink) || !sink_entries(&a->hd->sink)->blend_spread)) return -1;
    }
    return kept_pull(kind, spec->mode == H264BSDMI_CELLS_SPREAD ? 2 : spec->mode == H264BSDMI_CELLS_CHANGE, n, dec, nRegions, regions, 0, spec, boxes, spec->crop, spec->keep_after, stream,
                     got, current, kept, picId, keptPicId);
}
int h264bsdmiOutputCellMaps(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                            const h264bsdmi_cells_spec *spec, void *stream,
                            u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    return cells_pull(PULL_CELLS, n, dec, nRegions, regions, spec, NULL, stream, got, current, kept, picId, keptPicId);
}
/* The cell maps, and behind them the boxes of the connected groups of cells that pass a level */
int h264bsdmiOutputCellBoxes(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                             const h264bsdmi_cells_spec *cells, const h264bsdmi_boxes_spec *boxes, void *stream,
                             u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    return cells_pull(PULL_BOXES, n, dec, nRegions, regions, cells, boxes, stream, got, current, kept, picId, keptPicId);
}

/* Per cell of a grid where it went: h264bsdmiOutputCellMaps' regions and grid in CHANGE mode, h264bsdmiOutputRegionShift's search */
static int cell_shift_spec_refused(const h264bsdmi_cell_shift_spec *s)
{
    const u32 allowed = H264BSDMI_FLOW_COUNT | H264BSDMI_FLOW_DX | H264BSDMI_FLOW_DY | H264BSDMI_FLOW_BEST | H264BSDMI_FLOW_STILL | H264BSDMI_FLOW_TIES;
    if (!s || !s->data || ((uintptr_t)s->data & 3u)) return 1;
    if (!s->cols || s->cols > 4096u || !s->rows || s->rows > 4096u) return 1;
    if (s->cell != 8 && s->cell != 16 && s->cell != 32 && s->cell != 64) return 1;
    if (s->radius > H264BSDMI_SHIFT_MAX_RADIUS || s->crop > 1 || s->keep_after > 1) return 1;
    return !s->planes || (s->planes & ~allowed);
}
int h264bsdmiOutputCellShift(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                             const h264bsdmi_cell_shift_spec *spec, void *stream,
                             u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    if (cell_shift_spec_refused(spec)) return -1;
    return kept_pull(PULL_FLOW, 1, n, dec, nRegions, regions, 0, spec, NULL, spec->crop, spec->keep_after, stream, got, current, kept, picId, keptPicId);
}

/* Where the points of the kept pictures lie in the current ones, at any distance: binary descriptors and their Hamming matching over
 * h264bsdmiOutputRegionShift's regions.  The pattern of the descriptor is descriptor_pattern.h's, the kernel's copy of the same numbers */
const signed char *h264bsdmiDescriptorPattern(void)
{
    static const signed char pattern[4 * DESCRIPTOR_TESTS] = { DESCRIPTOR_PATTERN_VALUES };
    return pattern;
}
static int matches_spec_refused(const h264bsdmi_matches_spec *s)
{
    if (!s || !s->data || ((uintptr_t)s->data & 7u) || !s->kept_points || ((uintptr_t)s->kept_points & 7u) ||
        !s->current_points || ((uintptr_t)s->current_points & 7u)) return 1;
    if (s->max_points < 1 || s->max_points > H264BSDMI_MATCHES_MAX_POINTS || s->max_distance > 256 || s->ratio < 1 || s->ratio > 256) return 1;
    return s->max_move > 65535 || s->mutual_only > 1 || s->crop > 1 || s->keep_after > 1 || s->zero;
}
int h264bsdmiOutputPointMatches(u32 n, storage_t *const *dec, u32 nRegions, const h264bsdmi_region *regions,
                                const h264bsdmi_matches_spec *spec, void *stream,
                                u32 *got, u32 *current, u32 *kept, u32 *picId, u32 *keptPicId)
{
    if (matches_spec_refused(spec)) return -1;
    return kept_pull(PULL_MATCHES, 1, n, dec, nRegions, regions, H264BSDMI_SHIFT_MAX_SIDE, spec, NULL, spec->crop, spec->keep_after, stream,
                     got, current, kept, picId, keptPicId);
}

/* Which motion the point matches agree on: the consensus fit of h264bsdmiOutputPointMatches' records.  The one call here without
 * pictures: the instances only name the device, so none of the pull steps applies — the spec, then the instances (each on a sink of the
 * engine with the entry, distinct, one device), then the entry of instance 0's sink with that sink */
static int model_spec_refused(const h264bsdmi_model_spec *s)
{
    if (!s || !s->data || ((uintptr_t)s->data & 7u) || !s->matches || ((uintptr_t)s->matches & 7u) || !s->kept_points ||
        ((uintptr_t)s->kept_points & 7u) || !s->current_points || ((uintptr_t)s->current_points & 7u)) return 1;
    if (s->max_points < 1 || s->max_points > H264BSDMI_MODEL_MAX_POINTS || s->model > H264BSDMI_MODEL_SIMILARITY || s->tolerance > 255) return 1;
    if (s->model == H264BSDMI_MODEL_SIMILARITY ? s->max_scale && (s->max_scale < 256 || s->max_scale > 4096) : s->max_scale != 0) return 1;
    return s->min_inliers < 1 + s->model || s->min_inliers > 256 || s->zero[0] || s->zero[1] || s->zero[2];
}
int h264bsdmiOutputPointModel(u32 n, storage_t *const *dec, u32 nRecords, const h264bsdmi_model_spec *spec, void *stream)
{
    if (model_spec_refused(spec) || nRecords > 65535u || (n && !dec) || (!n && nRecords)) return -1;
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(dec[i]);
        if (!a || a->hd->sink.configure == cap_configure) return -1;           /* capture mode: there is no device */
        const EngSinkEntries *entries = sink_entries(&a->hd->sink);
        if (!entries || !entries->point_model) return -1;
        if (eng_sink_device(&a->hd->sink) != eng_sink_device(&dec_of(dec[0])->hd->sink)) return -1;
        for (u32 k = 0; k < i; k++)
            if (dec[k] == dec[i]) return -1;
    }
    if (!nRecords) return 0;
    const JobSink *sink = &dec_of(dec[0])->hd->sink;
    return sink_entries(sink)->point_model(sink, nRecords, spec, stream) ? -2 : 0;
}

static u32 *next_converted(storage_t *s, u32 *picId, u32 *isIdrPic, u32 *numErrMbs, int fmt)
{
    ApiDec *a = dec_of(s);
    if (!a) return NULL;
    const OutPic *o = pop_output(a, picId, isIdrPic, numErrMbs);
    if (!o || !a->hd->sink.fetch_converted) return NULL;
    return a->hd->sink.fetch_converted(a->hd->sink.user, o->slot, fmt);
}
u32 *h264bsdNextOutputPictureRGBA(storage_t *s, u32 *p, u32 *i, u32 *n) { return next_converted(s, p, i, n, 0); }
u32 *h264bsdNextOutputPictureBGRA(storage_t *s, u32 *p, u32 *i, u32 *n) { return next_converted(s, p, i, n, 1); }
u32 *h264bsdNextOutputPictureYCbCrA(storage_t *s, u32 *p, u32 *i, u32 *n) { return next_converted(s, p, i, n, 2); }

static const Sps *active_sps(storage_t *s)
{
    ApiDec *a = dec_of(s);
    return a ? a->hd->active_sps : NULL;
}

u32 h264bsdPicWidth(storage_t *s) { const Sps *p = active_sps(s); return p ? p->width_mbs : 0; }
u32 h264bsdPicHeight(storage_t *s) { const Sps *p = active_sps(s); return p ? p->height_mbs : 0; }
u32 h264bsdProfile(storage_t *s) { const Sps *p = active_sps(s); return p ? p->profile_idc : 0; }

u32 h264bsdVideoRange(storage_t *s) { return sps_full_range(active_sps(s)) ? 1 : 0; }
u32 h264bsdMatrixCoefficients(storage_t *s) { return sps_matrix_coefficients(active_sps(s)); }

void h264bsdCroppingParams(storage_t *s, u32 *croppingFlag, u32 *left, u32 *width, u32 *top, u32 *height)
{
    const Sps *p = active_sps(s);
    if (p && p->cropping) {
        *croppingFlag = 1;
        sps_window(p, 1, left, top, width, height);
    } else {
        *croppingFlag = 0;
        *left = *width = *top = *height = 0;
    }
}

void h264bsdSampleAspectRatio(storage_t *s, u32 *sarWidth, u32 *sarHeight)
{
    /* Table E-1 */
    static const u8 sar[14][2] = { { 0, 0 }, { 1, 1 }, { 12, 11 }, { 10, 11 }, { 16, 11 }, { 40, 33 }, { 24, 11 },
        { 20, 11 }, { 32, 11 }, { 80, 33 }, { 18, 11 }, { 15, 11 }, { 64, 33 }, { 160, 99 } };
    const Sps *p = active_sps(s);
    u32 w = 1, h = 1;
    if (p && p->vui_present && p->aspect_ratio_present) {
        if (p->aspect_ratio_idc < 14) { w = sar[p->aspect_ratio_idc][0]; h = sar[p->aspect_ratio_idc][1]; }
        else if (p->aspect_ratio_idc == 255) {
            w = p->sar_width; h = p->sar_height;
            if (!w || !h) w = h = 0;
        } else w = h = 0;
    }
    *sarWidth = w;
    *sarHeight = h;
}

/* 1 when at least one PPS with its SPS is stored and consistent (reference storage.c:793-829) */
u32 h264bsdCheckValidParamSets(storage_t *s)
{
    ApiDec *a = dec_of(s);
    if (!a) return 0;
    for (int i = 0; i < HD_MAX_PPS; i++) {
        const Pps *p = a->hd->pps[i];
        if (p && a->hd->sps[p->sps_id] && !hd_check_pps(p, a->hd->sps[p->sps_id])) return 1;     /* h264bsdValidParamSets, storage.c:863-885 */
    }
    return 0;
}

void h264bsdFlushBuffer(storage_t *s)
{
    ApiDec *a = dec_of(s);
    drop_current(a);
    if (a) hd_dpb_flush(&a->hd->dpb);
}

/* test/tooling hook: complete a hand-built frame job (see fj_finalize, hd_core.c) */
int h264bsdmiJobFinalize(u8 *job, u32 capacity, u32 n_coef_blocks)
{
    /* a hand-built job carries no FJ_CODED_WIDE flags (the parser sets them while it sums up the levels): derive them from
     * the coefficient blocks, with the parser's own bound */
    FjHeader *h = (FjHeader *)job;
    if (capacity >= sizeof(FjHeader) && (size_t)h->rec_off + (size_t)h->n_mbs * sizeof(FjMbRec) <= capacity) {
        FjMbRec *recs = (FjMbRec *)(job + h->rec_off);
        for (u32 a = 0; a < h->n_mbs; a++) {
            FjMbRec *r = &recs[a];
            r->coded &= ~FJ_CODED_WIDE;
            if (r->kind != FJ_MB_INTER || !(r->coded & 0x02FFFFFFu)) continue;
            const u32 n_l = (u32)__builtin_popcount(r->coded & 0xFFFFu), n_c = (u32)__builtin_popcount((r->coded >> 16) & 0xFFu);
            const u32 has_cdc = (r->coded & FJ_CODED_CHROMA_DC) ? 1u : 0u;
            if ((size_t)h->coef_off + ((size_t)r->coef_idx + n_l + has_cdc + n_c) * 32u > capacity) continue;      /* (fj_finalize rejects the job) */
            const int16_t *p = (const int16_t *)(job + h->coef_off) + 16u * (size_t)r->coef_idx;
            u32 sl = 0, sd = 0, sc = 0;                 /* the largest block's sum of each kind, like the parser's (hd_mb.c parse_residual) */
            for (u32 b = 0; b < n_l; b++, p += 16) { u32 t = 0; for (int i = 0; i < 16; i++) t += (u32)abs(p[i]); if (t > sl) sl = t; }
            if (has_cdc) {
                u32 t0 = 0, t1 = 0;
                for (int i = 0; i < 4; i++) { t0 += (u32)abs(p[i]); t1 += (u32)abs(p[4 + i]); }
                sd = t0 > t1 ? t0 : t1;
                p += 16;
            }
            for (u32 b = 0; b < n_c; b++, p += 16) { u32 t = 0; for (int i = 0; i < 16; i++) t += (u32)abs(p[i]); if (t > sc) sc = t; }
            if (!hd_residual_bound_ok(sl, sd, sc, r->qp_y, r->qp_c)) r->coded |= FJ_CODED_WIDE;
        }
    }
    return fj_finalize(job, capacity, n_coef_blocks);
}

void h264bsdConvertToRGBA(u32 width, u32 height, u8 *data, u32 *pOutput) { eng_convert_host(0, width, height, data, pOutput); }
void h264bsdConvertToBGRA(u32 width, u32 height, u8 *data, u32 *pOutput) { eng_convert_host(1, width, height, data, pOutput); }
void h264bsdConvertToYCbCrA(u32 width, u32 height, u8 *data, u32 *pOutput) { eng_convert_host(2, width, height, data, pOutput); }

/* ================================================================== host parse pipeline */
u32 h264bsdmiDecodePicture(storage_t *s, u8 *buf, u32 len, u32 picId, u32 *consumed, u32 *nErrors)
{
    u32 off = 0, last = H264BSD_RDY, errs = 0, stalls = 0;
    drop_current(dec_of(s));
    while (off < len) {
        u32 rb = 0;
        last = h264bsdDecode(s, buf + off, len - off, picId, &rb);
        off += rb;
        if (last == H264BSD_PIC_RDY) break;
        if (last >= H264BSD_ERROR) errs++;
        stalls = rb ? 0 : stalls + 1;              /* HDRS_RDY and friends repeat the same NAL once; never spin */
        if (stalls > 3) break;
    }
    if (consumed) *consumed = off;
    if (nErrors) *nErrors = errs;
    return last == H264BSD_PIC_RDY ? last : (u32)H264BSD_RDY;
}

/* A small persistent pool: workers sleep on a condition variable, a batch is an index range handed out by an atomic
 * counter (pictures differ a lot in parse time: I pictures cost several times a P picture).
 * One process may drive several GPUs (h264bsdmiSetDevice per thread): the workers are then split into one group per
 * device in use, a worker first takes the pictures of decoder instances that live on ITS device, and (H264BSDMI_PIN=2,
 * the default) is pinned to the CPUs of that device's NUMA node (eng_device_cpus: /sys/bus/pci/devices/<gpu>/
 * local_cpulist), so that the frame job it builds in pinned staging memory and the parser state it touches sit next to
 * the GPU they feed.  H264BSDMI_PIN=1: spread over all CPUs; 0: no pinning. */
typedef struct Batch {
    u32 n;
    storage_t *const *dec;
    u8 *const *buf;
    const u32 *len, *pic_id;
    u32 *status, *consumed, *n_errors;
    u8 **out;                               /* non-NULL: item i pulls first — h264bsdNextOutputPicture(dec[i]) -> out[i], out_id[i], out_idr[i], out_nerr[i] */
    u32 *out_id, *out_idr, *out_nerr;       /* (each may be NULL) */
    atomic_uchar *taken;                    /* one flag per item */
    unsigned char *began;                   /* per item, touched by the worker that took it only: its picture is on its way (item_pull_begin) */
    int active;                             /* pool threads currently inside this batch (guarded by g_pool.mu) */
    signed char *item_dev;                  /* device of every item's decoder instance (-1: capture mode) */
    int devs[16], n_devs;                   /* the devices in use in this batch */
    u32 workers;                            /* threads that work on this batch (run_batch): all of the pool, or fewer when the batch pulls */
    atomic_int pull_failed;                 /* a picture was popped from an instance's output queue and could not be fetched (HIP failure): the batch returns -1 */
} Batch;

static struct {
    pthread_mutex_t mu;
    pthread_cond_t wake, idle;
    pthread_t th[64];
    int n_threads, started, want, pin;
    int pull_workers;                       /* threads a batch that pulls pictures runs on (run_batch): the CPUs the process may have running at once — or
                                               all of the pool when the application (or H264BSDMI_THREADS) named the number of threads */
    unsigned generation;
    Batch *batch;
    pthread_mutex_t api_mu;                 /* one batch at a time */
} g_pool = { PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, PTHREAD_COND_INITIALIZER, { 0 }, 0, 0, 0, 0, 0, 0, NULL,
             PTHREAD_MUTEX_INITIALIZER };

/* An item of a batch that pulls (b->out) runs in two steps: item_pull_begin pops the instance's output queue and starts the picture on
 * its way to host memory, item_finish waits for it and — if the batch decodes as well (b->buf) — parses the instance's next picture.  A
 * worker begins its NEXT item before it finishes the current one (batch_take): while it parses, the next picture crosses the link, and
 * its wait finds the picture there (8.5 -> 8.8 k fps with 256 instances and 20 threads; DESIGN.md §5 has the whole account of the
 * host-output path, including what is still unexplained about it: a round gets LONGER with more pool threads). */
static void item_pull_begin(Batch *b, u32 i)
{
    ApiDec *a = dec_of(b->dec[i]);
    u32 id = 0, idr = 0, nerr = 0;
    const OutPic *o = a ? pop_output(a, &id, &idr, &nerr) : NULL;
    b->out[i] = NULL;
    if (b->out_id) b->out_id[i] = id;
    if (b->out_idr) b->out_idr[i] = idr;
    if (b->out_nerr) b->out_nerr[i] = nerr;
    if (!o) return;
    const JobSink *k = &a->hd->sink;
    if (k->fetch_begin && k->fetch_end) {
        if (k->fetch_begin(k->user, o->slot) == 0) b->began[i] = 1;        /* on its way: item_finish collects it */
        else atomic_store(&b->pull_failed, 1);
    } else if (k->fetch) {
        b->out[i] = k->fetch(k->user, o->slot);
        if (!b->out[i]) atomic_store(&b->pull_failed, 1);
    }
}

static void item_finish(Batch *b, u32 i)
{
    if (b->out) {
        const ApiDec *a = dec_of(b->dec[i]);
        if (b->began[i]) {
            b->out[i] = a->hd->sink.fetch_end(a->hd->sink.user);
            if (!b->out[i]) atomic_store(&b->pull_failed, 1);
        }
        if (!b->buf) return;
        /* pull AND decode: the reference's decoder drops what is still waiting in its output queue when the next slice arrives
         * (src/h264bsd_dpb.c:1260-1261), so an instance with more pictures to give is not fed — the caller comes back for them */
        if (a && a->hd->dpb.out_idx < a->hd->dpb.n_out) {
            b->status[i] = H264BSD_RDY; b->consumed[i] = 0;
            if (b->n_errors) b->n_errors[i] = 0;
            return;
        }
    }
    b->status[i] = h264bsdmiDecodePicture(b->dec[i], b->buf[i], b->len[i], b->pic_id ? b->pic_id[i] : 0,
                                          &b->consumed[i], b->n_errors ? &b->n_errors[i] : NULL);
}

/* item i has just been claimed by this worker; *held = the item it began before and has not finished (-1: none) */
static void batch_take(Batch *b, u32 i, int *held)
{
    if (!b->out) { item_finish(b, i); return; }
    item_pull_begin(b, i);
    if (*held >= 0) item_finish(b, (u32)*held);
    *held = (int)i;
}

/* Worker `me` of `nw`: group g = me % n_devs serves device devs[g].  It takes the items of its device i = k, k + gs,
 * ... (k = its index in the group, gs = group size) first — so that a stream is normally parsed by the same thread,
 * from the same NUMA node, every round — then whatever else is left anywhere. */
static void batch_work(Batch *b, u32 me, u32 nw)
{
    const u32 nd = b->n_devs > 0 ? (u32)b->n_devs : 1u;
    const u32 g = me % nd, k = me / nd, gs = (nw - g + nd - 1) / nd;
    const int my_dev = b->n_devs > 0 ? b->devs[g] : -1;
    u32 seen = 0;
    int held = -1;
    for (u32 i = 0; i < b->n; i++) {
        if (b->n_devs > 0 && b->item_dev[i] != my_dev) continue;
        if (seen++ % gs == k && !atomic_exchange(&b->taken[i], 1)) batch_take(b, i, &held);
    }
    for (int pass = 0; pass < 2; pass++)        /* leftovers: own device first */
        for (u32 i = 0; i < b->n; i++) {
            if (pass == 0 && b->n_devs > 0 && b->item_dev[i] != my_dev) continue;
            if (!atomic_load(&b->taken[i]) && !atomic_exchange(&b->taken[i], 1)) batch_take(b, i, &held);
        }
    if (held >= 0) item_finish(b, (u32)held);
}

static void pin_worker(u32 me, int device, int *pinned_to)
{
    if (g_pool.pin == 1 && *pinned_to != -2) {
        /* spread the workers over the CPUs (worker k -> CPU k * ncpu / nthreads) */
        const long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
        cpu_set_t set;
        CPU_ZERO(&set);
        CPU_SET((int)(((long)me * ncpu) / (g_pool.want > 0 ? g_pool.want : 1)) % (int)ncpu, &set);
        pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
        *pinned_to = -2;
    } else if (g_pool.pin == 2 && device >= 0 && *pinned_to != device) {
        int cpus[1024];
        const int n = eng_device_cpus(device, cpus, 1024);
        if (n > 0) {
            /* only CPUs this process may run on (a cpuset-restricted container may not own the GPU's node at all: then the
             * worker stays where the scheduler puts it) */
            cpu_set_t set, allowed;
            CPU_ZERO(&set);
            int usable = 0;
            if (sched_getaffinity(0, sizeof(allowed), &allowed) == 0) {
                for (int i = 0; i < n; i++) if (cpus[i] < CPU_SETSIZE && CPU_ISSET(cpus[i], &allowed)) { CPU_SET(cpus[i], &set); usable++; }
            }
            if (usable > 0) pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
        }
        *pinned_to = device;
    }
}

static void *pool_main(void *arg)
{
    const u32 me = (u32)(size_t)arg;        /* 1.. ; the caller's thread is worker 0 (never pinned: it is the application's) */
    int pinned_to = -1;
    unsigned seen = 0;
    pthread_mutex_lock(&g_pool.mu);
    for (;;) {
        while (g_pool.generation == seen) pthread_cond_wait(&g_pool.wake, &g_pool.mu);
        seen = g_pool.generation;
        Batch *b = g_pool.batch;
        if (!b) continue;
        b->active++;
        const u32 nw = b->workers;
        pthread_mutex_unlock(&g_pool.mu);
        if (me < nw) {
            pin_worker(me, b->n_devs > 0 ? b->devs[me % (u32)b->n_devs] : -1, &pinned_to);
            batch_work(b, me, nw);
        }
        pthread_mutex_lock(&g_pool.mu);
        if (--b->active == 0) pthread_cond_broadcast(&g_pool.idle);
    }
    return NULL;
}

/* CPUs this process may really use: the online count, cut down by the affinity mask and by a cgroup CPU quota
 * (containers: /sys/fs/cgroup/cpu.max, or cpu.cfs_quota_us / cpu.cfs_period_us under cgroup v1).  Parser threads
 * beyond that only take turns: on a box with 256 hardware threads and a quota of 16 CPUs, 64 threads parse 24 % fewer
 * pictures per second than 16. */
static long usable_cpus_q(int quota_bonus)
{
    long n = sysconf(_SC_NPROCESSORS_ONLN);
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0 && CPU_COUNT(&set) < n) n = CPU_COUNT(&set);
    long long quota = -1, period = 0;
    FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        char q[32] = "";
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"))) {
        if (fscanf(f, "%lld", &quota) != 1) quota = -1;
        fclose(f);
        if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r"))) { if (fscanf(f, "%lld", &period) != 1) period = 0; fclose(f); }
    }
    if (quota > 0 && period > 0) {
        /* A quota is CPU time per period, not a set of cores: with exactly `quota` threads the budget is not used up (the
         * thread that enqueues the device work between two rounds is not parsing, threads wait for each other at the end
         * of a round).  A quarter more threads than CPUs of quota measured best on the GPU box (256 hardware threads, quota
         * 16: 16 / 20 / 24 / 28 / 32 threads -> 17.5 / 18.7 / 16.8 / 16.9 / 16.0 k pictures per second end to end). */
        const long q = (long)((quota + period - 1) / period), q125 = q + q / 4;
        if (q >= 1 && q < n) n = !quota_bonus ? q : q125 < n ? q125 : n;
    }
    return n < 1 ? 1 : n;
}
static long usable_cpus(void) { return usable_cpus_q(1); }

/* Processes that share this host's CPUs, one per GPU (the usual multi-GPU launch): every one of them sizes its
 * parser pool for ITS share of the CPUs the container may use — eight ranks that each start usable_cpus() threads only take
 * turns.  H264BSDMI_HOST_SHARE says how many; without it the launcher's LOCAL_WORLD_SIZE (torch.distributed.run, mpirun
 * wrappers) is taken. */
static long host_share(void)
{
    const char *e = getenv("H264BSDMI_HOST_SHARE");
    int from_launcher = 0;
    if (!e || !*e) {
        /* The launcher's LOCAL_WORLD_SIZE only says that N processes run on this host — not that they share CPUs.  Where the launcher
         * (SLURM / mpirun binding, numactl or a cgroup per rank) has already given this process its own CPUs, usable_cpus() IS the
         * share, and dividing again would leave a CPU-bound pipeline with 1 / N of its threads.  The fallback therefore applies
         * only while the process's affinity mask is the whole host.  A cgroup CPU quota does not count as a partition:
         * a container's quota is normally shared by all the ranks started inside it (the GPU boxes of this project: 256 hardware
         * threads online, quota 16 for the container) — a launcher that gives every rank its own cgroup sets H264BSDMI_HOST_SHARE=1. */
        e = getenv("LOCAL_WORLD_SIZE");
        const long online = sysconf(_SC_NPROCESSORS_ONLN);
        cpu_set_t set;
        if (e && online > 0 && sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0 && CPU_COUNT(&set) < online) e = NULL;
        from_launcher = e != NULL;
    }
    long n = e ? atol(e) : 1;
    n = n < 1 ? 1 : n > 64 ? 64 : n;
    static int said;
    if (from_launcher && n > 1 && !said) {
        said = 1;
        fprintf(stderr, "h264bsd-mi355x: parser pool sized for 1 / %ld of this host's CPUs (LOCAL_WORLD_SIZE=%ld; H264BSDMI_HOST_SHARE or H264BSDMI_THREADS override)\n", n, n);
    }
    return n;
}

static int pool_default_threads(void)
{
    const char *e = getenv("H264BSDMI_THREADS");
    long n = e ? atol(e) : (usable_cpus() + host_share() - 1) / host_share();
    if (n < 1) n = 1;
    if (n > 64) n = 64;
    return (int)n;
}

int h264bsdmiSetParserThreads(int n)
{
    pthread_mutex_lock(&g_pool.mu);
    const int chosen = n >= 1 || getenv("H264BSDMI_THREADS") != NULL;
    if (n < 1) n = pool_default_threads();
    if (n > 64) n = 64;
    g_pool.want = n;
    g_pool.pin = getenv("H264BSDMI_PIN") ? atoi(getenv("H264BSDMI_PIN")) : 2;
    /* the caller's thread works too: n threads in total = n-1 pool threads (threads are only ever added) */
    while (g_pool.started < n - 1) {
        if (pthread_create(&g_pool.th[g_pool.started], NULL, pool_main, (void *)(size_t)(g_pool.started + 1))) break;
        pthread_detach(g_pool.th[g_pool.started]);
        g_pool.started++;
    }
    g_pool.n_threads = g_pool.started + 1;
    {
        const long lim = (usable_cpus_q(0) + host_share() - 1) / host_share();
        g_pool.pull_workers = chosen || lim < 1 || lim > g_pool.n_threads ? g_pool.n_threads : (int)lim;
    }
    const int r = g_pool.n_threads;
    pthread_mutex_unlock(&g_pool.mu);
    return r;
}

static int run_batch(Batch *b)
{
    const u32 n = b->n;
    pthread_mutex_lock(&g_pool.api_mu);
    if (!g_pool.n_threads) h264bsdmiSetParserThreads(0);
    atomic_uchar *taken = (atomic_uchar *)calloc(n, sizeof(atomic_uchar));
    unsigned char *began = (unsigned char *)calloc(n, 1);
    signed char *item_dev = (signed char *)malloc(n);
    if (!taken || !began || !item_dev) { free(taken); free(began); free(item_dev); pthread_mutex_unlock(&g_pool.api_mu); return -1; }
    b->taken = taken; b->began = began; b->item_dev = item_dev; b->active = 0; b->n_devs = 0;
    atomic_store(&b->pull_failed, 0);
    for (u32 i = 0; i < n; i++) {
        const ApiDec *a = dec_of(b->dec[i]);
        const int dv = a && a->hd ? eng_sink_device(&a->hd->sink) : -1;
        item_dev[i] = (signed char)dv;
        int known = dv < 0;
        for (int k = 0; k < b->n_devs && !known; k++) known = b->devs[k] == dv;
        if (!known && b->n_devs < 16) b->devs[b->n_devs++] = dv;
    }
    pthread_mutex_lock(&g_pool.mu);
    /* A batch that pulls pictures runs on no more threads than the process may have running at once.  The pool is a quarter larger than a
     * CPU quota (usable_cpus_q: that uses the budget up when threads only parse); threads that also wait for the device in between burn a
     * period's budget in bursts, and while the cgroup is throttled nothing feeds the link: 256 pulls + parses take 26.5 ms on 16 threads,
     * 29.5 on 20, 52 on 40 under a quota of 16 CPUs. */
    const u32 nw = (u32)(b->out ? g_pool.pull_workers : g_pool.n_threads);
    b->workers = nw;
    g_pool.batch = b;
    g_pool.generation++;
    pthread_cond_broadcast(&g_pool.wake);
    pthread_mutex_unlock(&g_pool.mu);
    batch_work(b, 0, nw);
    pthread_mutex_lock(&g_pool.mu);
    g_pool.batch = NULL;                    /* late wakers find nothing; those inside are counted in b.active */
    while (b->active) pthread_cond_wait(&g_pool.idle, &g_pool.mu);
    pthread_mutex_unlock(&g_pool.mu);
    free(taken);
    free(began);
    free(item_dev);
    pthread_mutex_unlock(&g_pool.api_mu);
    return atomic_load(&b->pull_failed) ? -1 : 0;      /* -1: a picture left an output queue and could not be fetched (its out[] entry is NULL) */
}

int h264bsdmiDecodePictureBatch(u32 n, storage_t *const *dec, u8 *const *buf, const u32 *len, const u32 *picId,
                                u32 *status, u32 *consumed, u32 *nErrors)
{
    if (!dec || !buf || !len || !status || !consumed) return -1;
    if (!n) return 0;
    Batch b = { n, dec, buf, len, picId, status, consumed, nErrors, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, { 0 }, 0, 0, 0 };
    return run_batch(&b);
}

/* h264bsdNextOutputPicture() of n decoder instances at once, on the parser pool's threads: every thread enqueues its pictures'
 * way out (layout kernel + copy to pinned host memory) and waits for ITS copies only, so the transfers of the instances overlap
 * each other and the device's remaining work.  pictures[i] = NULL when instance i has no picture to give. */
int h264bsdmiNextOutputPictureBatch(u32 n, storage_t *const *dec, u8 **pictures, u32 *picId, u32 *isIdrPic, u32 *numErrMbs)
{
    if (!dec || !pictures) return -1;
    if (!n) return 0;
    Batch b = { n, dec, NULL, NULL, NULL, NULL, NULL, NULL, pictures, picId, isIdrPic, numErrMbs, NULL, NULL, 0, NULL, { 0 }, 0, 0, 0 };
    return run_batch(&b);
}

/* One round of the reference's per-stream loop (posix/test_h264bsd.c:146-177: pull what is ready, then decode on) for n instances
 * at once: every pool thread pulls ITS instance's next picture and then parses that instance's next picture, so the transfers of
 * some instances run beside the parsing of others — with h264bsdmiNextOutputPictureBatch + h264bsdmiDecodePictureBatch the
 * CPUs idle while the pictures cross the link and the link idles while the CPUs parse. */
int h264bsdmiPullAndDecodePictureBatch(u32 n, storage_t *const *dec, u8 **pictures, u32 *outPicId, u32 *outIsIdrPic, u32 *outNumErrMbs,
                                       u8 *const *buf, const u32 *len, const u32 *picId, u32 *status, u32 *consumed, u32 *nErrors)
{
    if (!dec || !pictures || !buf || !len || !status || !consumed) return -1;
    if (!n) return 0;
    Batch b = { n, dec, buf, len, picId, status, consumed, nErrors, pictures, outPicId, outIsIdrPic, outNumErrMbs, NULL, NULL, 0, NULL, { 0 }, 0, 0, 0 };
    return run_batch(&b);
}
