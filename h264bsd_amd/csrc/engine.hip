/*
 * engine.hip — host side of the HIP engine: device context, per-decoder DPB in HBM (macroblock tiles,
 * kernels.hip.h), lazy batched execution of queued frame jobs ("ticks").  The HBM-resident replay sets used by bench.py and
 * the kernel tests (the bench library's include/h264bsd_mi355x_bench.h) are replay.hip.h, included at the end.
 *
 * Execution model.  A tick holds at most one picture per stream (pictures of one stream depend on each other
 * through the DPB; pictures of different streams never do).  A tick of N pictures is SIX launches (launch_tick):
 *     k_copy            grid (32, N)          x 256  whole-sample copy macroblocks, one run of <= 8 tiles per wavefront; on a HIP stream of its own
 *                                                    next to the inter kernels (single-lane engine and replay sets: SideLane), joined before k_frame_intra
 *     k_recon_inter_lb  grid (n_uni/32, N)    x 64   inter macroblocks with one motion vector: a chunk of 32 list entries per wavefront, binned by
 *                                                    interpolation class, four macroblocks at a time, a 4x4 block per lane
 *     k_recon_inter_lq  grid (n_quad/8, N)    x 64   inter macroblocks with one motion vector per 8x8 quadrant: a chunk of 8 list entries per wavefront, their quadrants
 *                                                    binned by interpolation class, 16 quadrants at a time, a 4x4 block per lane
 *     k_recon_inter     grid (n_rest, N)      x 64   inter macroblocks with finer partitions, one list entry per wavefront (launched when a picture has any)
 *     k_dbk             grid (n_dbk/512, N)   x 512  boundary strengths from metadata, one macroblock per lane; on a third HIP stream, next to the four above, joined before k_frame_dbk
 *     k_frame_intra     grid (N)              x 768  one workgroup per picture: intra macroblocks, dataflow-scheduled in LDS
 *     k_frame_dbk       grid (N)              x 768  one workgroup per picture: in-loop filter, dataflow-scheduled in LDS
 * Occupancy of the two per-picture kernels comes from batching streams: 256 pictures = one workgroup per CU.
 * Which pictures share a tick, and on which HIP stream a tick runs, is the lane scheduler's business (Lane, flush_locked;
 * for the replay sets h264bsdmiReplayCreateSched).
 *
 * This replaces, for the pixels, what the reference does synchronously inside h264bsdDecode
 * (src/h264bsd_slice_data.c:185 -> h264bsdDecodeMacroblock, src/h264bsd_decoder.c:475 ->
 * h264bsdFilterPicture) and the malloc'ed frame buffers of src/h264bsd_dpb.c:1014-1031.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <vector>
#include <algorithm>
#include "kernels.hip.h"
#include "kernels/k_tensor_out.hip.h"
#include "kernels/k_tensor_aa.hip.h"
#include "kernels/k_tensor_roi.hip.h"
#include "kernels/k_tensor_remap.hip.h"
#include "kernels/k_motion.hip.h"
#include "kernels/region_common.hip.h"
#include "kernels/luma_search.hip.h"
#include "kernels/k_region_stats.hip.h"
#include "kernels/k_keep.hip.h"
#include "kernels/k_blend.hip.h"
#include "kernels/k_blend_spread.hip.h"
#include "kernels/k_warp_kept.hip.h"
#include "kernels/k_region_change.hip.h"
#include "kernels/k_region_shift.hip.h"
#include "kernels/k_cell_shift.hip.h"
#include "kernels/k_corner_points.hip.h"
#include "kernels/k_point_matches.hip.h"
#include "kernels/k_point_model.hip.h"
#include "kernels/k_cell_maps.hip.h"
#include "kernels/k_cell_boxes.hip.h"
#include "engine.h"
#include "hip_owned.h"
#include "tick_plan.h"
#include "../../include/h264bsd_mi355x_bench.h"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "h264bsd-mi355x: HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), \
                    __FILE__, __LINE__, #expr);                                                    \
            return -1;                                                                             \
        }                                                                                          \
    } while (0)

namespace {

constexpr int MAX_DEVICES = 16;
struct PendingJob { Pinned<uint8_t> host; uint32_t bytes = 0, cap = 0; };     /* host.dev(): the device's address of the pinned buffer (k_h2d) */
constexpr size_t MAX_QUEUED_PICTURES = 8;    /* per decoder instance, before sink_submit starts the device on its own */

/* The completion of one h264bsdmiNextOutputTensorBatch call, shared by the instances it read from (tensor_out_locked): until it has
 * passed, their frame buffers must neither be decoded into (lane_launch) nor freed (fence_drop).  Back to Engine.fences when no
 * instance refers to it any more. */
struct Fence { Event ev; unsigned refs = 0; };

struct StreamCtx {
    uint32_t wmb = 0, hmb = 0, n_slots = 0, frame_bytes = 0;
    DeviceMem<uint8_t> d_frames, d_dbk;
    Pinned<uint8_t> h_frame[FJ_MAX_SLOTS];  /* host mirrors of the frame buffers, written by the layout kernel itself through their device pointers (out_begin) */
    int out_slot = -1;                      /* the frame buffer whose picture is on its way to host memory (sink_fetch_begin .. sink_fetch_end) */
    std::vector<Pinned<uint8_t>> retired_host;      /* host mirrors of the frame buffers a new parameter set replaced: a picture pulled just before lives in one (freed at the next pull) */
    Pinned<uint32_t> h_conv; DeviceMem<uint32_t> d_conv;       /* converted picture: host mirror (with its device pointer); device copy (device-resident output) */
    Event out_ev;                           /* recorded behind the copy of a picture on its way out: the caller waits for it OUTSIDE the engine's mutex */
    std::mutex qmu;                         /* guards pending / free_bufs (submit runs on the caller's threads) */
    PendingJob acquired;                    /* staging buffer the parser is currently filling (sink_acquire) */
    std::deque<PendingJob> pending;
    std::vector<PendingJob> free_bufs;      /* recycled pinned staging buffers */
    /* lane scheduling (flush_locked): the light lane this instance belongs to, where its latest picture was launched
     * (lane index, launch number on that lane) and the first round of the current flush that may take its next one */
    int group = 0, last_lane = -1;
    unsigned long long last_launch = 0;
    unsigned ready_round = 0;
    size_t flush_quota = 0;                 /* jobs that were queued when the current flush began: it takes no others (flush_locked) */
    Fence *fence = nullptr;                 /* the latest tensor pull that read this instance's frames (nullptr: none outstanding) */
    /* motion export (h264bsdmiSetMotionExport): one slot of side information per frame buffer (kernels/k_motion.hip.h), and what the
     * ages are counted from — FjHeader.pic_seq of the last picture (ghost jobs excluded) decoded into every frame buffer since
     * sink_configure */
    bool motion = false;
    DeviceMem<uint8_t> d_motion; size_t motion_bytes = 0;      /* n_slots x motion_bytes */
    uint32_t slot_seq[FJ_MAX_SLOTS] = {}; bool slot_has[FJ_MAX_SLOTS] = {};
    /* the kept picture (h264bsdmiKeepCurrentPictures): one frame of kept_wmb x kept_hmb macroblock tiles, allocated at the instance's
     * first keep; it outlives sink_configure with the same size and goes, behind Engine.kept_ev, with another size or the instance */
    DeviceMem<uint8_t> d_kept; uint32_t kept_wmb = 0, kept_hmb = 0;
    /* the background model (h264bsdmiBlendCurrentPictures): the low byte of every sample of the kept picture, a second frame in the
     * same tiles, allocated at the instance's first blend and freed with d_kept; not valid (it reads as 0x80) after a plain keep */
    DeviceMem<uint8_t> d_kept_lo; bool kept_lo_valid = false;
    /* the background spread (h264bsdmiBlendCurrentPicturesSpread): one byte per sample of the kept picture, a third frame in the same
     * tiles, allocated at the instance's first spread blend and freed with d_kept; not valid (it reads as the call's `lowest`) after a
     * plain keep.  A warp leaves it where it lies */
    DeviceMem<uint8_t> d_spread; bool spread_valid = false;
    /* warped kept pictures (h264bsdmiWarpKeptPictures): the frames a warp writes, hi and (where lo is valid) lo, swapped with the live
     * ones behind its launch; allocated at the instance's first warp and freed with d_kept */
    DeviceMem<uint8_t> d_kept_spare, d_kept_lo_spare;
};

/* k_dbk (boundary strengths) needs only the frame job, not pixels: it runs on a second HIP stream next to the
 * reconstruction kernels of the same tick and joins before k_frame_dbk (measured: 245.2 -> 237.5 ms per step).  k_copy runs on a
 * THIRD stream beside both and joins before k_frame_intra (round 6: 87.5-88.5 -> 84.4-85.0 ms per step; on the SAME stream as
 * k_dbk, in front of it or behind it, it gains a third of that; k_recon_inter<1> behind it on that stream loses 2.4 ms again).  Other placements that were measured — k_dbk forked behind k_copy or
 * behind the inter kernels, k_dbk of the NEXT tick next to this tick's per-picture kernels — kept the sum or lost
 * (docs/EXPERIMENTS.md); those variants are not in the product. */
struct SideLane {
    Stream stream; Event fork, join;            /* k_dbk */
    Stream copy_stream; Event copy_join;        /* k_copy (launch_tick) */
    bool create(int dbk_priority, bool with_priority)
    {
        if ((with_priority ? stream.create(dbk_priority) : stream.create()) != hipSuccess) return false;
        return fork.create(hipEventDisableTiming) == hipSuccess && join.create(hipEventDisableTiming) == hipSuccess &&
               copy_stream.create() == hipSuccess && copy_join.create(hipEventDisableTiming) == hipSuccess;
    }
};

/* A lane = one HIP stream that runs ticks one after the other, with its own device arena for the frame jobs of a tick
 * and its own descriptor staging.  Light lanes: one per stream group (decoder instances are dealt round-robin to the
 * groups), so that the per-picture kernels of one group — which last as long as the slowest picture of the tick —
 * overlap with the work of the other groups.  Heavy lanes: pictures that are mostly intra coded take 3-4 times as long
 * as the others in the per-picture kernels; they leave their group's tick and run on one of these, and the instance
 * rejoins its group HEAVY_DELAY rounds later if it has that many pictures queued.  Order inside one instance is kept by
 * events: every launch records ring[launch number % RING] on its lane, and a picture whose predecessor ran on another
 * lane makes its lane wait for that event (a recycled ring slot stands for a later launch of the same lane, which only
 * waits longer).  Measured on the replay sets: 256 desynchronised 1080p streams, 304 M MB/s with common
 * ticks, 550 M with heavy lanes, 660 M with 8 groups + 4 heavy lanes; more than ~12 busy HIP streams fall off a cliff
 * on this runtime (tools/probes/queue_probe.hip), and the runtime's default of 4 hardware queues serialises lanes:
 * the library asks for 16 (GPU_MAX_HW_QUEUES) when it is loaded before the HIP runtime starts. */
struct Lane {
    hipStream_t st = nullptr;                  /* own_st, or the engine's stream (single-lane engine) */
    Stream own_st;
    DeviceMem<uint8_t> d_arena; size_t arena_cap = 0;      /* device copies of the blobs of one tick */
    DeviceMem<FrameDesc> d_desc; Staged<FrameDesc> descs;      /* the tick's descriptors: device copy (descs.cap() of them), staging ring */
    Pinned<h264k::H2dItem> h_items;            /* pinned, 2 halves of descs.cap() under the guard of descs' halves: the tick's jobs for k_h2d (h_items.dev(): the device's view of it) */
    Staged<h264k::MotionKeepItem> mitems;      /* k_motion_keep's items (allocated by the first tick that holds a picture of an instance with motion export) */
    static constexpr unsigned RING = 64;
    Event ring[RING];
    unsigned long long launches = 0;
    Event tail;
    const SideLane *side = nullptr;
};
constexpr unsigned HEAVY_DELAY = 4;
constexpr unsigned MAX_LANES_TOTAL = 10;     /* light + heavy lanes of an engine (the engine's own stream and the side stream come on top) */
#ifndef CONVERT_WGS_N
#define CONVERT_WGS_N 128       /* a wavefront converts batches of CONV_BATCH tile pairs: 128 workgroups x 4 wavefronts = the 510 batches of a 1080p picture */
#endif
constexpr unsigned CONVERT_WGS = CONVERT_WGS_N;      /* workgroups per picture of k_convert_tiles in batched launches */
#ifndef CONV_WAVES_N
#define CONV_WAVES_N 4          /* wavefronts of a k_frame_dbk workgroup that convert another picture before they filter (TickShape.conv) */
#endif
#define CONVERT_GRID(n) dim3(CONVERT_WGS, (n))
/* Under lane scheduling a k_frame_dbk workgroup shares its compute unit with the other lanes' kernels: 8 wavefronts
 * hold less of the register file than the 12 that are best when a tick has the GPU to itself (desynchronised replay
 * with 9 groups: 763 vs 734 M MB/s; lock-step, single lane: 12 wavefronts 54.9 ms per step, 8: 56.8). */
#ifndef LANE_DBK_WAVES_N
#define LANE_DBK_WAVES_N 8
#endif
constexpr uint32_t LANE_DBK_WAVES = LANE_DBK_WAVES_N;

/* the item stride of the tensor pulls' staging ring: k_tensor_out / k_tensor_resize read TensorItems, k_tensor_aa AaItems, k_tensor_roi
 * RoiItems, k_motion_roi MotionItems, k_tensor_remap RemapItems, k_region_stats StatsItems, k_keep KeepItems, k_blend BlendItems, k_blend_spread SpreadItems, k_warp_kept WarpItems, k_kept_out KeptOutItems, k_region_change ChangeItems, k_region_shift ShiftItems, k_corner_points CornerItems,
 * k_cell_maps CellItems (k_cell_boxes: the same, and its BoxItems in slots of their own behind them), k_cell_shift FlowItems,
 * k_point_describe / k_point_match MatchItems */
constexpr size_t TITEM_BYTES = std::max({ sizeof(h264k::TensorItem), sizeof(h264k::AaItem), sizeof(h264k::RoiItem), sizeof(h264k::MotionItem),
                                          sizeof(h264k::RemapItem), sizeof(h264k::StatsItem), sizeof(h264k::KeepItem), sizeof(h264k::ChangeItem),
                                          sizeof(h264k::CellItem), sizeof(h264k::BoxItem), sizeof(h264k::ShiftItem), sizeof(h264k::BlendItem), sizeof(h264k::SpreadItem),
                                          sizeof(h264k::KeptOutItem), sizeof(h264k::CornerItem), sizeof(h264k::FlowItem), sizeof(h264k::MatchItem), sizeof(h264k::WarpItem) });
struct TItemSlot { uint8_t bytes[TITEM_BYTES]; };
struct Engine {
    std::mutex mu;
    int device = 0;
    Stream stream;
    Stream out_stream;                       /* pictures on their way to host memory (out_begin): behind the picture's OWN tick, not behind every lane */
    std::vector<Lane> lanes;                 /* [0, n_light) light lanes, then n_heavy heavy lanes */
    unsigned n_light = 1, n_heavy = 0, heavy_rr = 0, group_rr = 0;
    std::vector<StreamCtx *> streams;
    DeviceMem<uint8_t> conv_in; DeviceMem<uint32_t> conv_out; size_t conv_cap = 0; /* eng_convert_host scratch */
    std::vector<std::pair<StreamCtx *, PendingJob>> inflight;   /* staging buffers of enqueued, unfinished ticks */
    Event inflight_done;
    bool inflight_recorded = false;          /* inflight_done has been recorded behind everything in `inflight` */
    SideLane side;
    /* device error word (DEVERR_* bits, kernels.hip.h): the kernels OR into d_err, poll_errors() folds it into `errors`
     * whenever the host has waited for the device anyway */
    DeviceMem<uint32_t> d_err; Pinned<uint32_t> h_err;      /* device error words, their pinned host copy (with its device pointer) */
    uint32_t errors = 0;                       /* sticky bits (written with __atomic_fetch_or under mu, read without the lock) */
    uint32_t error_events = 0;                 /* how often a tripwire fired, ever: monotonic, so that a NEW occurrence of a bit that is
                                                  already set is visible (per-decoder copy-elision guard, the tests' delta) */
    DeviceMem<unsigned long long> tail_prof;   /* debug: per-wave cycle accounting of the per-picture kernels (block 0) */
    /* tensor pulls (tensor_out_locked): the staging ring of their items; fence events that no instance holds any more */
    Staged<TItemSlot> titems;
    std::vector<Fence *> fences;
    /* region and change statistics and the region shift with row bands (stats_scratch_locked): the regions' tickets (STATS_MAX_PARTIALS words, zero between
     * launches), then the bands' partial records; stats_ev is recorded behind the latest launch that used them, and the next one waits for it */
    DeviceMem<uint8_t> d_stats;
    Event stats_ev;
    /* kept pictures (StreamCtx.d_kept) are written on one caller's stream and read on another's: kept_ev is recorded behind EVERY launch
     * that reads or writes any of them and waited for by the next such launch, which puts them in one total order: the latest
     * recording covers all earlier ones, and a kept buffer is freed behind it (kept_drop) */
    Event kept_ev;
    bool kept_recorded = false;
    /* h264bsdmiOutputPointModel without a caller's stream: recorded behind its launch on the engine's stream, and waited for */
    Event model_ev;
};

/* One engine per HIP device, created on first use.  A decoder instance (or replay set) lives on the device that is
 * current for the thread that initialises it: h264bsdmiSetDevice() sets it for the calling thread (and, the first time,
 * the process default); one process can therefore drive several GPUs, and the usual one-process-per-GPU launch just
 * calls it once. */
Engine *g_engines[MAX_DEVICES] = {};
std::mutex g_engine_mu;
int g_default_device = -1;
thread_local int tl_device = -1;

int current_device()
{
    if (tl_device >= 0) return tl_device;
    if (g_default_device >= 0) return g_default_device;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    return d;
}

/* The HIP runtime maps streams onto 4 hardware queues unless told otherwise, and it reads the setting when it starts
 * (first HIP call of the process): lanes that share a queue run one after the other.  Ask for 16 unless the
 * application has chosen a value itself.  When the application has started the runtime before this library is loaded
 * this comes too late; set GPU_MAX_HW_QUEUES=16 in the environment then. */
__attribute__((constructor)) static void lib_init() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }

/* Lane configuration: H264BSDMI_LANES="<groups>,<heavy lanes>".  Default: 4,2 when HIP streams are found to run side
 * by side (streams_run_concurrently), else one lane = the engine's own stream. */
/* Do HIP streams really run side by side here?  The answer depends on how many hardware queues the runtime was started
 * with, which the library cannot see (and can only influence when it is loaded first): it is measured.  One workgroup
 * that spins for ~500 us on each of eight fresh streams: side by side they take about as long as one, on shared queues
 * several times as long.  Returns 1 when the eight ran concurrently. */
/* the device's two error words into their pinned host copy, in stream order behind a picture on its way out (out_end_locked) */
__global__ void k_err_words(const uint32_t *__restrict__ d_err, uint32_t *__restrict__ host) { if (threadIdx.x < 2) host[threadIdx.x] = d_err[threadIdx.x]; }
__global__ void k_spin(long long ticks) { const long long t0 = wall_clock64(); while (wall_clock64() - t0 < ticks) { } }

static int streams_run_concurrently(Engine *e)
{
    constexpr int N = 8;
    Stream st[N];
    Event ev[2];
    int ok = 1;
    float one = 0, all = 0;
    for (auto &s : st) if (s.create() != hipSuccess) ok = 0;
    for (auto &v : ev) if (v.create() != hipSuccess) ok = 0;
    int rate_khz = 100000;                                         /* wall_clock64 ticks at 100 MHz on gfx9 */
    if (hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, e->device) != hipSuccess || rate_khz <= 0) rate_khz = 100000;
    const long long ticks = (long long)rate_khz * 500 / 1000;      /* 500 us: long against the ~0.15 ms of event traffic around the eight */
    if (ok) {
        /* warm-up: code object load, and the hardware queue behind every stream (created on first use) */
        for (auto &s : st) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s, 1);
        for (auto &s : st) ok = ok && hipStreamSynchronize(s) == hipSuccess;
    }
    if (ok) {
        hipEventRecord(ev[0], st[0]);
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[0], ticks);
        hipEventRecord(ev[1], st[0]);
        ok = hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&one, ev[0], ev[1]) == hipSuccess;
    }
    if (ok) {
        /* st[0] starts the clock, waits for the other five, stops it */
        Event done[N];
        hipEventRecord(ev[0], st[0]);
        for (int i = 1; i < N; i++) hipStreamWaitEvent(st[i], ev[0], 0);
        for (int i = 0; i < N; i++) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[i], ticks);
        for (int i = 1; i < N; i++) {
            if (done[i].create(hipEventDisableTiming) != hipSuccess) { ok = 0; break; }
            hipEventRecord(done[i], st[i]);
            hipStreamWaitEvent(st[0], done[i], 0);
        }
        hipEventRecord(ev[1], st[0]);
        ok = ok && hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&all, ev[0], ev[1]) == hipSuccess;
    }
    if (getenv("H264BSDMI_TRACE_LANES")) fprintf(stderr, "h264bsd-mi355x: stream probe: one %.3f ms, eight %.3f ms, ok %d\n", one, all, ok);
    return ok && one > 0 && all < 1.7f * one;       /* measured: 16 hardware queues 1.24 x, 4 queues 3.1 x */
}

static int lanes_create(Engine *e)
{
    unsigned g = 1, k = 0;
    if (!getenv("H264BSDMI_LANES")) {
        if (streams_run_concurrently(e)) { g = 4; k = 2; }
        else fprintf(stderr, "h264bsd-mi355x: HIP streams do not run side by side in this process (the runtime was probably started with its "
                             "default of 4 hardware queues before this library was loaded): one lane; set GPU_MAX_HW_QUEUES=16\n");
    }
    if (const char *cfg = getenv("H264BSDMI_LANES")) {
        unsigned a = 0, b = 0;
        if (sscanf(cfg, "%u,%u", &a, &b) >= 1 && a >= 1) {
            /* whatever is asked for, stay below the cliff: more than ~12 busy HIP streams (lanes + the engine's own two) make
             * this runtime crawl (19-53 s instead of 0.2 s per lap, tools/probes/queue_probe.hip) */
            g = std::min(a, 8u); k = std::min(b, 4u);
            while (g + k > MAX_LANES_TOTAL && g > 1) g--;
            if (g != a || k != b) fprintf(stderr, "h264bsd-mi355x: H264BSDMI_LANES=%s clamped to %u,%u (at most %u lanes)\n", cfg, g, k, MAX_LANES_TOTAL);
        } else fprintf(stderr, "h264bsd-mi355x: H264BSDMI_LANES=%s ignored (expected <groups>,<heavy lanes>)\n", cfg);
    }
    std::vector<Lane> lanes(g + k);                        /* (handed to the engine only when complete) */
    for (unsigned i = 0; i < g + k; i++) {
        Lane &l = lanes[i];
        if (g == 1 && i == 0) { l.st = e->stream; l.side = &e->side; }      /* the single-lane engine: k_dbk next to the reconstruction kernels */
        else { HIP_TRY(l.own_st.create()); l.st = l.own_st; }
        HIP_TRY(l.tail.create(hipEventDisableTiming));
        for (auto &ev : l.ring) HIP_TRY(ev.create(hipEventDisableTiming));
    }
    e->n_light = g; e->n_heavy = k;
    e->lanes.swap(lanes);
    return 0;
}

Engine *engine_get(int device = -1)
{
    if (device < 0) device = current_device();
    if (device >= MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lk(g_engine_mu);
    if (g_engines[device]) return g_engines[device];
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n) return nullptr;
    std::unique_ptr<Engine> e(new Engine());          /* (released again if it cannot be completed; published, it lives until the process ends) */
    e->device = device;
    if (hipSetDevice(e->device) != hipSuccess || e->stream.create() != hipSuccess || e->inflight_done.create(hipEventDisableTiming) != hipSuccess ||
        ![&] {   /* the side stream (k_dbk next to the copy and inter kernels) gets the highest priority the device has: its few workgroups
                   * must not queue behind the hundred thousand of k_recon_inter */
            int lo = 0, hi = 0;
            const bool prio = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess;
            return e->side.create(hi, prio);
        }() ||
        e->d_err.alloc(256) != hipSuccess || hipMemset(e->d_err, 0, 256) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||   /* (hipMemset returns before the fill has run) */
        e->h_err.alloc(64, true) != hipSuccess) return nullptr;
    e->h_err[0] = e->h_err[1] = 0;
    return g_engines[device] = e.release();
}

/* how the two per-picture kernels split a picture: TailConfig (tick_plan.h), with the overrides of the environment read once */
TailConfig g_tail;
std::mutex g_tail_mu;
TailConfig tail_config()
{
    std::lock_guard<std::mutex> lk(g_tail_mu);
    if (!g_tail.from_env) {
        g_tail.from_env = true;
        if (const char *cfg = getenv("H264BSDMI_TAIL")) {
            unsigned v[7] = { 0, 0, 0, 0, 0, 0, 0 };
            if (sscanf(cfg, "%u,%u,%u,%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) >= 6) {
                g_tail.dbk_rows_light = v[0]; g_tail.dbk_rows_heavy = v[1]; g_tail.dbk_waves = v[2];
                g_tail.intra_rows_light = v[3]; g_tail.intra_rows_heavy = v[4]; g_tail.intra_waves = v[5];
                g_tail.dbk_chroma_waves = v[6];          /* optional seventh number; 0 = five twelfths of dbk_waves */
            } else fprintf(stderr, "h264bsd-mi355x: H264BSDMI_TAIL=%s ignored (expected six or seven numbers)\n", cfg);
        }
        if (const char *cfg = getenv("H264BSDMI_BAND_BUDGET")) g_tail.band_budget = (uint32_t)strtoul(cfg, nullptr, 10);
        if (const char *cfg = getenv("H264BSDMI_HEAVY_BUDGET")) g_tail.heavy_budget = (uint32_t)strtoul(cfg, nullptr, 10);
    }
    return g_tail;
}
static uint16_t bands_for(uint32_t hmb, uint32_t rows)
{
    if (!rows || rows >= hmb) return 1;
    return (uint16_t)std::min<uint32_t>((hmb + rows - 1) / rows, 64u);
}

/* ticket counters of the per-picture kernels (take_ticket, kernels.hip.h): one set per HIP stream that launches ticks —
 * launches on one stream run one after the other, launches on different streams may overlap.  [0,1] k_frame_dbk,
 * [2,3] k_frame_intra. */
std::mutex g_ticket_mu;
auto *const g_tickets = new std::vector<std::pair<hipStream_t, DeviceMem<uint32_t>>>[MAX_DEVICES];     /* (never destroyed, like the engines: no HIP call at exit) */
static uint32_t *tickets_for(hipStream_t st)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    for (auto &p : g_tickets[dev]) if (p.first == st) return p.second;
    /* zeroed ON the stream whose kernels count in it: hipMemset() on device memory returns before the fill has run, on the
     * null stream, which the (non-blocking) lane streams do not wait for — a fill that landed in the middle of the first
     * banded launch handed out tickets twice and left a band of a picture without a workgroup (rare, under load only) */
    DeviceMem<uint32_t> d;
    if (d.alloc(64) != hipSuccess || hipMemsetAsync(d, 0, 64, st) != hipSuccess) return nullptr;
    g_tickets[dev].emplace_back(st, std::move(d));
    return g_tickets[dev].back().second;
}
} // namespace
/* a stream is about to be destroyed (Stream, hip_owned.h): its counters go with it (a later stream may get the same handle and must not inherit them) */
void tickets_release(hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    for (int d = 0; d < MAX_DEVICES; d++)
        g_tickets[d].erase(std::remove_if(g_tickets[d].begin(), g_tickets[d].end(), [&](const auto &p) { return p.first == st; }), g_tickets[d].end());
}
namespace {
/* a banded launch that ended early (a scheduler gave up: DEVERR_*_SCHED) leaves its ticket counters non-zero, and every later
 * banded launch on that stream would map tickets to the wrong picture and band: after a device error all of them start over */
static void tickets_rezero(int dev)
{
    std::lock_guard<std::mutex> lk(g_ticket_mu);
    if (dev < 0 || dev >= MAX_DEVICES) return;
    for (auto &p : g_tickets[dev]) (void)hipMemsetAsync(p.second, 0, 64, p.first);
}

/* ---- launch of one tick (TickShape: tick_plan.h) ---- */

/* descriptor of one picture: device addresses of the sections of its (device-resident) frame job */
void make_desc(FrameDesc &d, const uint8_t *host_blob, const uint8_t *dev_blob, uint8_t *dev_frames, uint32_t frame_bytes,
               uint8_t *dev_dbk, TickShape *shape, uint32_t *dev_err)
{
    const FjHeader *h = reinterpret_cast<const FjHeader *>(host_blob);
    d.recs = reinterpret_cast<const FjMbRec *>(dev_blob + h->rec_off);
    d.mvx = reinterpret_cast<const int16_t *>(dev_blob + h->mvx_off);
    d.coefs = reinterpret_cast<const int16_t *>(dev_blob + h->coef_off);
    d.lvl = reinterpret_cast<const uint32_t *>(dev_blob + h->lvl_off);
    d.idx = reinterpret_cast<const uint16_t *>(dev_blob + h->idx_off);
    d.copy = reinterpret_cast<const FjCopy *>(dev_blob + h->copy_off);
    d.gen = reinterpret_cast<const FjGen *>(dev_blob + h->gen_off);
    d.n_copy = h->n_copy;
    d.n_gen = h->n_gen;
    d.n_gen_uni = h->n_gen_uniform;
    d.n_gen_quad = h->n_gen_quad;
    d.dbki = reinterpret_cast<const uint16_t *>(dev_blob + h->dbk_off);
    d.n_dbk = h->n_dbk;
    d.dbk = dev_dbk;
    d.cur = dev_frames + (size_t)h->cur_slot * frame_bytes;
    d.n_mbs = h->n_mbs;
    d.n_levels = h->n_intra_levels;
    d.wmb = h->width_mbs;
    d.wmb_magic = (uint32_t)(0x100000000ull / (h->width_mbs ? h->width_mbs : 1u)) + 1u;
    d.hmb = h->height_mbs;
    d.any_deblock = h->any_deblock;
    {
        const TailConfig tc = tail_config();
        const bool heavy = h->n_intra * 4u > h->n_mbs;
        d.heavy = heavy ? 1 : 0;
        d.dbk_bands = bands_for(h->height_mbs, heavy ? tc.dbk_rows_heavy : tc.dbk_rows_light);
        /* a concealed macroblock may wait for the macroblocks below it (FJ_NEED_D*): such a picture stays in one band,
         * a band never waits for a band that started after it */
        d.intra_bands = h->intra_down_deps ? 1 : bands_for(h->height_mbs, heavy ? tc.intra_rows_heavy : tc.intra_rows_light);
    }
    d.err = dev_err;
    d.conv_src = nullptr; d.conv_dst = nullptr; d.conv_fmt = 0; d.conv_pad = 0;
    for (uint32_t k = 0; k < FJ_MAX_SLOTS; k++) d.slot[k] = k < h->n_slots ? dev_frames + (size_t)k * frame_bytes : nullptr;
    if (shape) {
        shape->n_frames++;
        shape->max_mbs = std::max(shape->max_mbs, h->n_mbs);
        shape->max_copy = std::max(shape->max_copy, h->n_copy);
        shape->max_gen = std::max(shape->max_gen, h->n_gen);
        shape->max_gen_uni = std::max(shape->max_gen_uni, h->n_gen_uniform);
        shape->max_gen_quad = std::max(shape->max_gen_quad, h->n_gen_quad);
        shape->max_gen_rest = std::max(shape->max_gen_rest, h->n_gen - h->n_gen_uniform - h->n_gen_quad);
        shape->max_dbk = std::max(shape->max_dbk, h->n_dbk);
        shape->any_deblock |= h->any_deblock != 0;
        shape->max_levels = std::max(shape->max_levels, h->n_intra_levels);
        shape->max_w = std::max<uint32_t>(shape->max_w, h->width_mbs);
        shape->max_h = std::max<uint32_t>(shape->max_h, h->height_mbs);
        shape->any_tail |= h->n_intra_levels != 0 || h->any_deblock != 0;
        shape->n_heavy += d.heavy;
        if (h->any_deblock) (d.heavy ? shape->want_heavy : shape->want_light)[0] = std::max<uint32_t>((d.heavy ? shape->want_heavy : shape->want_light)[0], d.dbk_bands);
        if (h->n_intra_levels) (d.heavy ? shape->want_heavy : shape->want_light)[1] = std::max<uint32_t>((d.heavy ? shape->want_heavy : shape->want_light)[1], d.intra_bands);
        if (h->n_intra_levels && h->intra_down_deps) shape->intra_whole = true;
    }
}

struct TickTimers { Event ev[6]; Event sev[5]; bool on = false; bool copy_timed = false; unsigned mask = 31u; };   /* copy_timed: sev[3..4] were recorded by the latest launch_tick */   /* mask bit k: kernel k of KERNELS is timed */   /* boundaries of the 5 kernels of a tick; sev[1..2] = k_dbk on the side stream, sev[3..4] = k_copy on the copy stream */

/* k_dbk of one tick on st: the side stream beside the reconstruction kernels (SideLane), or the tick's own stream */
static void launch_kdbk(hipStream_t st, const FrameDesc *d_desc, const TickShape &s, uint32_t launches[5])
{
    /* one macroblock per lane, no stride loop: the grid is as long as the tick's longest list (a 1080p picture: at most 16 workgroups) */
    hipLaunchKernelGGL(h264k::k_dbk, dim3((s.max_dbk + 64 * DBK_WG_WAVES - 1) / (64 * DBK_WG_WAVES), s.n_frames), dim3(64 * DBK_WG_WAVES), 0, st, d_desc);
    if (launches) launches[2]++;
}
/* The three inter kernels of one tick, one per part of the general-inter list; n_uni, n_quad, n_rest: the entries in the tick's longest part of each
 * kind.  Single-wavefront workgroups: a chunk of entries each in the first two, one entry in the third. */
static void launch_inter(hipStream_t st, const FrameDesc *d_desc, uint32_t n_uni, uint32_t n_quad, uint32_t n_rest, uint32_t n_frames)
{
    if (n_uni) hipLaunchKernelGGL(h264k::k_recon_inter_lb, dim3((n_uni + INTER_LB_CHUNK - 1) / INTER_LB_CHUNK, n_frames), dim3(64), 0, st, d_desc);
    if (n_quad) hipLaunchKernelGGL(h264k::k_recon_inter_lq, dim3((n_quad + INTER_LQ_CHUNK - 1) / INTER_LQ_CHUNK, n_frames), dim3(64), 0, st, d_desc);
    if (n_rest) hipLaunchKernelGGL(h264k::k_recon_inter, dim3(n_rest, n_frames), dim3(64), 0, st, d_desc);
}
/* the dynamic LDS every device has allowed the per-picture kernels so far: [0 k_frame_dbk, 1 k_frame_intra][plain, banded variant][device] */
std::mutex g_tail_lds_mu;
size_t g_tail_lds[2][2][MAX_DEVICES] = {};
/* What the two per-picture kernels share between plan and launch on st.  *tickets: the stream's ticket counters when the launch is banded, else
 * nullptr; fn, the variant about to be launched, gets its LDS limit raised when this device has not yet seen one as large as the plan's for it. */
static int tail_prepare(hipStream_t st, int which, const BandPlan &bp, const void *fn, uint32_t **tickets)
{
    const bool banded = bp.bands > 1;
    *tickets = banded ? tickets_for(st) : nullptr;
    if (banded && !*tickets) return -1;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_tail_lds_mu);
    if (bp.lds > g_tail_lds[which][banded][dev]) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bp.lds));
        g_tail_lds[which][banded][dev] = bp.lds;
    }
    return 0;
}

int launch_tick(hipStream_t st, const FrameDesc *d_desc, const TickShape &s, TickTimers *tt, uint32_t launches[5],
                unsigned stages = 7u, const SideLane *side = nullptr, unsigned long long *prof = nullptr)
{
    const bool timed = tt && tt->on;
    const unsigned tmask = timed ? tt->mask : 0u;
    /* timer boundary i closes kernel i-1 and opens kernel i: recorded where either of the two is timed */
    auto boundary = [&](unsigned i) -> int {
        if ((((tmask << 1) | tmask) >> i) & 1u) HIP_TRY(hipEventRecord(tt->ev[i], st));
        return 0;
    };
    if (boundary(0)) return -1;
    const bool do_dbk = (stages & 4u) && s.any_deblock && s.max_dbk;
    const bool do_copy = (stages & 1u) && s.max_copy;
    const bool aside = side && side->stream && do_dbk;
    /* k_copy on a stream of its own beside k_recon_inter (and k_dbk): the copies are HBM-bound, the inter kernel is bound by
     * instruction issue, and they write different macroblocks of the picture; both are joined in front of k_frame_intra, whose
     * macroblocks read them.  84.5-85.2 against 87.5-88.5 ms per step (docs/EXPERIMENTS.md, "k_copy beside the inter kernels"). */
    const bool copy_aside = aside && do_copy && side->copy_stream;
    if (tt) tt->copy_timed = false;
    auto launch_copy = [&](hipStream_t cs) {
        hipLaunchKernelGGL(h264k::k_copy, dim3(std::min<uint32_t>((s.max_copy + 3) / 4, COPY_WGS), s.n_frames), dim3(256), 0, cs, d_desc);   /* COPY_WGS workgroups per picture walk its run list */
        if (launches) launches[0]++;
    };
    if (aside) {
        HIP_TRY(hipEventRecord(side->fork, st));                 /* after the previous tick's k_frame_dbk: the records are free */
        HIP_TRY(hipStreamWaitEvent(side->stream, side->fork, 0));
        if (copy_aside) {
            const bool ctimed = timed && (tmask & 1u) && tt->sev[3] && tt->sev[4];
            if (tt) tt->copy_timed = ctimed;
            HIP_TRY(hipStreamWaitEvent(side->copy_stream, side->fork, 0));
            if (ctimed) HIP_TRY(hipEventRecord(tt->sev[3], side->copy_stream));
            launch_copy(side->copy_stream);
            if (ctimed) HIP_TRY(hipEventRecord(tt->sev[4], side->copy_stream));
            HIP_TRY(hipEventRecord(side->copy_join, side->copy_stream));
        }
        /* k_dbk on the side stream, which now waits for whatever frees the tick's deblocking scratch; the join event behind it */
        const bool dtimed = timed && (tmask & 4u);
        if (dtimed && tt->sev[1]) HIP_TRY(hipEventRecord(tt->sev[1], side->stream));
        launch_kdbk(side->stream, d_desc, s, launches);
        if (dtimed && tt->sev[2]) HIP_TRY(hipEventRecord(tt->sev[2], side->stream));
        HIP_TRY(hipEventRecord(side->join, side->stream));
    }
    if (do_copy && !copy_aside) launch_copy(st);
    if (boundary(1)) return -1;
    if ((stages & 1u) && s.max_gen) {
        launch_inter(st, d_desc, s.max_gen_uni, s.max_gen_quad, s.max_gen_rest, s.n_frames);
        if (launches) launches[1]++;
    }
    if (boundary(2)) return -1;
    if (do_dbk && !aside) launch_kdbk(st, d_desc, s, launches);
    if (boundary(3)) return -1;
    const TailConfig tc = tail_config();                         /* the row bands of the two per-picture kernels: plan_bands (tick_plan.h) */
    if (copy_aside) HIP_TRY(hipStreamWaitEvent(st, side->copy_join, 0));      /* (the copies have to be there before the intra macroblocks read them) */
    if (s.max_levels && (stages & 2u)) {
        BandPlan bp;
        /* a picture with concealed macroblocks must stay in one band (FjHeader.intra_down_deps): fewer wavefronts, never
         * shorter bands */
        if (plan_bands(s, tc, 1, std::max<uint32_t>(1u, std::min<uint32_t>(tc.intra_waves, h264k::TAIL_WAVES)), h264k::intra_lds_bytes, false, bp)) {
            fprintf(stderr, "h264bsd-mi355x: picture of %u x %u macroblocks is too large for k_frame_intra\n", s.max_w, s.max_h); return -1;
        }
        uint32_t *tickets;
        if (tail_prepare(st, 1, bp, bp.bands > 1 ? (const void *)h264k::k_frame_intra<true> : (const void *)h264k::k_frame_intra<false>, &tickets)) return -1;
        if (bp.bands > 1) hipLaunchKernelGGL(h264k::k_frame_intra<true>, dim3(s.n_frames * bp.bands), dim3(64 * bp.waves), bp.lds, st, d_desc, prof, tickets + 2, bp.bands, bp.rows, bp.light_cap);
        else hipLaunchKernelGGL(h264k::k_frame_intra<false>, dim3(s.n_frames), dim3(64 * bp.waves), bp.lds, st, d_desc, prof, nullptr, 1u, bp.rows, 1u);
        if (launches) launches[3]++;
    }
    if (boundary(4)) return -1;
    if (aside) HIP_TRY(hipStreamWaitEvent(st, side->join, 0));
    if (s.any_deblock && (stages & 4u)) {
        BandPlan bp;
        if (plan_bands(s, tc, 0, std::max<uint32_t>(1u, std::min<uint32_t>(s.dbk_waves ? s.dbk_waves : tc.dbk_waves, h264k::DBK_WAVES)), h264k::dbk_lds_bytes, true, bp)) {
            fprintf(stderr, "h264bsd-mi355x: picture %u macroblocks wide is too large for k_frame_dbk\n", s.max_w); return -1;
        }
        const uint32_t waves = bp.waves;      /* five twelfths of a workgroup's wavefronts start on the chroma graph (k_frame_dbk.hip.h); the seventh number of H264BSDMI_TAIL overrides */
        const uint32_t chroma_waves = tc.dbk_chroma_waves ? tc.dbk_chroma_waves : std::max<uint32_t>(1u, (waves * 5u + 6u) / 12u);     /* 12 -> 5 (4 / 5 / 6: 31.6 / 30.3 / 30.3 ms per step), 8 -> 3 */
        const uint32_t conv_waves = !s.conv ? 0u : std::min<uint32_t>(s.conv_waves ? s.conv_waves : (uint32_t)CONV_WAVES_N, waves > chroma_waves + 1u ? waves - chroma_waves - 1u : 0u);
        uint32_t *tickets;
        if (tail_prepare(st, 0, bp, bp.bands > 1 ? (const void *)h264k::k_frame_dbk<true> : (const void *)h264k::k_frame_dbk<false>, &tickets)) return -1;
        if (bp.bands > 1) hipLaunchKernelGGL(h264k::k_frame_dbk<true>, dim3(s.n_frames * bp.bands), dim3(64 * waves), bp.lds, st, d_desc, prof, tickets, bp.bands, bp.rows, bp.light_cap, chroma_waves, conv_waves);
        else hipLaunchKernelGGL(h264k::k_frame_dbk<false>, dim3(s.n_frames), dim3(64 * waves), bp.lds, st, d_desc, prof, nullptr, 1u, bp.rows, 1u, chroma_waves, conv_waves);
        if (launches) launches[4]++;
    }
    if (s.conv && !(s.any_deblock && (stages & 4u)))             /* no k_frame_dbk in this tick: nobody hosted the conversion */
        hipLaunchKernelGGL(h264k::k_convert_rest, dim3(CONVERT_WGS, s.n_frames), dim3(256), 0, st, d_desc);
    if (boundary(5)) return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Fold the device error word into the engine's sticky error bits.  Called where the host waits for the stream anyway. */
static void fold_errors(Engine *e)                    /* h_err holds a copy of the device's words that has arrived */
{
    const uint32_t fresh = e->h_err[0] & ~e->errors;
    /* monotonic: the pinned words are written by copies on two streams, an older snapshot may land last */
    if (e->h_err[1] > __atomic_load_n(&e->error_events, __ATOMIC_RELAXED)) __atomic_store_n(&e->error_events, e->h_err[1], __ATOMIC_RELAXED);
    if (fresh) {
        fprintf(stderr, "h264bsd-mi355x: DEVICE ERROR 0x%x:%s%s%s — pixels of the affected pictures are not trustworthy\n", fresh,
                (fresh & DEVERR_RESIDUAL_RANGE) ? " residual outside [-512,511] reached the kernels (host check missed it)" : "",
                (fresh & DEVERR_INTRA_SCHED) ? " k_frame_intra scheduler gave up" : "", (fresh & DEVERR_DBK_SCHED) ? " k_frame_dbk scheduler gave up" : "");
        __atomic_fetch_or(&e->errors, fresh, __ATOMIC_RELAXED);
        tickets_rezero(e->device);
    }
}
int poll_errors(Engine *e)
{
    HIP_TRY(hipMemcpyAsync(e->h_err, e->d_err, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    fold_errors(e);
    return 0;
}

/* ---- lazy execution of the queued jobs of all decoder instances ---- */
/* Recycle the pinned staging buffers of ticks whose copies have completed (all of them after wait != 0). */
int reap_locked(Engine *e, bool wait)
{
    if (e->inflight.empty()) return 0;
    if (wait) {
        /* (after a failed flush the event may be missing: wait for the lanes themselves before the staging buffers go back) */
        if (!e->inflight_recorded) for (auto &l : e->lanes) if (l.st) (void)hipStreamSynchronize(l.st);
        if (poll_errors(e)) return -1;
    } else if (!e->inflight_recorded || hipEventQuery(e->inflight_done) != hipSuccess) return 0;
    for (auto &f : e->inflight) {
        std::lock_guard<std::mutex> ql(f.first->qmu);
        f.first->free_bufs.push_back(std::move(f.second));
    }
    e->inflight.clear();
    return 0;
}

/* s no longer refers to its fence; the fence goes back to the pool when no instance does */
static void fence_unref(Engine *e, StreamCtx *s)
{
    Fence *f = s->fence;
    if (!f) return;
    s->fence = nullptr;
    if (--f->refs == 0) e->fences.push_back(f);
}
/* s's frame buffers are about to be cleared or freed: a tensor pull that still reads them must finish first */
static void fence_drop(Engine *e, StreamCtx *s)
{
    if (s->fence) (void)hipEventSynchronize(s->fence->ev);
    fence_unref(e, s);
}

/* s's kept picture is about to be freed: every launch that reads or writes a kept buffer must have finished */
static void kept_drop(Engine *e, StreamCtx *s)
{
    if (!s->d_kept) return;
    if (e->kept_recorded) (void)hipEventSynchronize(e->kept_ev);
    s->d_kept.reset(); s->d_kept_lo.reset(); s->d_kept_spare.reset(); s->d_kept_lo_spare.reset(); s->d_spread.reset();
    s->kept_wmb = s->kept_hmb = 0; s->kept_lo_valid = false; s->spread_valid = false;
}

/* ---- motion export: the side information of a picture kept beside its frame buffer (kernels/k_motion.hip.h) ----
 * The job about to be launched for instance s, as an item of the tick's k_motion_keep launch.  The side information of a frame
 * buffer is that of the last job decoded into it that is no ghost: ghost jobs (pre-passes of the picture that follows in the same
 * slot) write nothing and leave the table alone, the deblock-only job of a picture that was rendered as several jobs comes last
 * and carries the records the reference ends up with.  The kernel gets the ages as they stood BEFORE this job. */
static void motion_keep_item(StreamCtx *s, const uint8_t *host_blob, const uint8_t *dev_blob, std::vector<h264k::MotionKeepItem> &keep)
{
    const FjHeader *h = reinterpret_cast<const FjHeader *>(host_blob);
    if (h->ghost || !s->d_motion || h->cur_slot >= s->n_slots || h->n_mbs != s->wmb * s->hmb) return;
    h264k::MotionKeepItem it{ reinterpret_cast<const FjMbRec *>(dev_blob + h->rec_off), reinterpret_cast<const int16_t *>(dev_blob + h->mvx_off),
                              s->d_motion + (size_t)h->cur_slot * s->motion_bytes, h->n_mbs, s->wmb, s->n_slots, h->n_mvx, {} };
    for (uint32_t k = 0; k < s->n_slots; k++)
        it.age[k] = s->slot_has[k] && k != h->cur_slot ? (uint8_t)std::min<uint32_t>(h->pic_seq - s->slot_seq[k], 255u) : 0;
    s->slot_seq[h->cur_slot] = h->pic_seq; s->slot_has[h->cur_slot] = true;
    keep.push_back(it);
}
/* one k_motion_keep launch for the tick just enqueued on lane l; it reads the jobs where the tick's kernels read them */
static int motion_keep_launch(Lane &l, const std::vector<h264k::MotionKeepItem> &keep)
{
    HIP_TRY(l.mitems.reserve(keep.size(), std::max<size_t>(2 * keep.size(), 64)));
    memcpy(l.mitems.host(), keep.data(), keep.size() * sizeof(h264k::MotionKeepItem));
    uint32_t max_mbs = 0;
    for (const auto &it : keep) max_mbs = std::max(max_mbs, it.n_mbs);
    hipLaunchKernelGGL(h264k::k_motion_keep, dim3(std::min<uint32_t>((max_mbs + 15u) / 16u, 1024u), (uint32_t)keep.size()), dim3(256), 0, l.st,
                       l.mitems.dev());
    HIP_TRY(hipGetLastError());
    HIP_TRY(l.mitems.submit(l.st));
    return 0;
}

/* One tick on one lane: the front jobs of `part` (popped here) are copied to the lane's arena and launched. */
static int lane_launch(Engine *e, unsigned lane_idx, const std::vector<StreamCtx *> &part)
{
    Lane &l = e->lanes[lane_idx];
    size_t bytes = 0;
    for (StreamCtx *s : part) {
        std::lock_guard<std::mutex> ql(s->qmu);
        bytes += (s->pending.front().bytes + 255u) & ~255u;
    }
    if (bytes > l.arena_cap) {
        HIP_TRY(hipStreamSynchronize(l.st));               /* earlier ticks may still read the old arena */
        l.arena_cap = bytes + bytes / 4;
        HIP_TRY(l.d_arena.alloc(l.arena_cap));
    }
    if (part.size() > l.descs.cap()) {
        HIP_TRY(hipStreamSynchronize(l.st));               /* earlier ticks may still read the old descriptors */
        HIP_TRY(l.d_desc.alloc(2 * part.size() * sizeof(FrameDesc)));
        HIP_TRY(l.h_items.alloc(2 * 2 * part.size() * sizeof(h264k::H2dItem), true));
    }
    HIP_TRY(l.descs.reserve(part.size(), 2 * part.size()));      /* staged in pinned memory so that the copy can be asynchronous; the k_h2d items ride on the same half */
    FrameDesc *descs = l.descs.host();
    const size_t items_half = (size_t)l.descs.half() * l.descs.cap();
    h264k::H2dItem *items = l.h_items + items_half;
    /* how the jobs reach the device: one k_h2d launch that reads the pinned staging buffers (256 hipMemcpyAsync calls per tick before) */
    TickShape shape;
    size_t off = 0;
    std::vector<std::pair<int, unsigned long long>> waited;
    std::vector<const Fence *> fenced;
    std::vector<h264k::MotionKeepItem> keep;       /* the jobs of this tick whose side information is kept: none unless an instance asked */
    for (size_t i = 0; i < part.size(); i++) {
        StreamCtx *s = part[i];
        PendingJob j;
        { std::lock_guard<std::mutex> ql(s->qmu); j = std::move(s->pending.front()); s->pending.pop_front(); }
        if (s->fence) {         /* a tensor pull (on the caller's stream) may still read the frame buffer this picture is decoded into */
            if (hipEventQuery(s->fence->ev) == hipSuccess) fence_unref(e, s);
            else if (std::find(fenced.begin(), fenced.end(), s->fence) == fenced.end()) {
                HIP_TRY(hipStreamWaitEvent(l.st, s->fence->ev, 0));
                fenced.push_back(s->fence);
            }
        }
        if (s->last_lane >= 0 && (unsigned)s->last_lane != lane_idx) {     /* its previous picture ran on another lane */
            const std::pair<int, unsigned long long> key(s->last_lane, s->last_launch);
            if (std::find(waited.begin(), waited.end(), key) == waited.end()) {
                HIP_TRY(hipStreamWaitEvent(l.st, e->lanes[s->last_lane].ring[s->last_launch % Lane::RING], 0));
                waited.push_back(key);
            }
        }
        items[i] = h264k::H2dItem{ j.host.dev(), l.d_arena + off, j.bytes, 0u };
        make_desc(descs[i], j.host, l.d_arena + off, s->d_frames, s->frame_bytes, s->d_dbk, &shape, e->d_err);
        if (s->motion) motion_keep_item(s, j.host, l.d_arena + off, keep);
        off += (j.bytes + 255u) & ~255u;
        e->inflight.emplace_back(s, std::move(j));
        e->inflight_recorded = false;
        s->last_lane = (int)lane_idx; s->last_launch = l.launches;
    }
    hipLaunchKernelGGL(h264k::k_h2d, dim3(h264k::H2D_CHUNKS, (uint32_t)part.size()), dim3(256), 0, l.st, l.h_items.dev() + items_half);
    HIP_TRY(hipMemcpyAsync(l.d_desc, descs, part.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, l.st));
    HIP_TRY(l.descs.submit(l.st));
    if (e->lanes.size() > 1) shape.dbk_waves = LANE_DBK_WAVES;
    shape.load = (uint32_t)e->streams.size();
    if (launch_tick(l.st, l.d_desc, shape, nullptr, nullptr, 7u, l.side)) return -1;
    /* behind the tick's kernels and in front of the ring event: a pull that waits for the picture finds its side information, the
     * arena's next tick is behind it on this stream, and the picture's own kernels are not delayed */
    if (!keep.empty() && motion_keep_launch(l, keep)) return -1;
    HIP_TRY(hipEventRecord(l.ring[l.launches % Lane::RING], l.st));
    l.launches++;
    return 0;
}

/* Enqueue the pending jobs, round by round: a round takes at most one picture per instance; the light pictures of a
 * group form one tick on the group's lane, the heavy pictures of all groups one tick on a heavy lane (Lane, above).
 * wait: block until the pixels exist; otherwise return once everything is enqueued (the staging buffers stay owned by
 * `inflight`). */
int flush_locked(Engine *e, bool wait = true)
{
    HIP_TRY(hipSetDevice(e->device));
    if (reap_locked(e, false)) return -1;
    if (e->lanes.empty() && lanes_create(e)) return -1;      /* on first use: a process that only runs replay sets keeps its HIP streams for those */
    const bool multi = e->lanes.size() > 1;
    bool started = false;
    std::vector<std::vector<StreamCtx *>> part(e->n_light);
    std::vector<StreamCtx *> heavy;
    /* A flush enqueues what was submitted BEFORE it began.  An application may call h264bsdmiFlushAsync() on one thread while
     * its other threads are already parsing the next round (the call takes as long as enqueueing 256 jobs does): pictures that
     * arrive meanwhile wait for the next flush instead of forming straggler ticks of a few streams each. */
    for (StreamCtx *s : e->streams) { std::lock_guard<std::mutex> ql(s->qmu); s->flush_quota = s->pending.size(); }
    for (unsigned round = 0;; round++) {
        bool any_pending = false;
        for (auto &p : part) p.clear();
        heavy.clear();
        for (StreamCtx *s : e->streams) {
            std::lock_guard<std::mutex> ql(s->qmu);
            if (s->pending.empty() || !s->flush_quota) continue;
            any_pending = true;
            if (s->ready_round > round) continue;
            s->flush_quota--;
            const FjHeader *h = reinterpret_cast<const FjHeader *>(s->pending.front().host.get());
            if (e->n_heavy && h->n_intra * 4u > h->n_mbs) heavy.push_back(s);
            else part[(unsigned)s->group % e->n_light].push_back(s);
        }
        if (!any_pending) break;
        started = true;
        for (unsigned g = 0; g < e->n_light; g++)
            if (!part[g].empty() && lane_launch(e, g, part[g])) return -1;
        if (!heavy.empty()) {
            if (lane_launch(e, e->n_light + e->heavy_rr++ % e->n_heavy, heavy)) return -1;
            for (StreamCtx *s : heavy) s->ready_round = round + 1 + HEAVY_DELAY;
        }
    }
    for (StreamCtx *s : e->streams) s->ready_round = 0;          /* rounds count from the start of a flush */
    /* Lanes never wait for the engine's own stream: everything that stream does to frame buffers (clearing them in
     * sink_configure, laying pictures out for the application) is complete when the call that enqueued it returns. */
    if (started && multi)
        for (auto &l : e->lanes) {                               /* the engine's stream continues behind all lanes */
            HIP_TRY(hipEventRecord(l.tail, l.st));
            HIP_TRY(hipStreamWaitEvent(e->stream, l.tail, 0));
        }
    if (!e->inflight.empty()) { HIP_TRY(hipEventRecord(e->inflight_done, e->stream)); e->inflight_recorded = true; }
    return wait ? reap_locked(e, true) : 0;
}

/* ---- JobSink implementation ---- */
struct SinkUser { Engine *e; StreamCtx *s; };

void stream_release(StreamCtx *s, bool keep_pulled = false)
{
    s->pending.clear();
    s->free_bufs.clear();
    s->acquired = PendingJob();
    s->d_frames.reset(); s->d_dbk.reset(); s->d_motion.reset();
    /* keep_pulled (a new sequence re-allocates the frame buffers, sink_configure): h264bsdmiPullAndDecodePictureBatch hands out a picture and
     * parses on in the same call — the picture must outlive the activation of a parameter set that the parsing may bring */
    for (auto &p : s->h_frame) { if (keep_pulled && p) s->retired_host.push_back(std::move(p)); p.reset(); }
    if (!keep_pulled) s->retired_host.clear();
    s->h_conv.reset(); s->d_conv.reset(); s->out_ev.reset();
}

int sink_configure(void *user, uint32_t wmb, uint32_t hmb, uint32_t n_slots)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    std::lock_guard<std::mutex> lk(u->e->mu);
    if (flush_locked(u->e)) return -1;
    HIP_TRY(hipSetDevice(u->e->device));
    if (u->e->out_stream) HIP_TRY(hipStreamSynchronize(u->e->out_stream));
    fence_drop(u->e, u->s);
    if (u->s->kept_wmb != wmb || u->s->kept_hmb != hmb) kept_drop(u->e, u->s);        /* the same coded size keeps the kept picture */
    stream_release(u->s, true);
    u->s->wmb = wmb; u->s->hmb = hmb; u->s->n_slots = n_slots;
    u->s->frame_bytes = fj_frame_bytes(wmb, hmb);
    const size_t total = (size_t)n_slots * u->s->frame_bytes + 256;
    HIP_TRY(u->s->d_frames.alloc(total));
    HIP_TRY(hipMemsetAsync(u->s->d_frames, 0, total, u->e->stream));
    HIP_TRY(u->s->d_dbk.alloc(DBK_SCRATCH_BYTES(wmb * hmb)));
    HIP_TRY(hipMemsetAsync(u->s->d_dbk, 0, DBK_SCRATCH_BYTES(wmb * hmb), u->e->stream));
    if (u->s->motion) {                                    /* zeroed: every block invalid; the ages start from nothing */
        u->s->motion_bytes = h264k::motion_slot_bytes(wmb * hmb);
        HIP_TRY(u->s->d_motion.alloc((size_t)n_slots * u->s->motion_bytes));
        HIP_TRY(hipMemsetAsync(u->s->d_motion, 0, (size_t)n_slots * u->s->motion_bytes, u->e->stream));
        memset(u->s->slot_has, 0, sizeof(u->s->slot_has));
    }
    HIP_TRY(hipStreamSynchronize(u->e->stream));           /* the lanes do not order themselves behind this stream */
    u->s->last_lane = -1;
    return 0;
}

/* staging buffer for a frame job of up to `bytes`: recycled pinned memory of this stream, else a new allocation */
static int take_buffer(SinkUser *u, uint32_t bytes, PendingJob *out)
{
    PendingJob j;
    {
        std::lock_guard<std::mutex> ql(u->s->qmu);
        for (size_t i = 0; i < u->s->free_bufs.size(); i++)
            if (u->s->free_bufs[i].cap >= bytes) {
                j = std::move(u->s->free_bufs[i]);
                u->s->free_bufs.erase(u->s->free_bufs.begin() + (long)i);
                break;
            }
    }
    if (!j.host) {
        HIP_TRY(hipSetDevice(u->e->device));
        j.cap = bytes + 65536;                              /* pinned: recycled across pictures */
        HIP_TRY(j.host.alloc(j.cap, true));
    }
    *out = std::move(j);
    return 0;
}

/* The parser builds the next frame job directly in pinned staging memory (JobSink.acquire): nothing is copied on
 * the host between parsing and the H2D transfer. */
uint8_t *sink_acquire(void *user, uint32_t bytes)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    StreamCtx *s = u->s;
    if (s->acquired.host && s->acquired.cap >= bytes) return s->acquired.host;     /* previous picture was abandoned */
    if (s->acquired.host) {
        std::lock_guard<std::mutex> ql(s->qmu);
        s->free_bufs.push_back(std::move(s->acquired));
        s->acquired = PendingJob();
    }
    if (take_buffer(u, bytes, &s->acquired)) return nullptr;
    return s->acquired.host;
}

int sink_submit(void *user, const uint8_t *blob, uint32_t bytes)
{
    /* runs on the application's / the parser pool's threads, concurrently for different decoder instances: only the
     * stream's own queue lock is taken */
    SinkUser *u = static_cast<SinkUser *>(user);
    PendingJob j;
    if (u->s->acquired.host && blob == u->s->acquired.host) {
        j = std::move(u->s->acquired);
        u->s->acquired = PendingJob();
    } else {
        if (take_buffer(u, bytes, &j)) return -1;
        memcpy(j.host, blob, bytes);
    }
    j.bytes = bytes;
    size_t backlog;
    {
        std::lock_guard<std::mutex> ql(u->s->qmu);
        u->s->pending.push_back(std::move(j));
        backlog = u->s->pending.size();
    }
    /* An application that decodes without pulling pictures (frame skipping, decoding ahead) must not pile up pinned
     * staging buffers (worst-case sized, ~8 MB each for 1080p): past a few queued pictures the queues are enqueued on
     * the device — asynchronously, the caller does not wait for pixels — and the buffers recycle. */
    if (backlog >= MAX_QUEUED_PICTURES) {
        std::lock_guard<std::mutex> lk(u->e->mu);
        if (flush_locked(u->e, false)) return -1;
    }
    return 0;
}

/* how often a tripwire of the kernels has fired on this device, as last folded in (poll_errors runs wherever the host waits for the
 * device): no wait here.  Monotonic: a decoder compares it with the value it saw when it was created */
uint32_t sink_errors(void *user)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    return __atomic_load_n(&u->e->error_events, __ATOMIC_RELAXED);
}

/* A picture leaves the device.  Under the engine's mutex only what must be ordered: the instance's queued pictures are enqueued (not
 * awaited), the layout kernel — which writes pinned host memory itself — follows behind the picture's tick, an event of the INSTANCE is
 * recorded behind it.  The wait for that event — the pixels' whole latency: the tick's kernels, 3.1 MB over PCIe — happens outside the mutex, so that the other
 * instances of the process go on submitting, flushing and pulling meanwhile (rounds 1-4 held the mutex across a synchronous
 * copy: one picture at a time for the whole process).  Reference: the zero-copy alias of src/h264bsd_decoder.c:599-646. */
#ifndef OUT_EVENT_FLAGS
#define OUT_EVENT_FLAGS (hipEventDisableTiming | hipEventBlockingSync)    /* the waiter sleeps: under a CPU quota a spinning waiter takes the time the parser threads need */
#endif
static int out_begin(SinkUser *u, bool to_host, hipStream_t *st)          /* mutex held */
{
    /* Only an instance whose OWN pictures are still queued makes the engine enqueue (everything: ticks are formed across instances).
     * One whose pictures are all on the device already leaves the other instances' queues alone — when the pulls of one round run
     * beside the parsing of the next (h264bsdmiPullAndDecodePictureBatch), a flush per pull would cut that round's tick into as many
     * straggler ticks as there are pulls. */
    Engine *e = u->e;
    StreamCtx *s = u->s;
    bool mine;
    { std::lock_guard<std::mutex> ql(s->qmu); mine = !s->pending.empty(); }
    if (mine && flush_locked(e, false)) return -1;
    if (!mine) HIP_TRY(hipSetDevice(e->device));
    if (!s->out_ev) HIP_TRY(s->out_ev.create(OUT_EVENT_FLAGS));
    *st = e->stream;                                   /* device-resident output: on the engine's stream, which is behind every lane since the last flush */
    if (to_host) {
        /* A picture bound for host memory waits for the tick that made it (or a later one of its lane), not for whatever else the engine's
         * stream is behind: instances whose tick is done hand their pictures over while other instances' ticks still run.  Nothing the
         * device does later can touch the frame before the call returns — the instance's next job is submitted after that. */
        if (!e->out_stream) HIP_TRY(e->out_stream.create());
        if (s->last_lane >= 0) {
            hipEvent_t made = e->lanes[s->last_lane].ring[s->last_launch % Lane::RING];
            if (hipEventQuery(made) != hipSuccess) HIP_TRY(hipStreamWaitEvent(e->out_stream, made, 0));      /* (long done, usually: no barrier packet then) */
        }
        *st = e->out_stream;
    }
    return 0;
}
static int out_end_locked(SinkUser *u, hipStream_t st)  /* mutex held: the device's error words travel with the picture */
{
    hipLaunchKernelGGL(k_err_words, dim3(1), dim3(64), 0, st, u->e->d_err, u->e->h_err.dev());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(u->s->out_ev, st));
    return 0;
}
static int out_wait(SinkUser *u)                      /* mutex NOT held */
{
    if (hipEventSynchronize(u->s->out_ev) != hipSuccess) return -1;
    std::lock_guard<std::mutex> lk(u->e->mu);
    fold_errors(u->e);                                 /* (a later copy may have overwritten h_err meanwhile: it is as good or newer) */
    return 0;
}

int sink_fetch_begin(void *user, uint32_t slot)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    StreamCtx *s = u->s;
    std::lock_guard<std::mutex> lk(u->e->mu);
    hipStream_t st;
    s->out_slot = -1;
    if (slot >= s->n_slots || out_begin(u, true, &st)) return -1;
    s->retired_host.clear();
    if (!s->h_frame[slot] && s->h_frame[slot].alloc(s->frame_bytes, true) != hipSuccess) return -1;
    /* the layout kernel writes the host mirror itself: 16-byte pieces over the link run at 49 GB/s (tools/probes/d2h_probe.hip: as fast as
     * whole rows, and as fast as the copy engine moves one large buffer), and a picture costs ONE launch on the compute queue instead
     * of a kernel, two copy-engine transfers and the hand-overs between the engines */
    hipLaunchKernelGGL(h264k::k_detile, dim3(512, 1), dim3(256), 0, st, s->d_frames + (size_t)slot * s->frame_bytes,
                       s->h_frame[slot].dev(), s->wmb, s->hmb, (size_t)0, (size_t)0);
    if (hipGetLastError() != hipSuccess) return -1;
    if (out_end_locked(u, st)) return -1;
    s->out_slot = (int)slot;
    return 0;
}
uint8_t *sink_fetch_end(void *user)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    StreamCtx *s = u->s;
    if (s->out_slot < 0 || out_wait(u)) return nullptr;
    return s->h_frame[s->out_slot];
}
uint8_t *sink_fetch(void *user, uint32_t slot) { return sink_fetch_begin(user, slot) ? nullptr : sink_fetch_end(user); }

uint32_t *sink_fetch_converted(void *user, uint32_t slot, int fmt)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    StreamCtx *s = u->s;
    {
        std::lock_guard<std::mutex> lk(u->e->mu);
        hipStream_t st;
        if (slot >= s->n_slots || out_begin(u, true, &st)) return nullptr;
        const uint32_t w = s->wmb * 16, h = s->hmb * 16;
        const size_t bytes = (size_t)w * h * 4;
        if (!s->h_conv && s->h_conv.alloc(bytes, true) != hipSuccess) return nullptr;
        hipLaunchKernelGGL(h264k::k_convert_tiles, dim3(1024, 1), dim3(256), 0, st,
                           s->d_frames + (size_t)slot * s->frame_bytes, s->h_conv.dev(), s->wmb, s->hmb, fmt, (size_t)0, (size_t)0);
        if (hipGetLastError() != hipSuccess) return nullptr;
        if (out_end_locked(u, st)) return nullptr;
    }
    if (out_wait(u)) return nullptr;
    return s->h_conv;
}

void *sink_fetch_device(void *user, uint32_t slot, int fmt, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void **stream)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    StreamCtx *s = u->s;
    void *ret;
    {
        std::lock_guard<std::mutex> lk(u->e->mu);
        hipStream_t st;
        if (slot >= s->n_slots || out_begin(u, false, &st)) return nullptr;
        const uint32_t fw = s->wmb * 16, fh = s->hmb * 16;
        if (!w || !h || x0 + w > fw || y0 + h > fh) return nullptr;
        uint8_t *frame = s->d_frames + (size_t)slot * s->frame_bytes;
        /* frames are macroblock tiles in HBM: every picture that leaves is laid out by a kernel, the whole uncropped I420
         * frame by k_detile, everything else (window, conversion) by k_output */
        const size_t bytes = (size_t)fw * fh * 4;
        if (!s->d_conv && s->d_conv.alloc(bytes) != hipSuccess) return nullptr;
        if (fmt == 3 && x0 == 0 && y0 == 0 && w == fw && h == fh) {
            hipLaunchKernelGGL(h264k::k_detile, dim3(512, 1), dim3(256), 0, u->e->stream, frame, reinterpret_cast<uint8_t *>(s->d_conv.get()),
                               s->wmb, s->hmb, (size_t)0, (size_t)0);
        } else {
            const uint32_t n = fmt == 3 ? w * h * 3 / 8 : w * h / 4;
            hipLaunchKernelGGL(h264k::k_output, dim3((n + 255) / 256 < 2048 ? (n + 255) / 256 + 1 : 2048), dim3(256), 0, u->e->stream,
                               frame, reinterpret_cast<uint8_t *>(s->d_conv.get()), fw, fh, fmt, x0, y0, w, h);
        }
        ret = s->d_conv;
        if (out_end_locked(u, st)) return nullptr;
        if (stream) *stream = st;
    }
    if (out_wait(u)) return nullptr;
    return ret;
}

void sink_close(void *user)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    {
        std::lock_guard<std::mutex> lk(u->e->mu);
        hipSetDevice(u->e->device);
        reap_locked(u->e, true);
        hipStreamSynchronize(u->e->stream);
        if (u->e->out_stream) hipStreamSynchronize(u->e->out_stream);      /* (a pull that failed half way may have left its kernel behind) */
        fence_drop(u->e, u->s);
        kept_drop(u->e, u->s);
        stream_release(u->s);
        auto &v = u->e->streams;
        v.erase(std::remove(v.begin(), v.end(), u->s), v.end());
    }
    delete u->s;
    delete u;
}

/* ---- the next pictures of many instances into one caller-owned tensor (h264bsdmiNextOutputTensorBatch[Colour|Resize]) ---- */
/* five kernel families, each one kernel per dtype, layout, number of channels and REF; the channel order and the whole colour transform
 * are in the items (colour_item); filter, fit and border are run-time arguments */
enum { TK_OUT, TK_RESIZE, TK_AA, TK_ROI, TK_REMAP };
template <int DT, int L, int C> static const void *tensor_kernel_of(int kind, bool ref)
{
#define TK_CASE(K, NAME) \
    case K: return ref ? reinterpret_cast<const void *>(&h264k::NAME<DT, L, C, true>) : reinterpret_cast<const void *>(&h264k::NAME<DT, L, C, false>)
    switch (kind) {
    TK_CASE(TK_OUT, k_tensor_out);
    TK_CASE(TK_RESIZE, k_tensor_resize);
    TK_CASE(TK_AA, k_tensor_aa);
    TK_CASE(TK_ROI, k_tensor_roi);
    TK_CASE(TK_REMAP, k_tensor_remap);
    }
#undef TK_CASE
    return nullptr;
}
/* the channels of a spec's slice and its size in bytes */
static size_t spec_channels(const h264bsdmi_tensor_spec &t) { return t.channels == h264k::TO_Y ? 1 : t.channels >= h264k::TO_RGBA ? 4 : 3; }
static size_t spec_slice_bytes(const h264bsdmi_tensor_spec &t)
{
    return spec_channels(t) * t.width * t.height * (t.dtype == h264k::TO_U8 ? 1 : t.dtype == h264k::TO_F16 ? 2 : 4);
}
template <int DT> static const void *tensor_kernel_dt(int kind, bool ref, uint32_t layout, size_t C)
{
    if (layout == h264k::TO_NCHW) {
        if (C == 1) return tensor_kernel_of<DT, h264k::TO_NCHW, 1>(kind, ref);
        if (C == 3) return tensor_kernel_of<DT, h264k::TO_NCHW, 3>(kind, ref);
    } else if (layout == h264k::TO_NHWC) {
        if (C == 1) return tensor_kernel_of<DT, h264k::TO_NHWC, 1>(kind, ref);
        if (C == 3) return tensor_kernel_of<DT, h264k::TO_NHWC, 3>(kind, ref);
        return tensor_kernel_of<DT, h264k::TO_NHWC, 4>(kind, ref);
    }
    return nullptr;
}
static const void *tensor_kernel(int kind, const h264bsdmi_tensor_spec &t, bool ref)
{
    switch (t.dtype) {
    case h264k::TO_U8: return tensor_kernel_dt<h264k::TO_U8>(kind, ref, t.layout, spec_channels(t));
    case h264k::TO_F16: return tensor_kernel_dt<h264k::TO_F16>(kind, ref, t.layout, spec_channels(t));
    case h264k::TO_F32: return tensor_kernel_dt<h264k::TO_F32>(kind, ref, t.layout, spec_channels(t));
    }
    return nullptr;
}

/* The colour map of one picture's item (matrix, range): per output channel c the affine map of the 8-bit (Y, Cb - 128, Cr - 128) to
 * the value written, and the clamp bounds of [0, 1] under the output scale (U8: 255 v; floats: (v - mean[c]) / std[c]), folded in
 * double.  H264BSDMI_MATRIX_REFERENCE: the reference's integer BT.601, (298 (Y - 16) + 409 (Cr - 128) + 128) >> 8 and its relatives
 * clamped to 0..255, on the 255 scale whatever the dtype: coefficients / 256, offset (128 - 16 * 298) / 256, bounds [0, 255].  Every
 * partial sum of the kernel's FMA chain is then a multiple of 1/256 below 2^10, so the chain is exact, and the clamped value truncated
 * is the reference's arithmetic shift.  bgr: the channel order for k_tensor_out, which uses yuv_pixel instead. */
static void colour_item(h264k::TensorItem &it, const h264bsdmi_tensor_spec &t, uint32_t matrix, uint32_t range)
{
    const bool bgr = t.channels == h264k::TO_BGR || t.channels == h264k::TO_BGRA;
    if (matrix == H264BSDMI_MATRIX_REFERENCE) {
        static const float R[3][3] = { { 298, 0, 409 }, { 298, -100, -208 }, { 298, 516, 0 } };     /* R, G, B of (Y, Cb, Cr) */
        for (int c = 0; c < 3; c++) {
            for (int j = 0; j < 3; j++) it.k[c][j] = t.channels == h264k::TO_Y ? (j == 0 ? 1.0f : 0.0f) : R[bgr ? 2 - c : c][j] / 256.0f;
            it.k[c][3] = t.channels == h264k::TO_Y ? 0.0f : (128.0f - 16.0f * 298.0f) / 256.0f;
            it.lo[c] = 0.0f;
            it.hi[c] = 255.0f;
        }
        it.bgr = bgr;
        return;
    }
    static const double K[][2] = { { 0.299, 0.114 }, { 0.2126, 0.0722 }, { 0.2627, 0.0593 }, { 0.30, 0.11 }, { 0.212, 0.087 } };  /* Kr, Kb */
    const double kr = K[matrix - H264BSDMI_MATRIX_BT601][0], kb = K[matrix - H264BSDMI_MATRIX_BT601][1], kg = 1.0 - kr - kb;
    const bool full = range == H264BSDMI_RANGE_FULL;
    const double sy = full ? 1.0 / 255 : 1.0 / 219, oy = full ? 0.0 : -16.0 / 219;      /* Y' = sy Y + oy */
    const double sc = full ? 1.0 / 255 : 1.0 / 224;                                      /* Pb = sc (Cb - 128), Pr = sc (Cr - 128) */
    const double rgb[3][3] = { { 1, 0, 2 * (1 - kr) }, { 1, -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg }, { 1, 2 * (1 - kb), 0 } };
    const double luma[3] = { 1, 0, 0 };
    for (int c = 0; c < 3; c++) {
        const double *m = t.channels == h264k::TO_Y ? luma : rgb[bgr ? 2 - c : c];         /* (Y', Pb, Pr) -> the value of output channel c */
        const double scale = t.dtype == h264k::TO_U8 ? 255.0 : 1.0 / t.std[c], shift = t.dtype == h264k::TO_U8 ? 0.0 : -t.mean[c] / (double)t.std[c];
        it.k[c][0] = (float)(m[0] * sy * scale);
        it.k[c][1] = (float)(m[1] * sc * scale);
        it.k[c][2] = (float)(m[2] * sc * scale);
        it.k[c][3] = (float)(m[0] * oy * scale + shift);
        const double lo = shift, hi = scale + shift;
        it.lo[c] = (float)std::min(lo, hi);
        it.hi[c] = (float)std::max(lo, hi);
    }
}

/* The three steps every pull shares, under the engine's mutex.  pull_begin_locked: the instances' queued jobs are enqueued, once for
 * the batch; the current half of the item staging is made large enough for n_items and free. */
static int pull_begin_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_items)
{
    bool mine = false;
    for (uint32_t i = 0; i < n && !mine; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        std::lock_guard<std::mutex> ql(s->qmu);
        mine = !s->pending.empty();
    }
    if (mine && flush_locked(e, false)) return -1;
    HIP_TRY(e->titems.reserve(n_items, 256));
    return 0;
}
/* st waits for the tick that produced each picture (deduplicated per lane launch) */
static int pull_wait_pictures(Engine *e, uint32_t n, const SinkTensorPic *pics, hipStream_t st)
{
    std::vector<std::pair<int, unsigned long long>> waited;
    for (uint32_t i = 0; i < n; i++) {
        const StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        if (s->last_lane < 0) continue;
        const std::pair<int, unsigned long long> key(s->last_lane, s->last_launch);
        if (std::find(waited.begin(), waited.end(), key) != waited.end()) continue;
        hipEvent_t made = e->lanes[s->last_lane].ring[s->last_launch % Lane::RING];
        if (hipEventQuery(made) != hipSuccess) HIP_TRY(hipStreamWaitEvent(st, made, 0));
        waited.push_back(key);
    }
    return 0;
}
/* behind the pull's launch on st: the staging half is guarded and handed on, the device's error words travel with the data, and a
 * fence is handed to every instance */
static int pull_end_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, hipStream_t st, hipEvent_t *fence_ev)
{
    HIP_TRY(e->titems.submit(st));
    hipLaunchKernelGGL(k_err_words, dim3(1), dim3(64), 0, st, e->d_err, e->h_err.dev());
    HIP_TRY(hipGetLastError());
    Fence *fc;
    if (e->fences.empty()) {
        std::unique_ptr<Fence> fresh(new Fence());
        HIP_TRY(fresh->ev.create(hipEventDisableTiming));
        fc = fresh.release();
    } else { fc = e->fences.back(); e->fences.pop_back(); }
    HIP_TRY(hipEventRecord(fc->ev, st));
    for (uint32_t i = 0; i < n; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        fence_unref(e, s);
        s->fence = fc; fc->refs++;
    }
    *fence_ev = fc->ev;
    return 0;
}

/* ---- what the pulls (whole pictures, regions, motion regions, coordinate maps, region statistics) share, under the engine's mutex ---- */
static const StreamCtx *pic_stream(const SinkTensorPic &p) { return static_cast<SinkUser *>(p.sink->user)->s; }
/* The refusals per picture: a slot of its instance, frames, a window inside the coded size; for pixels also a matrix that agrees
 * with ref (one kernel: every picture of the call takes the reference conversion, or none) and an even window.  motion: the side
 * information instead of the frames, no matrix and no parity rule. */
static bool pull_pictures_ok(uint32_t n, const SinkTensorPic *pics, bool ref, bool motion)
{
    for (uint32_t i = 0; i < n; i++) {
        const SinkTensorPic &p = pics[i];
        const StreamCtx *s = pic_stream(p);
        if (p.slot >= s->n_slots || !p.w || !p.h || p.x0 + p.w > s->wmb * 16 || p.y0 + p.h > s->hmb * 16) return false;
        if (motion ? !s->motion || !s->d_motion : !s->d_frames) return false;
        if (motion) continue;
        if ((p.matrix == H264BSDMI_MATRIX_REFERENCE) != ref || (!ref && (p.matrix < H264BSDMI_MATRIX_BT601 || p.matrix > H264BSDMI_MATRIX_SMPTE240)))
            return false;
        if ((p.x0 | p.y0 | p.w | p.h) & 1u) return false;
    }
    return true;
}
/* an inner rectangle (left, top, w, h) of a width x height slice */
static bool pull_box_ok(const uint32_t *box, uint32_t width, uint32_t height)
{
    return box[2] && box[3] && box[0] + box[2] <= width && box[1] + box[3] <= height;
}
/* the refusals per region: a picture of the call, a box within the limits of the interface, an inner rectangle inside the slice */
static bool pull_regions_ok(uint32_t n, uint32_t n_regs, const SinkRegion *regs, uint32_t width, uint32_t height)
{
    for (uint32_t r = 0; r < n_regs; r++) {
        const SinkRegion &g = regs[r];
        if (g.pic >= n || !g.w || !g.h || g.w > 16384u || g.h > 16384u || abs(g.x) > 16384 || abs(g.y) > 16384) return false;
        if (!pull_box_ok(g.box, width, height)) return false;
    }
    return true;
}
/* the item of one picture: its frame, its window and its colour map, into slice `index` of the tensor */
static h264k::TensorItem picture_item(const SinkTensorPic &p, const h264bsdmi_tensor_spec &t, size_t index)
{
    const StreamCtx *s = pic_stream(p);
    h264k::TensorItem it{ s->d_frames + (size_t)p.slot * s->frame_bytes, static_cast<uint8_t *>(t.data) + index * spec_slice_bytes(t),
                          s->wmb, p.x0, p.y0, p.w, p.h, 0u };
    colour_item(it, t, p.matrix, p.range);
    return it;
}
static void copy3(float *d, const float *s) { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; }
/* The call's pad in [0, 1] per channel, folded in double, ONE rule for every family (their bit-for-bit equalities rest on it).  pad:
 * under the output's scale, written where there is nothing to interpolate (U8 floor(255 pad + 0.5), floats (pad - mean) / std).  spad:
 * around the picture, under the scale of the samples that are interpolated — REF the 8-bit value whatever the dtype, else 255 pad (U8) / as pad. */
struct PullPad { float pad[3], spad[3]; };
static PullPad fold_pad(const float *pad, uint32_t dtype, const float *mean, const float *std, bool ref)
{
    PullPad pp;
    for (int c = 0; c < 3; c++) {
        const double q = std::floor(255.0 * pad[c] + 0.5), nrm = ((double)pad[c] - mean[c]) / std[c];
        pp.pad[c] = dtype == h264k::TO_U8 ? (float)q : (float)nrm;
        pp.spad[c] = ref ? (float)q : dtype == h264k::TO_U8 ? (float)(255.0 * pad[c]) : (float)nrm;
    }
    return pp;
}
/* grid.x walks the slice's tiles of cols x rows (per_block of them at a time in a workgroup), at most 1024 workgroups; grid.y = the items */
static dim3 pull_grid(uint32_t width, uint32_t height, uint32_t cols, uint32_t rows, uint32_t n_items, uint32_t per_block = 1)
{
    const uint32_t tiles = (width + cols - 1u) / cols * ((height + rows - 1u) / rows);
    return dim3(std::min((tiles + per_block - 1u) / per_block, 1024u), n_items);
}
/* behind the filled items: st waits for the pictures' ticks, the launches of 256-lane workgroups one behind the other (ONE for most
 * pulls; where there are two the second reads what the first wrote), the fence and the error words behind the last */
struct PullLaunch { const void *fn; dim3 grid; void *kargs; };
static int pull_launch_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, hipStream_t st, std::initializer_list<PullLaunch> launches,
                              hipEvent_t *fence_ev)
{
    if (pull_wait_pictures(e, n, pics, st)) return -1;
    for (const PullLaunch &l : launches) {
        void *args[] = { l.kargs };
        HIP_TRY(hipLaunchKernel(l.fn, l.grid, dim3(256), args, 0, st));
    }
    return pull_end_locked(e, n, pics, st, fence_ev);
}

/* The pulls below take the same steps in the same order, without host waits: the refusals; pull_begin_locked;
 * the items and the arguments are filled; pull_launch_locked: st waits for each picture's producing tick, ONE launch lays out every
 * item, and a fence recorded behind it is handed to every instance: lane_launch makes an instance's next tick wait for it, and the
 * frame buffers are not cleared or freed before it has passed (fence_drop).  *fence_ev: the fence's event. */
/* h264bsdmiNextOutputTensorBatchResize with any filter and fit but resize = 1's own bilinear stretch: one AaItem per picture,
 * k_tensor_aa */
static int aa_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, const h264bsdmi_tensor_spec &t, uint32_t chroma,
                         const h264bsdmi_resize_spec &rs, hipStream_t st, hipEvent_t *fence_ev)
{
    const bool ref = pics[0].matrix == H264BSDMI_MATRIX_REFERENCE;
    if (!t.resize || rs.filter > H264BSDMI_FILTER_BICUBIC_AA || rs.fit > H264BSDMI_FIT_LETTERBOX) return -1;
    const void *fn = tensor_kernel(TK_AA, t, ref);
    if (!fn || n > 65535u) return -1;                                   /* grid.y */
    if (!pull_pictures_ok(n, pics, ref, false)) return -1;
    for (uint32_t i = 0; i < n; i++)
        if (!pull_box_ok(pics[i].box, t.width, t.height)) return -1;
    if (pull_begin_locked(e, n, pics, n)) return -1;
    h264k::AaItem *items = e->titems.host<h264k::AaItem>();
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t *box = pics[i].box;
        items[i] = h264k::AaItem{ picture_item(pics[i], t, pics[i].index), box[0], box[1], box[2], box[3] };
    }
    h264k::AaArgs aargs{ e->titems.dev<h264k::AaItem>(), t.width, t.height, chroma, rs.filter, {}, {}, {} };
    copy3(aargs.mean, t.mean); copy3(aargs.std, t.std); copy3(aargs.pad, fold_pad(rs.pad, t.dtype, t.mean, t.std, ref).pad);
    return pull_launch_locked(e, n, pics, st, { { fn, pull_grid(t.width, t.height, h264k::TAA_COLS, h264k::TAA_ROWS, n), &aargs } }, fence_ev);
}

/* h264bsdmiNextOutputTensorBatch[Colour|Resize]: one TensorItem per picture, k_tensor_out without resize, k_tensor_resize for
 * resize = 1's own bilinear stretch; every other filter and fit is aa_out_locked's */
static int tensor_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, const h264bsdmi_tensor_spec &t, uint32_t chroma,
                             const h264bsdmi_resize_spec *rs, hipStream_t st, hipEvent_t *fence_ev)
{
    if (rs && (rs->filter != H264BSDMI_FILTER_BILINEAR || rs->fit != H264BSDMI_FIT_STRETCH))
        return aa_out_locked(e, n, pics, t, chroma, *rs, st, fence_ev);
    const bool ref = pics[0].matrix == H264BSDMI_MATRIX_REFERENCE;
    const void *fn = tensor_kernel(t.resize ? TK_RESIZE : TK_OUT, t, ref);
    if (!fn || n > 65535u) return -1;                                   /* grid.y */
    if (!pull_pictures_ok(n, pics, ref, false)) return -1;
    if (pull_begin_locked(e, n, pics, n)) return -1;
    h264k::TensorItem *items = e->titems.host<h264k::TensorItem>();
    for (uint32_t i = 0; i < n; i++) items[i] = picture_item(pics[i], t, pics[i].index);
    h264k::TensorArgs targs{ e->titems.dev<h264k::TensorItem>(), t.width, t.height, chroma, {}, {} };
    copy3(targs.mean, t.mean); copy3(targs.std, t.std);
    /* k_tensor_out: a wavefront per unit of 64 x 16, four to a workgroup */
    const dim3 grid = t.resize ? pull_grid(t.width, t.height, h264k::TCR_COLS, h264k::TCR_ROWS, n) : pull_grid(t.width, t.height, 64, 16, n, 4);
    return pull_launch_locked(e, n, pics, st, { { fn, grid, &targs } }, fence_ev);
}

/* h264bsdmiOutputTensorRegions: the items are the n_regs regions, each a box of one of the n pictures, which were popped earlier and
 * are read where they lie; k_tensor_roi for every filter and fit.  The pictures are still one per instance, so the producers'
 * events and the fence are taken once per instance however many regions name it. */
static int regions_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                              const h264bsdmi_tensor_spec &t, uint32_t chroma, const h264bsdmi_resize_spec &rs, hipStream_t st,
                              hipEvent_t *fence_ev)
{
    const bool ref = pics[0].matrix == H264BSDMI_MATRIX_REFERENCE;
    if (!t.resize || rs.filter > H264BSDMI_FILTER_BICUBIC_AA || rs.fit > H264BSDMI_FIT_LETTERBOX) return -1;
    const void *fn = tensor_kernel(TK_ROI, t, ref);
    if (!fn || n_regs > 65535u) return -1;                              /* grid.y */
    if (!pull_pictures_ok(n, pics, ref, false) || !pull_regions_ok(n, n_regs, regs, t.width, t.height)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::RoiItem *items = e->titems.host<h264k::RoiItem>();
    std::vector<h264k::TensorItem> of_pic(n);                           /* the colour map once per picture */
    for (uint32_t i = 0; i < n; i++) of_pic[i] = picture_item(pics[i], t, 0);
    for (uint32_t r = 0; r < n_regs; r++) {
        const SinkRegion &g = regs[r];
        items[r] = h264k::RoiItem{ of_pic[g.pic], g.x, g.y, g.w, g.h, g.box[0], g.box[1], g.box[2], g.box[3] };
        items[r].t.dst += g.index * spec_slice_bytes(t);
    }
    h264k::RoiArgs rargs{ e->titems.dev<h264k::RoiItem>(), t.width, t.height, chroma, rs.filter, {}, {}, {}, {} };
    const PullPad pp = fold_pad(rs.pad, t.dtype, t.mean, t.std, ref);
    copy3(rargs.mean, t.mean); copy3(rargs.std, t.std); copy3(rargs.pad, pp.pad); copy3(rargs.spad, pp.spad);
    return pull_launch_locked(e, n, pics, st, { { fn, pull_grid(t.width, t.height, h264k::TAA_COLS, h264k::TAA_ROWS, n_regs), &rargs } }, fence_ev);
}

/* h264bsdmiOutputMotionRegions: the regions of regions_out_locked, read from the side information beside each picture's frame
 * buffer instead of from its pixels, by one k_motion_roi launch.  The same ordering: behind the ticks that made the pictures
 * (k_motion_keep runs in front of a tick's ring event), and the same fence, so that the next picture decoded into one of these
 * slots — and the k_motion_keep behind it — waits for this launch. */
static int motion_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                             const h264bsdmi_motion_spec &m, hipStream_t st, hipEvent_t *fence_ev)
{
    static const void *const fns[2][2] = {
        { reinterpret_cast<const void *>(&h264k::k_motion_roi<h264k::TO_F16, h264k::TO_NCHW>), reinterpret_cast<const void *>(&h264k::k_motion_roi<h264k::TO_F16, h264k::TO_NHWC>) },
        { reinterpret_cast<const void *>(&h264k::k_motion_roi<h264k::TO_F32, h264k::TO_NCHW>), reinterpret_cast<const void *>(&h264k::k_motion_roi<h264k::TO_F32, h264k::TO_NHWC>) } };
    const uint32_t all = H264BSDMI_MOTION_PLANE_MV | H264BSDMI_MOTION_PLANE_VALID | H264BSDMI_MOTION_PLANE_AGE | H264BSDMI_MOTION_PLANE_QP;
    if (!m.data || !m.width || !m.height || m.layout > h264k::TO_NHWC || (m.dtype != h264k::TO_F16 && m.dtype != h264k::TO_F32) ||
        !m.planes || (m.planes & ~all) || m.sampler > H264BSDMI_MOTION_AREA || m.units > H264BSDMI_MOTION_UNITS_OUTPUT || m.per_picture > 1u) return -1;
    if (n_regs > 65535u) return -1;                                     /* grid.y */
    if (!pull_pictures_ok(n, pics, false, true) || !pull_regions_ok(n, n_regs, regs, m.width, m.height)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::MotionItem *items = e->titems.host<h264k::MotionItem>();
    const size_t C = ((m.planes & H264BSDMI_MOTION_PLANE_MV) ? 2 : 0) + ((m.planes & H264BSDMI_MOTION_PLANE_VALID) ? 1 : 0) +
                     ((m.planes & H264BSDMI_MOTION_PLANE_AGE) ? 1 : 0) + ((m.planes & H264BSDMI_MOTION_PLANE_QP) ? 1 : 0);
    const size_t slice = C * m.width * m.height * (m.dtype == h264k::TO_F16 ? 2 : 4);
    for (uint32_t r = 0; r < n_regs; r++) {
        const SinkRegion &g = regs[r];
        const SinkTensorPic &p = pics[g.pic];
        const StreamCtx *s = pic_stream(p);
        items[r] = h264k::MotionItem{ s->d_motion + (size_t)p.slot * s->motion_bytes, static_cast<uint8_t *>(m.data) + g.index * slice,
                                      s->wmb, s->hmb, p.x0, p.y0, p.w, p.h, g.x, g.y, g.w, g.h, g.box[0], g.box[1], g.box[2], g.box[3] };
    }
    h264k::MotionArgs margs{ e->titems.dev<h264k::MotionItem>(), m.width, m.height, m.planes, m.sampler, m.units, m.per_picture };
    return pull_launch_locked(e, n, pics, st, { { fns[m.dtype == h264k::TO_F32][m.layout],
                                                  pull_grid(m.width, m.height, h264k::TAA_COLS, h264k::TAA_ROWS, n_regs), &margs } }, fence_ev);
}

/* The scratch in which the row bands of k_region_stats, k_region_change, k_region_shift and k_corner_points meet (Engine.d_stats), allocated at its first
 * use for the largest of the four (two records, a partial SAD surface, a band's best points); two launches must not use it at once: st waits for the event behind the previous one
 * (banded_launch_locked, the one caller, records stats_ev behind its launch). */
static int stats_scratch_locked(Engine *e, hipStream_t st, uint32_t **tickets, uint8_t **partials)
{
    const size_t ticket_bytes = h264k::STATS_MAX_PARTIALS * sizeof(uint32_t);
    if (!e->d_stats) {
        DeviceMem<uint8_t> fresh;
        HIP_TRY(e->stats_ev.create(hipEventDisableTiming));
        HIP_TRY(fresh.alloc(ticket_bytes + (size_t)h264k::STATS_MAX_PARTIALS * std::max({ h264k::STATS_MAX_RECORD, h264k::CHANGE_MAX_RECORD, h264k::SHIFT_MAX_PARTIAL, h264k::CORNER_PARTIAL })));
        HIP_TRY(hipMemsetAsync(fresh, 0, ticket_bytes, st));
        e->d_stats = std::move(fresh);
    } else HIP_TRY(hipStreamWaitEvent(st, e->stats_ev, 0));
    *tickets = reinterpret_cast<uint32_t *>(e->d_stats.get());
    *partials = e->d_stats.get() + ticket_bytes;
    return 0;
}

/* What the picture-analysis pulls below share (region statistics, change statistics, region shift, cell maps and cell boxes).
 * region_clip: box ∩ window of region g of picture p in luma samples of the coded frame, all zero when empty, and its height in
 * macroblock rows (0 when empty). */
struct RegionClip { uint32_t x0, y0, x1, y1, mb_rows; };
static RegionClip region_clip(const SinkTensorPic &p, const SinkRegion &g)
{
    const int64_t bx0 = std::max<int64_t>(g.x, 0), bx1 = std::min<int64_t>((int64_t)g.x + g.w, p.w);
    const int64_t by0 = std::max<int64_t>(g.y, 0), by1 = std::min<int64_t>((int64_t)g.y + g.h, p.h);
    RegionClip c{ 0u, 0u, 0u, 0u, 0u };
    if (bx1 > bx0 && by1 > by0) {
        c.x0 = p.x0 + (uint32_t)bx0; c.x1 = p.x0 + (uint32_t)bx1;
        c.y0 = p.y0 + (uint32_t)by0; c.y1 = p.y0 + (uint32_t)by1;
        c.mb_rows = ((c.y1 + 15u) >> 4) - (c.y0 >> 4);
    }
    return c;
}
/* the row bands per region of a banded launch: one value for the launch, about 1024 workgroups in all, at most the macroblock rows of
 * the tallest box ∩ window, 1 from 1024 regions on */
static uint32_t band_count(uint32_t n_regs, uint32_t tallest)
{
    return n_regs >= h264k::STATS_MAX_PARTIALS ? 1u : std::min(h264k::STATS_MAX_PARTIALS / n_regs, std::max(tallest, 1u));
}
/* every picture's instance has a kept picture of its coded size (api.c names only instances that have one) */
static bool kept_pictures_ok(uint32_t n, const SinkTensorPic *pics)
{
    for (uint32_t i = 0; i < n; i++) {
        const StreamCtx *s = pic_stream(pics[i]);
        if (!s->d_kept || s->kept_wmb != s->wmb || s->kept_hmb != s->hmb) return false;
    }
    return true;
}
/* What the item of region g reads: the frame of its picture, the kept picture of its instance (null without one), box ∩ window, the
 * window itself and the box's origin, which may be negative or beyond the frame, all in luma samples of the coded frame.  *tallest,
 * where the launch is banded, takes the clip's macroblock rows */
struct RegionSource { const uint8_t *frame; const uint8_t *kept; uint32_t wmb; RegionClip c; uint32_t wx0, wy0, wx1, wy1; int32_t ox, oy; const uint8_t *spread; };
static RegionSource region_source(const SinkTensorPic *pics, const SinkRegion &g, uint32_t *tallest = nullptr)
{
    const SinkTensorPic &p = pics[g.pic];
    const StreamCtx *s = pic_stream(p);
    const RegionClip c = region_clip(p, g);
    if (tallest) *tallest = std::max(*tallest, c.mb_rows);
    return RegionSource{ s->d_frames + (size_t)p.slot * s->frame_bytes, s->d_kept.get(), s->wmb, c, p.x0, p.y0, p.x0 + p.w, p.y0 + p.h,
                         (int32_t)p.x0 + g.x, (int32_t)p.y0 + g.y, s->d_spread.get() };
}
/* the refusals every analysis pull makes behind those of its own spec: regions that fit grid.y, pictures, regions, and with vs_kept
 * the kept pictures */
static bool analysis_regions_ok(uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs, bool vs_kept)
{
    if (n_regs > 65535u) return false;                                  /* grid.y */
    if (!pull_pictures_ok(n, pics, true, false) || !pull_regions_ok(n, n_regs, regs, 1u, 1u)) return false;
    return !vs_kept || kept_pictures_ok(n, pics);
}
/* A grid of cols x rows square cells of side `cell` over rectangles of rect_w x rect_h luma samples, one workgroup each: the cell side
 * as a shift (min_shift .. max_shift), the rectangles per row of rectangles and per region; refused: a side that is none of these, a
 * grid beyond max_grid either way, more than max_workgroups in the launch.  Both callers ask behind analysis_regions_ok, where the
 * side and the grid used to be refused ahead of it: every refusal returns -1 with nothing done, so the order does not show */
struct CellLimits { uint32_t min_shift, max_shift, rect_w, rect_h, max_grid, max_workgroups; };
static const CellLimits CELLS_LIMITS{ 2u, 6u, h264k::CELLS_RECT_W, h264k::CELLS_RECT_H, h264k::CELLS_MAX_GRID, h264k::CELLS_MAX_WORKGROUPS };
static const CellLimits FLOW_LIMITS{ h264k::FLOW_MIN_SHIFT, h264k::FLOW_MAX_SHIFT, h264k::FLOW_RECT_W, h264k::FLOW_RECT_H, h264k::FLOW_MAX_GRID,
                                     h264k::FLOW_MAX_WORKGROUPS };
struct CellGrid { uint32_t shift, rects_x, rects; };
static bool cell_grid(uint32_t cell, uint32_t cols, uint32_t rows, uint32_t n_regs, const CellLimits &lim, CellGrid *g)
{
    uint32_t shift = lim.min_shift;
    while (shift < lim.max_shift && (1u << shift) != cell) shift++;
    if ((1u << shift) != cell || !cols || cols > lim.max_grid || !rows || rows > lim.max_grid) return false;
    const uint32_t rw = lim.rect_w >> shift, rh = lim.rect_h >> shift;
    const uint32_t rects_x = (cols + rw - 1u) / rw, rects = rects_x * ((rows + rh - 1u) / rh);
    *g = CellGrid{ shift, rects_x, rects };
    return (uint64_t)rects * n_regs <= lim.max_workgroups;
}
/* k_region_shift or k_cell_shift of a radius: from radius SHIFT_QUADS_FROM on a thread takes SHIFT_QUADS quads of displacements per
 * template dword, below that one: as measured, each is the faster on its side (docs/EXPERIMENTS.md, "Region shift") */
template <typename Args> static const void *shift_kernel_of(uint32_t radius, void (*quads)(Args), void (*one)(Args))
{
    return reinterpret_cast<const void *>(radius >= h264k::SHIFT_QUADS_FROM ? quads : one);
}
/* the refusals of `source` and `bins` (0, or a power of two 16 .. 256); *shift = 8 - log2 bins, 0 without a histogram */
static bool source_bins_ok(uint32_t source, uint32_t bins, uint32_t *shift)
{
    uint32_t sh = 8u;
    while (sh > 0u && (256u >> sh) != bins) sh--;                           /* bins == 256 >> sh; sh == 0 also stands for "no such shift" */
    *shift = bins ? sh : 0u;
    return source <= H264BSDMI_STATS_RGB && (!bins || (bins >= 16u && (256u >> sh) == bins));
}
/* k_region_stats or k_region_change of a source, with or without the histogram */
template <int SRC> static const void *banded_kernel_of(bool change, bool hist)
{
    if (change) return hist ? reinterpret_cast<const void *>(&h264k::k_region_change<SRC, true>) : reinterpret_cast<const void *>(&h264k::k_region_change<SRC, false>);
    return hist ? reinterpret_cast<const void *>(&h264k::k_region_stats<SRC, true>) : reinterpret_cast<const void *>(&h264k::k_region_stats<SRC, false>);
}
static const void *banded_kernel(bool change, uint32_t source, bool hist)
{
    const void *const fns[3] = { banded_kernel_of<h264k::ST_Y>(change, hist), banded_kernel_of<h264k::ST_YCBCR>(change, hist),
                                 banded_kernel_of<h264k::ST_RGB>(change, hist) };
    return fns[source];
}

/* launches that touch kept pictures run one behind the other, whatever streams they are on (Engine.kept_ev) */
static int kept_order_begin(Engine *e, hipStream_t st)
{
    if (!e->kept_ev) HIP_TRY(e->kept_ev.create(hipEventDisableTiming));
    if (e->kept_recorded) HIP_TRY(hipStreamWaitEvent(st, e->kept_ev, 0));
    return 0;
}
static int kept_order_end(Engine *e, hipStream_t st)
{
    HIP_TRY(hipEventRecord(e->kept_ev, st));
    e->kept_recorded = true;
    return 0;
}

/* Behind the filled items of k_region_stats, k_region_change, k_region_shift and k_corner_points: ONE launch of S = band_count row bands per region.
 * With S > 1 the bands meet in the engine's scratch (Engine.d_stats), which two launches must not use at once: st waits for the event
 * behind the previous such launch, and stats_ev is recorded behind this one.  kept: the launch reads kept pictures, whose ordering
 * encloses it.  The same ordering and fence as the other pulls. */
template <typename Args>
static int banded_launch_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, hipStream_t st, const void *fn, uint32_t n_regs,
                                uint32_t tallest, Args *kargs, bool kept, hipEvent_t *fence_ev)
{
    const uint32_t S = band_count(n_regs, tallest);
    if (S > 1u && stats_scratch_locked(e, st, &kargs->tickets, &kargs->partials)) return -1;
    if (kept && kept_order_begin(e, st)) return -1;
    if (pull_launch_locked(e, n, pics, st, { { fn, dim3(S, n_regs), kargs } }, fence_ev)) return -1;
    if (S > 1u) HIP_TRY(hipEventRecord(e->stats_ev, st));
    return kept ? kept_order_end(e, st) : 0;
}

/* h264bsdmiOutputRegionStats: one StatsItem per region, box ∩ window in luma samples of the coded frame, ONE banded k_region_stats
 * launch */
static int stats_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                            const h264bsdmi_stats_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    uint32_t shift;
    if (!sp.data || (reinterpret_cast<uintptr_t>(sp.data) & 7u) || sp.crop > 1u || !source_bins_ok(sp.source, sp.bins, &shift)) return -1;
    if (!analysis_regions_ok(n, pics, n_regs, regs, false)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::StatsItem *items = e->titems.host<h264k::StatsItem>();
    const uint32_t stride = h264k::stats_record_bytes(sp.source == H264BSDMI_STATS_Y ? 1u : 3u, sp.bins);
    uint32_t tallest = 0u;
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r], &tallest);
        items[r] = h264k::StatsItem{ s.frame, static_cast<uint8_t *>(sp.data) + (size_t)regs[r].index * stride, s.wmb, s.c.x0, s.c.y0, s.c.x1, s.c.y1 };
    }
    h264k::StatsArgs sargs{ e->titems.dev<h264k::StatsItem>(), nullptr, nullptr, sp.bins, shift };
    return banded_launch_locked(e, n, pics, st, banded_kernel(false, sp.source, sp.bins != 0u), n_regs, tallest, &sargs, false, fence_ev);
}

/* h264bsdmiKeepCurrentPictures: the frame buffer of every picture into its instance's kept-picture buffer (allocated here at the first
 * keep, and at the first after sink_configure dropped it for a change of size), ONE k_keep launch, the same ordering and fence as the
 * pulls: the next picture decoded into one of these slots waits for the copy. */
static int keep_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, hipStream_t st, hipEvent_t *fence_ev)
{
    if (n > 65535u) return -1;                                          /* grid.y */
    if (!pull_pictures_ok(n, pics, true, false)) return -1;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t k = 0; k < i; k++)
            if (pics[k].sink == pics[i].sink) return -1;                /* one kept picture per instance */
    if (pull_begin_locked(e, n, pics, n)) return -1;
    if (kept_order_begin(e, st)) return -1;
    h264k::KeepItem *items = e->titems.host<h264k::KeepItem>();
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        if (!s->d_kept) {
            HIP_TRY(s->d_kept.alloc(s->frame_bytes));
            s->kept_wmb = s->wmb; s->kept_hmb = s->hmb;
        }
        items[i] = h264k::KeepItem{ s->d_frames + (size_t)pics[i].slot * s->frame_bytes, s->d_kept.get(), s->frame_bytes };
        largest = std::max(largest, s->frame_bytes);
    }
    const uint32_t chunks = std::min((largest / 16u + 1023u) / 1024u, h264k::KEEP_MAX_CHUNKS);     /* about four 16-byte moves per lane */
    if (pull_wait_pictures(e, n, pics, st)) return -1;
    hipLaunchKernelGGL(h264k::k_keep, dim3(std::max(chunks, 1u), n), dim3(256), 0, st, e->titems.dev<h264k::KeepItem>());
    HIP_TRY(hipGetLastError());
    if (pull_end_locked(e, n, pics, st, fence_ev)) return -1;
    for (uint32_t i = 0; i < n; i++) {                                  /* a copy: the fraction is 0x80, the spread reads as `lowest` */
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        s->kept_lo_valid = false; s->spread_valid = false;
    }
    return kept_order_end(e, st);
}

/* h264bsdmiBlendCurrentPictures: keep_out_locked's pictures, checks, ordering and fence, with ONE k_blend launch that blends every
 * frame buffer into its instance's kept picture (d_kept: the high bytes, d_kept_lo: the low bytes, allocated here at the first blend).
 * An instance that holds no kept picture, or of which api.c knows none (fresh), starts with a copy.  sp.moving: n_moving words,
 * zeroed on st ahead of the launch; picture i counts into word pics[i].index. */
static int blend_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, const uint32_t *fresh, const h264bsdmi_blend_spec &sp,
                            uint32_t n_moving, hipStream_t st, hipEvent_t *fence_ev)
{
    if (n > 65535u) return -1;                                          /* grid.y */
    if (sp.shift > 7u || sp.hold > 255u || (sp.moving_shift > 7u && sp.moving_shift != H264BSDMI_BLEND_FROZEN)) return -1;
    if (!pull_pictures_ok(n, pics, true, false)) return -1;
    for (uint32_t i = 0; i < n; i++) {
        if (sp.moving && pics[i].index >= n_moving) return -1;
        for (uint32_t k = 0; k < i; k++)
            if (pics[k].sink == pics[i].sink) return -1;                /* one kept picture per instance */
    }
    if (pull_begin_locked(e, n, pics, n)) return -1;
    if (kept_order_begin(e, st)) return -1;
    h264k::BlendItem *items = e->titems.host<h264k::BlendItem>();
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        uint32_t flags = fresh[i] ? (uint32_t)h264k::BLEND_FRESH : 0u;
        if (!s->d_kept) {
            HIP_TRY(s->d_kept.alloc(s->frame_bytes));
            s->kept_wmb = s->wmb; s->kept_hmb = s->hmb;
            flags |= h264k::BLEND_FRESH;
        }
        if (!s->d_kept_lo) {
            s->kept_lo_valid = false;
            HIP_TRY(s->d_kept_lo.alloc(s->frame_bytes));
        }
        if (!s->kept_lo_valid) flags |= h264k::BLEND_LO_UNSET;
        items[i] = h264k::BlendItem{ s->d_frames + (size_t)pics[i].slot * s->frame_bytes, s->d_kept.get(), s->d_kept_lo.get(), s->frame_bytes,
                                     flags, pics[i].index };
        largest = std::max(largest, s->frame_bytes);
    }
    /* 16 tiles per workgroup and step, about four steps per workgroup */
    const uint32_t chunks = std::min((largest / 384u + 63u) / 64u, h264k::BLEND_MAX_CHUNKS);
    if (sp.moving) HIP_TRY(hipMemsetAsync(sp.moving, 0, (size_t)n_moving * sizeof(uint32_t), st));
    if (pull_wait_pictures(e, n, pics, st)) return -1;
    const h264k::BlendArgs bargs{ e->titems.dev<h264k::BlendItem>(), static_cast<uint32_t *>(sp.moving), sp.shift, sp.hold,
                                  sp.moving_shift == H264BSDMI_BLEND_FROZEN ? h264k::BLEND_FROZEN : sp.moving_shift };
    hipLaunchKernelGGL(h264k::k_blend, dim3(std::max(chunks, 1u), n), dim3(256), 0, st, bargs);
    HIP_TRY(hipGetLastError());
    if (pull_end_locked(e, n, pics, st, fence_ev)) return -1;
    for (uint32_t i = 0; i < n; i++) static_cast<SinkUser *>(pics[i].sink->user)->s->kept_lo_valid = true;
    return kept_order_end(e, st);
}

/* h264bsdmiBlendCurrentPicturesSpread: blend_out_locked with ONE k_blend_spread launch, which beside d_kept and d_kept_lo reads and
 * writes the instance's spread (d_spread, allocated here at the first spread blend).  flags[i]: ENG_SPREAD_* (engine.h) — what api.c
 * knows of the instance's kept picture and of its spread; the engine adds what it knows itself (no buffer yet, a plain keep came
 * last).  Behind the launch the spread of every instance of the call is valid. */
static int blend_spread_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, const uint32_t *flags, const h264bsdmi_blend_spec &sp,
                                   const h264bsdmi_spread_spec &vs, uint32_t n_moving, hipStream_t st, hipEvent_t *fence_ev)
{
    if (n > 65535u) return -1;                                          /* grid.y */
    if (sp.shift > 7u || sp.hold > 255u || (sp.moving_shift > 7u && sp.moving_shift != H264BSDMI_BLEND_FROZEN)) return -1;
    if (vs.gain < 1u || vs.gain > 8u || vs.highest > 255u || vs.lowest > vs.highest || vs.update > H264BSDMI_SPREAD_STILL) return -1;
    if (!pull_pictures_ok(n, pics, true, false)) return -1;
    for (uint32_t i = 0; i < n; i++) {
        if (sp.moving && pics[i].index >= n_moving) return -1;
        for (uint32_t k = 0; k < i; k++)
            if (pics[k].sink == pics[i].sink) return -1;                /* one kept picture per instance */
    }
    if (pull_begin_locked(e, n, pics, n)) return -1;
    if (kept_order_begin(e, st)) return -1;
    h264k::SpreadItem *items = e->titems.host<h264k::SpreadItem>();
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        uint32_t f = flags[i] & ENG_SPREAD_FRESH ? (uint32_t)h264k::BLEND_FRESH : 0u;
        if (flags[i] & ENG_SPREAD_UNSET) f |= h264k::BLEND_V_UNSET;
        if (!s->d_kept) {
            HIP_TRY(s->d_kept.alloc(s->frame_bytes));
            s->kept_wmb = s->wmb; s->kept_hmb = s->hmb;
            f |= h264k::BLEND_FRESH;
        }
        if (!s->d_kept_lo) {
            s->kept_lo_valid = false;
            HIP_TRY(s->d_kept_lo.alloc(s->frame_bytes));
        }
        if (!s->d_spread) {
            s->spread_valid = false;
            HIP_TRY(s->d_spread.alloc(s->frame_bytes));
        }
        if (!s->kept_lo_valid) f |= h264k::BLEND_LO_UNSET;
        if (!s->spread_valid) f |= h264k::BLEND_V_UNSET;
        items[i] = h264k::SpreadItem{ s->d_frames + (size_t)pics[i].slot * s->frame_bytes, s->d_kept.get(), s->d_kept_lo.get(), s->d_spread.get(),
                                      s->frame_bytes, f, pics[i].index };
        largest = std::max(largest, s->frame_bytes);
    }
    /* 16 tiles per workgroup and step, about four steps per workgroup */
    const uint32_t chunks = std::min((largest / 384u + 63u) / 64u, h264k::BLEND_MAX_CHUNKS);
    if (sp.moving) HIP_TRY(hipMemsetAsync(sp.moving, 0, (size_t)n_moving * sizeof(uint32_t), st));
    if (pull_wait_pictures(e, n, pics, st)) return -1;
    const h264k::SpreadArgs sargs{ e->titems.dev<h264k::SpreadItem>(), static_cast<uint32_t *>(sp.moving), sp.shift, sp.hold,
                                   sp.moving_shift == H264BSDMI_BLEND_FROZEN ? h264k::BLEND_FROZEN : sp.moving_shift, vs.gain, vs.lowest, vs.highest, vs.update };
    hipLaunchKernelGGL(h264k::k_blend_spread, dim3(std::max(chunks, 1u), n), dim3(256), 0, st, sargs);
    HIP_TRY(hipGetLastError());
    if (pull_end_locked(e, n, pics, st, fence_ev)) return -1;
    for (uint32_t i = 0; i < n; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        s->kept_lo_valid = true; s->spread_valid = true;
    }
    return kept_order_end(e, st);
}

/* h264bsdmiWarpKeptPictures: the kept picture of every pics[i].sink (each holds one of its coded size, or the call is refused)
 * resampled through maps[i] inside the window of pics[i], with ONE k_warp_kept launch inside the kept pictures' ordering: from the live
 * buffers into the instance's spare ones (allocated here at the first warp; the lo spare only while lo is valid), every byte of which
 * the launch writes; then live and spare change places on the host.  The ordering makes that safe across streams: every launch that
 * reads or writes a kept buffer, this one included, is enqueued behind the previous one, so the next reader of d_kept runs behind this
 * launch and the next warp, which writes the buffers that are live now, behind every reader of them.  Under CURRENT the current
 * pictures are read: the checks, the flush, the wait and the fence of keep_out_locked; under REPLICATE no frame buffer is read, as in
 * kept_out_locked.  sp.count: n_count words, zeroed on st ahead of the launch; picture i counts into word pics[i].index. */
static int warp_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, const h264bsdmi_warp_map *maps, const h264bsdmi_warp_spec &sp,
                           uint32_t n_count, hipStream_t st, hipEvent_t *fence_ev)
{
    const bool current = sp.outside == H264BSDMI_WARP_CURRENT;
    if (n > 65535u || !maps || sp.outside > H264BSDMI_WARP_CURRENT) return -1;                 /* grid.y */
    if (current && !pull_pictures_ok(n, pics, true, false)) return -1;
    for (uint32_t i = 0; i < n; i++) {
        const SinkTensorPic &p = pics[i];
        const StreamCtx *s = pic_stream(p);
        if (!p.w || !p.h || p.x0 + p.w > s->wmb * 16 || p.y0 + p.h > s->hmb * 16 || ((p.x0 | p.y0 | p.w | p.h) & 1u)) return -1;
        if (sp.count && p.index >= n_count) return -1;
        const int32_t lin[4] = { maps[i].a, maps[i].b, maps[i].d, maps[i].e };
        for (int32_t v : lin)
            if (v > H264BSDMI_WARP_MAX_COEFFICIENT || v < -H264BSDMI_WARP_MAX_COEFFICIENT) return -1;
        for (uint32_t k = 0; k < i; k++)
            if (pics[k].sink == p.sink) return -1;                      /* one kept picture per instance */
    }
    if (!kept_pictures_ok(n, pics)) return -1;
    if (current ? pull_begin_locked(e, n, pics, n) : (e->titems.reserve(n, 256) != hipSuccess)) return -1;
    if (kept_order_begin(e, st)) return -1;
    h264k::WarpItem *items = e->titems.host<h264k::WarpItem>();
    uint32_t most = 0;
    for (uint32_t i = 0; i < n; i++) {
        const SinkTensorPic &p = pics[i];
        StreamCtx *s = static_cast<SinkUser *>(p.sink->user)->s;
        const size_t bytes = (size_t)s->kept_wmb * s->kept_hmb * h264k::TILE;
        const bool lo = s->kept_lo_valid && s->d_kept_lo;
        if (!s->d_kept_spare) HIP_TRY(s->d_kept_spare.alloc(bytes));
        if (lo && !s->d_kept_lo_spare) HIP_TRY(s->d_kept_lo_spare.alloc(bytes));
        items[i] = h264k::WarpItem{ current ? s->d_frames + (size_t)p.slot * s->frame_bytes : nullptr, s->d_kept.get(), lo ? s->d_kept_lo.get() : nullptr,
                                    s->d_kept_spare.get(), lo ? s->d_kept_lo_spare.get() : nullptr, s->kept_wmb, s->kept_hmb, p.x0, p.y0, p.w, p.h,
                                    p.index, { maps[i].a, maps[i].b, maps[i].c, maps[i].d, maps[i].e, maps[i].f } };
        most = std::max(most, ((s->kept_wmb + 3u) / 4u) * s->kept_hmb);
    }
    if (sp.count) HIP_TRY(hipMemsetAsync(sp.count, 0, (size_t)n_count * sizeof(uint32_t), st));
    if (current && pull_wait_pictures(e, n, pics, st)) return -1;
    const h264k::WarpArgs wargs{ e->titems.dev<h264k::WarpItem>(), static_cast<uint32_t *>(sp.count), sp.outside };
    hipLaunchKernelGGL(h264k::k_warp_kept, dim3(std::min(std::max(most, 1u), h264k::WARP_MAX_BLOCKS), n), dim3(256), 0, st, wargs);
    HIP_TRY(hipGetLastError());
    if (pull_end_locked(e, n, pics, st, fence_ev)) return -1;
    for (uint32_t i = 0; i < n; i++) {
        StreamCtx *s = static_cast<SinkUser *>(pics[i].sink->user)->s;
        std::swap(s->d_kept, s->d_kept_spare);
        if (s->kept_lo_valid && s->d_kept_lo) std::swap(s->d_kept_lo, s->d_kept_lo_spare);
    }
    return kept_order_end(e, st);
}

/* h264bsdmiOutputKeptPictures: the kept pictures of the instances pics[i].sink (each holds one of its coded size, or the call is
 * refused) as planar I420 into the caller's buffers, ONE k_kept_out launch inside the kept pictures' ordering.  No frame buffer is
 * read: nothing is flushed and no picture is waited for; the fence only carries the wait of a call without a stream. */
static int kept_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, void *const *picture, void *const *fraction, hipStream_t st,
                           hipEvent_t *fence_ev)
{
    if (n > 65535u || !picture) return -1;                              /* grid.y */
    for (uint32_t i = 0; i < n; i++) {
        if (!picture[i] || (reinterpret_cast<uintptr_t>(picture[i]) & 15u) || (fraction && (reinterpret_cast<uintptr_t>(fraction[i]) & 15u))) return -1;
        for (uint32_t k = 0; k < i; k++)
            if (pics[k].sink == pics[i].sink) return -1;
    }
    if (!kept_pictures_ok(n, pics)) return -1;
    HIP_TRY(e->titems.reserve(n, 256));
    if (kept_order_begin(e, st)) return -1;
    h264k::KeptOutItem *items = e->titems.host<h264k::KeptOutItem>();
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; i++) {
        const StreamCtx *s = pic_stream(pics[i]);
        items[i] = h264k::KeptOutItem{ s->d_kept.get(), s->kept_lo_valid ? s->d_kept_lo.get() : nullptr, static_cast<uint8_t *>(picture[i]),
                                       fraction ? static_cast<uint8_t *>(fraction[i]) : nullptr, s->kept_wmb, s->kept_hmb };
        largest = std::max(largest, s->kept_wmb * s->kept_hmb * 24u);
    }
    const uint32_t chunks = std::min((largest + 1023u) / 1024u, h264k::BLEND_MAX_CHUNKS);          /* about four 16-byte pieces per lane */
    hipLaunchKernelGGL(h264k::k_kept_out, dim3(std::max(chunks, 1u), n), dim3(256), 0, st, e->titems.dev<h264k::KeptOutItem>());
    HIP_TRY(hipGetLastError());
    if (pull_end_locked(e, n, pics, st, fence_ev)) return -1;
    return kept_order_end(e, st);
}

/* every picture's instance has, beside the kept picture, a valid spread (api.c names only instances that have one) */
static bool spread_frames_ok(uint32_t n, const SinkTensorPic *pics)
{
    for (uint32_t i = 0; i < n; i++) {
        const StreamCtx *s = pic_stream(pics[i]);
        if (!s->d_spread || !s->spread_valid) return false;
    }
    return kept_pictures_ok(n, pics);
}

/* h264bsdmiOutputKeptSpread: kept_out_locked's launch with the spread in the place of hi and no fraction: k_kept_out as it stands */
static int kept_spread_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, void *const *spread, hipStream_t st, hipEvent_t *fence_ev)
{
    if (n > 65535u || !spread) return -1;                               /* grid.y */
    for (uint32_t i = 0; i < n; i++) {
        if (!spread[i] || (reinterpret_cast<uintptr_t>(spread[i]) & 15u)) return -1;
        for (uint32_t k = 0; k < i; k++)
            if (pics[k].sink == pics[i].sink) return -1;
    }
    if (!spread_frames_ok(n, pics)) return -1;
    HIP_TRY(e->titems.reserve(n, 256));
    if (kept_order_begin(e, st)) return -1;
    h264k::KeptOutItem *items = e->titems.host<h264k::KeptOutItem>();
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; i++) {
        const StreamCtx *s = pic_stream(pics[i]);
        items[i] = h264k::KeptOutItem{ s->d_spread.get(), nullptr, static_cast<uint8_t *>(spread[i]), nullptr, s->kept_wmb, s->kept_hmb };
        largest = std::max(largest, s->kept_wmb * s->kept_hmb * 24u);
    }
    const uint32_t chunks = std::min((largest + 1023u) / 1024u, h264k::BLEND_MAX_CHUNKS);          /* about four 16-byte pieces per lane */
    hipLaunchKernelGGL(h264k::k_kept_out, dim3(std::max(chunks, 1u), n), dim3(256), 0, st, e->titems.dev<h264k::KeptOutItem>());
    HIP_TRY(hipGetLastError());
    if (pull_end_locked(e, n, pics, st, fence_ev)) return -1;
    return kept_order_end(e, st);
}

/* h264bsdmiOutputRegionChange: one ChangeItem per region, the current picture and the kept picture of its instance at box ∩ window,
 * ONE banded k_region_change launch.  A picture whose instance has no kept picture of its coded size is refused. */
static int change_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                             const h264bsdmi_change_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    uint32_t shift;
    if (!sp.data || (reinterpret_cast<uintptr_t>(sp.data) & 7u) || sp.crop > 1u || sp.keep_after > 1u ||
        !source_bins_ok(sp.source, sp.bins, &shift)) return -1;
    if (sp.threshold[0] > 255u || sp.threshold[1] > 255u || sp.threshold[2] > 255u) return -1;
    if (!analysis_regions_ok(n, pics, n_regs, regs, true)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::ChangeItem *items = e->titems.host<h264k::ChangeItem>();
    const uint32_t stride = h264k::change_record_bytes(sp.source == H264BSDMI_STATS_Y ? 1u : 3u, sp.bins);
    uint32_t tallest = 0u;
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r], &tallest);
        items[r] = h264k::ChangeItem{ s.frame, s.kept, static_cast<uint8_t *>(sp.data) + (size_t)regs[r].index * stride, s.wmb, s.c.x0, s.c.y0, s.c.x1, s.c.y1 };
    }
    h264k::ChangeArgs cargs{ e->titems.dev<h264k::ChangeItem>(), nullptr, nullptr, sp.bins, shift, { sp.threshold[0], sp.threshold[1], sp.threshold[2] } };
    return banded_launch_locked(e, n, pics, st, banded_kernel(true, sp.source, sp.bins != 0u), n_regs, tallest, &cargs, true, fence_ev);
}

/* h264bsdmiOutputRegionShift: one ShiftItem per region — the current picture and the kept picture of its instance, the record, box ∩
 * window and the window itself (the search clamps there), in luma samples of the coded frame — and ONE banded k_region_shift launch,
 * the bands' partial SAD surfaces in the scratch.  The kept pictures as in change_out_locked; the sink does not look at keep_after. */
static int shift_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                            const h264bsdmi_shift_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    if (!sp.data || (reinterpret_cast<uintptr_t>(sp.data) & 7u) || sp.radius > H264BSDMI_SHIFT_MAX_RADIUS || sp.surface > 1u || sp.crop > 1u ||
        sp.keep_after > 1u) return -1;
    for (uint32_t r = 0; r < n_regs; r++)
        if (regs[r].w > H264BSDMI_SHIFT_MAX_SIDE || regs[r].h > H264BSDMI_SHIFT_MAX_SIDE) return -1;        /* the 32-bit sums */
    if (!analysis_regions_ok(n, pics, n_regs, regs, true)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::ShiftItem *items = e->titems.host<h264k::ShiftItem>();
    const uint32_t stride = h264k::shift_record_bytes(sp.radius, sp.surface);
    uint32_t tallest = 0u;
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r], &tallest);
        items[r] = h264k::ShiftItem{ s.frame, s.kept, static_cast<uint8_t *>(sp.data) + (size_t)regs[r].index * stride, s.wmb, s.c.x0, s.c.y0, s.c.x1, s.c.y1,
                                     s.wx0, s.wy0, s.wx1, s.wy1 };
    }
    const void *fn = shift_kernel_of(sp.radius, &h264k::k_region_shift<h264k::SHIFT_QUADS>, &h264k::k_region_shift<1u>);
    h264k::ShiftArgs sargs{ e->titems.dev<h264k::ShiftItem>(), nullptr, nullptr, sp.radius, sp.surface };
    return banded_launch_locked(e, n, pics, st, fn, n_regs, tallest, &sargs, true, fence_ev);
}

/* h264bsdmiOutputCornerPoints: one CornerItem per region — the current picture, the record, box ∩ window and the window itself (the
 * luma is replicated there) in luma samples of the coded frame — and ONE banded k_corner_points launch of the score's kernel, the
 * bands' best points in the scratch.  No kept picture is read. */
static int corners_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                              const h264bsdmi_corners_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    if (!sp.data || (reinterpret_cast<uintptr_t>(sp.data) & 7u) || sp.score > H264BSDMI_CORNERS_HARRIS || (sp.block != 3u && sp.block != 5u) ||
        sp.nms < 1u || sp.nms > H264BSDMI_CORNERS_MAX_NMS || sp.max_points < 1u || sp.max_points > H264BSDMI_CORNERS_MAX_POINTS ||
        sp.crop > 1u || sp.zero || (sp.score == H264BSDMI_CORNERS_HARRIS && sp.min_score >> 63)) return -1;
    if (!analysis_regions_ok(n, pics, n_regs, regs, false)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::CornerItem *items = e->titems.host<h264k::CornerItem>();
    const uint32_t stride = h264k::corner_record_bytes(sp.max_points);
    uint32_t tallest = 0u;
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r], &tallest);
        items[r] = h264k::CornerItem{ s.frame, static_cast<uint8_t *>(sp.data) + (size_t)regs[r].index * stride, s.wmb, s.c.x0, s.c.y0, s.c.x1, s.c.y1,
                                      s.wx0, s.wy0, s.wx1, s.wy1 };
    }
    const void *const fns[2][2] = {
        { reinterpret_cast<const void *>(&h264k::k_corner_points<h264k::CORNER_MIN_EIGEN, 3>), reinterpret_cast<const void *>(&h264k::k_corner_points<h264k::CORNER_MIN_EIGEN, 5>) },
        { reinterpret_cast<const void *>(&h264k::k_corner_points<h264k::CORNER_HARRIS, 3>), reinterpret_cast<const void *>(&h264k::k_corner_points<h264k::CORNER_HARRIS, 5>) } };
    const void *fn = fns[sp.score][sp.block == 5u];
    h264k::CornerArgs cargs{ e->titems.dev<h264k::CornerItem>(), nullptr, nullptr, sp.nms, sp.max_points, sp.min_score };
    return banded_launch_locked(e, n, pics, st, fn, n_regs, tallest, &cargs, false, fence_ev);
}

/* h264bsdmiOutputCellMaps: one CellItem per region — the frame, in CHANGE mode the kept frame, the slice, the box's origin (signed) and
 * box ∩ window in luma samples of the coded frame — and ONE k_cell_maps launch of (rectangles of the grid, regions) workgroups.  Every
 * cell is owned by one workgroup: no scratch.  CHANGE: the kept pictures' ordering, and a picture whose instance has no kept picture
 * of its coded size is refused (api.c names only instances that have one). */
template <int MODE, int SRC> static const void *cells_kernel(bool quad)
{
    return quad ? reinterpret_cast<const void *>(&h264k::k_cell_maps<MODE, SRC, true>) : reinterpret_cast<const void *>(&h264k::k_cell_maps<MODE, SRC, false>);
}
/* What cells_out_locked and cell_boxes_out_locked share: the refusals, pull_begin_locked with room for `extra` more item slots behind
 * the CellItems, the CellItems, and the k_cell_maps launch as CellsLaunch describes it (not made yet) */
struct CellsLaunch { const void *fn; dim3 grid; h264k::CellArgs args; bool change; uint32_t shift, channels; };
static int cells_prepare_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                                const h264bsdmi_cells_spec &sp, uint32_t extra, CellsLaunch *L)
{
    const bool spread = sp.mode == H264BSDMI_CELLS_SPREAD, change = sp.mode == H264BSDMI_CELLS_CHANGE || spread;   /* change: kept pictures are read */
    if (!sp.data || (reinterpret_cast<uintptr_t>(sp.data) & 3u)) return -1;
    if (sp.source > H264BSDMI_STATS_RGB || sp.crop > 1u || sp.mode > H264BSDMI_CELLS_SPREAD || sp.keep_after > 1u) return -1;
    if (!sp.planes || (sp.planes & ~(spread ? 15u : change ? 63u : 31u))) return -1;
    if (spread && (sp.source == H264BSDMI_STATS_RGB || sp.keep_after)) return -1;
    if (sp.threshold[0] > 255u || sp.threshold[1] > 255u || sp.threshold[2] > 255u) return -1;
    if (!change && (sp.threshold[0] || sp.threshold[1] || sp.threshold[2] || sp.keep_after)) return -1;
    if (!analysis_regions_ok(n, pics, n_regs, regs, change) || (spread && !spread_frames_ok(n, pics))) return -1;
    CellGrid G;
    if (!cell_grid(sp.cell, sp.cols, sp.rows, n_regs, CELLS_LIMITS, &G)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs + extra)) return -1;
    h264k::CellItem *items = e->titems.host<h264k::CellItem>();
    const uint32_t channels = sp.source == H264BSDMI_STATS_Y ? 1u : 3u;
    const size_t slice = ((sp.planes & 1u) + channels * (size_t)__builtin_popcount(sp.planes >> 1)) * sp.rows * sp.cols;      /* words */
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r]);
        items[r] = h264k::CellItem{ s.frame, change ? s.kept : nullptr, static_cast<uint32_t *>(sp.data) + (size_t)regs[r].index * slice, s.wmb, s.ox, s.oy,
                                    s.c.x0, s.c.y0, s.c.x1, s.c.y1, spread ? s.spread : nullptr };
    }
    const bool quad = sp.cell >= 16u;
    const void *const fns[3][3] = {
        { cells_kernel<0, h264k::ST_Y>(quad), cells_kernel<0, h264k::ST_YCBCR>(quad), cells_kernel<0, h264k::ST_RGB>(quad) },
        { cells_kernel<1, h264k::ST_Y>(quad), cells_kernel<1, h264k::ST_YCBCR>(quad), cells_kernel<1, h264k::ST_RGB>(quad) },
        { cells_kernel<2, h264k::ST_Y>(quad), cells_kernel<2, h264k::ST_YCBCR>(quad), nullptr } };                       /* SPREAD has no RGB */
    *L = CellsLaunch{ fns[sp.mode][sp.source], dim3(G.rects, n_regs),
                      { e->titems.dev<h264k::CellItem>(), sp.cols, sp.rows, G.shift, G.rects_x, sp.planes, { sp.threshold[0], sp.threshold[1], sp.threshold[2] } },
                      change, G.shift, channels };
    return 0;
}
static int cells_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                            const h264bsdmi_cells_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    CellsLaunch L;
    if (cells_prepare_locked(e, n, pics, n_regs, regs, sp, 0u, &L)) return -1;
    if (L.change && kept_order_begin(e, st)) return -1;
    if (pull_launch_locked(e, n, pics, st, { { L.fn, L.grid, &L.args } }, fence_ev)) return -1;
    return L.change ? kept_order_end(e, st) : 0;
}

/* h264bsdmiOutputCellBoxes: what cells_out_locked enqueues, and between its k_cell_maps launch and the fence ONE k_cell_boxes launch
 * of one workgroup per region, which labels the chosen map of the slice the launch before it wrote: the fence and the error words
 * stand behind both, and in CHANGE mode the kept pictures' ordering encloses both.  One BoxItem per region in the staging slots behind
 * the CellItems: the boxes slice and the origin of the source window, which the CellItem does not carry. */
static int cell_boxes_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                                 const h264bsdmi_cells_spec &sp, const h264bsdmi_boxes_spec &bs, hipStream_t st, hipEvent_t *fence_ev)
{
    const uint32_t channels = sp.source == H264BSDMI_STATS_Y ? 1u : 3u;
    if (!bs.data || (reinterpret_cast<uintptr_t>(bs.data) & 3u) || !bs.max_boxes || bs.max_boxes > h264k::BOXES_MAX_BOXES) return -1;
    if (!bs.plane || (bs.plane & (bs.plane - 1u)) || !(bs.plane & sp.planes)) return -1;
    if (sp.mode == H264BSDMI_CELLS_CHANGE && bs.plane == H264BSDMI_CELL_DSUM) return -1;
    if (bs.channel >= (bs.plane == H264BSDMI_CELL_COUNT ? 1u : channels)) return -1;
    if (bs.sense > H264BSDMI_BOXES_BELOW || (bs.connectivity != 4u && bs.connectivity != 8u) || !bs.min_cells) return -1;
    if (!sp.cols || !sp.rows || (uint64_t)sp.cols * sp.rows > h264k::BOXES_MAX_CELLS) return -1;       /* what one workgroup's LDS holds */
    CellsLaunch L;
    if (cells_prepare_locked(e, n, pics, n_regs, regs, sp, n_regs, &L)) return -1;
    h264k::BoxItem *items = reinterpret_cast<h264k::BoxItem *>(e->titems.host<TItemSlot>() + n_regs);
    const size_t words = (size_t)(1u + bs.max_boxes) * 8u;
    for (uint32_t r = 0; r < n_regs; r++) {
        const SinkTensorPic &p = pics[regs[r].pic];
        items[r] = h264k::BoxItem{ static_cast<uint32_t *>(bs.data) + (size_t)regs[r].index * words, (int32_t)p.x0, (int32_t)p.y0 };
    }
    /* COUNT, then per set bit of planes in ascending order `channels` maps */
    const uint32_t before = bs.plane == H264BSDMI_CELL_COUNT ? 0u
        : (sp.planes & 1u) + L.channels * (uint32_t)__builtin_popcount(sp.planes & (bs.plane - 1u) & ~1u) + bs.channel;
    h264k::BoxArgs bargs{ L.args.items, reinterpret_cast<const h264k::BoxItem *>(e->titems.dev<TItemSlot>() + n_regs), sp.cols, sp.rows, L.shift,
                          before * sp.rows * sp.cols, bs.max_boxes, bs.sense, bs.level, bs.connectivity, bs.min_cells };
    if (L.change && kept_order_begin(e, st)) return -1;
    if (pull_launch_locked(e, n, pics, st, { { L.fn, L.grid, &L.args }, { reinterpret_cast<const void *>(&h264k::k_cell_boxes), dim3(n_regs), &bargs } },
                           fence_ev)) return -1;
    return L.change ? kept_order_end(e, st) : 0;
}

/* h264bsdmiOutputCellShift: one FlowItem per region — the current picture and the kept picture of its instance, the slice, the box's
 * origin (signed), box ∩ window and the window itself (the search clamps there) in luma samples of the coded frame — and ONE k_cell_shift
 * launch of (rectangles of the grid, regions) workgroups inside the kept pictures' ordering.  Every cell is owned by one workgroup: no
 * scratch.  The kept pictures as in shift_out_locked; keep_after is not looked at. */
static int flow_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                           const h264bsdmi_cell_shift_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    const uint32_t all = H264BSDMI_FLOW_COUNT | H264BSDMI_FLOW_DX | H264BSDMI_FLOW_DY | H264BSDMI_FLOW_BEST | H264BSDMI_FLOW_STILL | H264BSDMI_FLOW_TIES;
    if (!sp.data || (reinterpret_cast<uintptr_t>(sp.data) & 3u)) return -1;
    if (sp.radius > H264BSDMI_SHIFT_MAX_RADIUS || !sp.planes || (sp.planes & ~all) || sp.crop > 1u || sp.keep_after > 1u) return -1;
    if (!analysis_regions_ok(n, pics, n_regs, regs, true)) return -1;
    CellGrid G;
    if (!cell_grid(sp.cell, sp.cols, sp.rows, n_regs, FLOW_LIMITS, &G)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::FlowItem *items = e->titems.host<h264k::FlowItem>();
    const size_t slice = (size_t)__builtin_popcount(sp.planes) * sp.rows * sp.cols;                   /* words */
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r]);
        items[r] = h264k::FlowItem{ s.frame, s.kept, static_cast<uint32_t *>(sp.data) + (size_t)regs[r].index * slice, s.wmb, s.ox, s.oy,
                                    s.c.x0, s.c.y0, s.c.x1, s.c.y1, s.wx0, s.wy0, s.wx1, s.wy1 };
    }
    const void *fn = shift_kernel_of(sp.radius, &h264k::k_cell_shift<h264k::SHIFT_QUADS>, &h264k::k_cell_shift<1u>);
    h264k::FlowArgs fargs{ e->titems.dev<h264k::FlowItem>(), sp.cols, sp.rows, G.shift, G.rects_x, sp.planes, sp.radius };
    if (kept_order_begin(e, st)) return -1;
    if (pull_launch_locked(e, n, pics, st, { { fn, dim3(G.rects, n_regs), &fargs } }, fence_ev)) return -1;
    return kept_order_end(e, st);
}

/* h264bsdmiOutputPointMatches: one MatchItem per region — the current picture and the kept picture of its instance, the record, the two
 * point records (the caller's, read on st), box ∩ window and the window itself (the luma is replicated there) in luma samples of the coded
 * frame — and TWO launches inside the kept pictures' ordering, the fence and the error words behind both: k_point_describe of (groups of
 * slots, regions) workgroups writes the descriptors into the record, k_point_match of one workgroup per region reads them there and
 * writes the rest.  No scratch of the engine.  The kept pictures as in shift_out_locked; keep_after is not looked at. */
static int matches_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_regs, const SinkRegion *regs,
                              const h264bsdmi_matches_spec &sp, hipStream_t st, hipEvent_t *fence_ev)
{
    const auto misaligned = [](const void *p) { return !p || (reinterpret_cast<uintptr_t>(p) & 7u); };
    if (misaligned(sp.data) || misaligned(sp.kept_points) || misaligned(sp.current_points)) return -1;
    if (sp.max_points < 1u || sp.max_points > h264k::MATCH_MAX_K || sp.max_distance > 256u || sp.ratio < 1u || sp.ratio > 256u ||
        sp.max_move > 65535u || sp.mutual_only > 1u || sp.crop > 1u || sp.keep_after > 1u || sp.zero) return -1;
    if (!analysis_regions_ok(n, pics, n_regs, regs, true)) return -1;
    if (pull_begin_locked(e, n, pics, n_regs)) return -1;
    h264k::MatchItem *items = e->titems.host<h264k::MatchItem>();
    const size_t stride = h264k::matches_record_bytes(sp.max_points), pstride = h264k::corner_record_bytes(sp.max_points);
    for (uint32_t r = 0; r < n_regs; r++) {
        const RegionSource s = region_source(pics, regs[r]);
        const size_t index = regs[r].index;
        items[r] = h264k::MatchItem{ s.frame, s.kept, static_cast<uint8_t *>(sp.data) + index * stride,
                                     static_cast<const uint8_t *>(sp.kept_points) + index * pstride, static_cast<const uint8_t *>(sp.current_points) + index * pstride,
                                     s.wmb, s.c.x0, s.c.y0, s.c.x1, s.c.y1, s.wx0, s.wy0, s.wx1, s.wy1 };
    }
    h264k::MatchArgs margs{ e->titems.dev<h264k::MatchItem>(), sp.max_points, sp.max_distance, sp.ratio, sp.max_move, sp.mutual_only };
    if (kept_order_begin(e, st)) return -1;
    const uint32_t groups = (2u * sp.max_points + h264k::MATCH_GROUP - 1u) / h264k::MATCH_GROUP;
    if (pull_launch_locked(e, n, pics, st, { { reinterpret_cast<const void *>(&h264k::k_point_describe), dim3(groups, n_regs), &margs },
                                             { reinterpret_cast<const void *>(&h264k::k_point_match), dim3(n_regs), &margs } }, fence_ev)) return -1;
    return kept_order_end(e, st);
}

/* h264bsdmiOutputTensorRemap: the current pictures of the n instances sampled through n_maps coordinate maps by one k_tensor_remap
 * launch, map r into slice maps[r].index.  The fence goes to each distinct instance, so that the next picture decoded into one of
 * these slots waits for this launch.  The maps are the caller's: read on st. */
static int remap_out_locked(Engine *e, uint32_t n, const SinkTensorPic *pics, uint32_t n_maps, const SinkRemap *maps,
                            const h264bsdmi_tensor_spec &t, uint32_t chroma, const h264bsdmi_remap_spec &rm, hipStream_t st,
                            hipEvent_t *fence_ev)
{
    const bool ref = pics[0].matrix == H264BSDMI_MATRIX_REFERENCE;
    if (!t.resize || rm.filter > H264BSDMI_REMAP_BILINEAR || rm.border > H264BSDMI_BORDER_REPLICATE) return -1;
    const void *fn = tensor_kernel(TK_REMAP, t, ref);
    if (!fn || n_maps > 65535u) return -1;                              /* grid.y */
    if (!pull_pictures_ok(n, pics, ref, false)) return -1;
    for (uint32_t r = 0; r < n_maps; r++)
        if (maps[r].pic >= n || !maps[r].map || (reinterpret_cast<uintptr_t>(maps[r].map) & 7u)) return -1;
    if (pull_begin_locked(e, n, pics, n_maps)) return -1;
    h264k::RemapItem *items = e->titems.host<h264k::RemapItem>();
    std::vector<h264k::TensorItem> of_pic(n);                           /* the colour map once per picture */
    for (uint32_t i = 0; i < n; i++) of_pic[i] = picture_item(pics[i], t, 0);
    for (uint32_t r = 0; r < n_maps; r++) {
        items[r] = h264k::RemapItem{ of_pic[maps[r].pic], static_cast<const float *>(maps[r].map) };
        items[r].t.dst += maps[r].index * spec_slice_bytes(t);
    }
    /* pad: a non-finite coordinate; spad: outside the window */
    h264k::RemapArgs rargs{ e->titems.dev<h264k::RemapItem>(), t.width, t.height, chroma, rm.filter, rm.border, {}, {}, {}, {} };
    const PullPad pp = fold_pad(rm.pad, t.dtype, t.mean, t.std, ref);
    copy3(rargs.mean, t.mean); copy3(rargs.std, t.std); copy3(rargs.pad, pp.pad); copy3(rargs.spad, pp.spad);
    return pull_launch_locked(e, n, pics, st, { { fn, pull_grid(t.width, t.height, h264k::TRM_COLS, h264k::TRM_ROWS, n_maps), &rargs } }, fence_ev);
}

/* What every entry that enqueues on a caller's stream or the engine's own shares: the engine's mutex, its device, the refusal of a
 * capturing stream, and, when the caller gave no stream, the wait for the event the body names and the device's error words.
 * body(st, &done): enqueues on st under the mutex; *done: the event behind everything it enqueued, which is looked at only without a
 * caller's stream (a body may leave it unset on one). */
template <typename Body> static int engine_call(Engine *e, void *stream, Body body)
{
    hipEvent_t done = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        HIP_TRY(hipSetDevice(e->device));
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : e->stream;
        if (stream) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            HIP_TRY(hipStreamIsCapturing(st, &cs));
            if (cs != hipStreamCaptureStatusNone) return -1;                      /* graph capture of this call is not supported */
        }
        if (body(st, &done)) return -1;
    }
    if (stream) return 0;
    if (hipEventSynchronize(done) != hipSuccess) return -1;            /* (a later call may have recorded it again: that only waits longer) */
    std::lock_guard<std::mutex> lk(e->mu);
    fold_errors(e);
    return 0;
}
/* What JobSink.tensor_out, tensor_regions, motion_regions, tensor_remap, region_stats, keep_pictures, blend_pictures, kept_pictures_out, region_change, region_shift, corner_points, cell_maps and cell_boxes, and EngSinkEntries.cell_shift and point_matches, share: one engine (one device) per call, and engine_call
 * around the call's own *_out_locked, body(e, st, &fence_ev), with the fence as the event to wait for. */
template <typename Body> static int sink_tensor_call(uint32_t n, const SinkTensorPic *pics, void *stream, Body body)
{
    if (!n) return 0;
    if (!pics) return -1;
    Engine *e = static_cast<SinkUser *>(pics[0].sink->user)->e;
    for (uint32_t i = 1; i < n; i++)
        if (static_cast<SinkUser *>(pics[i].sink->user)->e != e) return -1;        /* one device per call */
    return engine_call(e, stream, [&](hipStream_t st, hipEvent_t *fence_ev) { return body(e, st, fence_ev); });
}
int sink_tensor_out(uint32_t n, const SinkTensorPic *pics, const h264bsdmi_tensor_spec *spec, uint32_t chroma,
                    const h264bsdmi_resize_spec *resize, void *stream)
{
    if (n && !spec) return -1;
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return tensor_out_locked(e, n, pics, *spec, chroma, resize, st, fence_ev);
    });
}
/* the calls that take a list (regions, maps): nothing to do without items, a refusal without one of the pointers */
template <typename Body> static int sink_list_call(uint32_t n, const SinkTensorPic *pics, uint32_t n_items, bool pointers, void *stream, Body body)
{
    if (!n_items) return 0;
    if (!pointers) return -1;
    return sink_tensor_call(n, pics, stream, body);
}
int sink_tensor_regions(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                        const h264bsdmi_tensor_spec *spec, uint32_t chroma, const h264bsdmi_resize_spec *resize, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && resize && (!n || spec), stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return regions_out_locked(e, n, pics, n_regions, regions, *spec, chroma, *resize, st, fence_ev);
    });
}
int sink_motion_regions(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                        const h264bsdmi_motion_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return motion_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_tensor_remap(uint32_t n, const SinkTensorPic *pics, uint32_t n_maps, const SinkRemap *maps,
                      const h264bsdmi_tensor_spec *spec, uint32_t chroma, const h264bsdmi_remap_spec *remap, void *stream)
{
    return sink_list_call(n, pics, n_maps, maps && spec && remap, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return remap_out_locked(e, n, pics, n_maps, maps, *spec, chroma, *remap, st, fence_ev);
    });
}
int sink_region_stats(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                      const h264bsdmi_stats_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return stats_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_keep_pictures(uint32_t n, const SinkTensorPic *pics, void *stream)
{
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return keep_out_locked(e, n, pics, st, fence_ev);
    });
}
int sink_blend_pictures(uint32_t n, const SinkTensorPic *pics, const uint32_t *fresh, const h264bsdmi_blend_spec *spec, uint32_t n_moving,
                        void *stream)
{
    if (n && (!spec || !fresh)) return -1;
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return blend_out_locked(e, n, pics, fresh, *spec, n_moving, st, fence_ev);
    });
}
int sink_kept_pictures_out(uint32_t n, const SinkTensorPic *pics, void *const *picture, void *const *fraction, void *stream)
{
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return kept_out_locked(e, n, pics, picture, fraction, st, fence_ev);
    });
}
int sink_region_change(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                       const h264bsdmi_change_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return change_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_region_shift(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                      const h264bsdmi_shift_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return shift_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_corner_points(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                       const h264bsdmi_corners_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return corners_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_cell_maps(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                   const h264bsdmi_cells_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return cells_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_cell_boxes(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                    const h264bsdmi_cells_spec *cells, const h264bsdmi_boxes_spec *boxes, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && cells && boxes, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return cell_boxes_out_locked(e, n, pics, n_regions, regions, *cells, *boxes, st, fence_ev);
    });
}
int sink_cell_shift(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                    const h264bsdmi_cell_shift_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return flow_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
int sink_point_matches(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                       const h264bsdmi_matches_spec *spec, void *stream)
{
    return sink_list_call(n, pics, n_regions, regions && spec, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return matches_out_locked(e, n, pics, n_regions, regions, *spec, st, fence_ev);
    });
}
/* EngSinkEntries.warp_kept (h264bsdmiWarpKeptPictures) */
int sink_warp_kept(uint32_t n, const SinkTensorPic *pics, const h264bsdmi_warp_map *maps, const h264bsdmi_warp_spec *spec, uint32_t n_count,
                   void *stream)
{
    if (n && (!spec || !maps)) return -1;
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return warp_out_locked(e, n, pics, maps, *spec, n_count, st, fence_ev);
    });
}
/* EngSinkEntries.blend_spread (h264bsdmiBlendCurrentPicturesSpread) and kept_spread_out (h264bsdmiOutputKeptSpread) */
int sink_blend_spread(uint32_t n, const SinkTensorPic *pics, const uint32_t *flags, const h264bsdmi_blend_spec *spec,
                      const h264bsdmi_spread_spec *spread, uint32_t n_moving, void *stream)
{
    if (n && (!spec || !spread || !flags)) return -1;
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return blend_spread_out_locked(e, n, pics, flags, *spec, *spread, n_moving, st, fence_ev);
    });
}
int sink_kept_spread_out(uint32_t n, const SinkTensorPic *pics, void *const *spread, void *stream)
{
    return sink_tensor_call(n, pics, stream, [&](Engine *e, hipStream_t st, hipEvent_t *fence_ev) {
        return kept_spread_out_locked(e, n, pics, spread, st, fence_ev);
    });
}
/* EngSinkEntries.point_model (h264bsdmiOutputPointModel): the first entry without pictures — the sink only names the engine, nothing is
 * staged (the kernel finds record r of the four arrays by its stride), no fence goes to an instance and no kept picture is touched, so
 * none of pull_begin_locked / pull_end_locked / the kept pictures' ordering applies.  One launch of a workgroup per record; without a
 * caller's stream the device's error words follow it and the call waits for an event of the engine's own. */
int sink_point_model(const JobSink *sink, uint32_t n_records, const h264bsdmi_model_spec *spec, void *stream)
{
    if (!n_records) return 0;
    if (!sink || sink->configure != sink_configure || !spec) return -1;
    const h264bsdmi_model_spec &sp = *spec;
    const auto misaligned = [](const void *p) { return !p || (reinterpret_cast<uintptr_t>(p) & 7u); };
    if (misaligned(sp.data) || misaligned(sp.matches) || misaligned(sp.kept_points) || misaligned(sp.current_points)) return -1;
    if (sp.max_points < 1u || sp.max_points > h264k::MODEL_MAX_K || sp.model > h264k::MODEL_SIMILARITY || sp.tolerance > 255u) return -1;
    if (sp.model == h264k::MODEL_SIMILARITY ? sp.max_scale && (sp.max_scale < 256u || sp.max_scale > 4096u) : sp.max_scale != 0u) return -1;
    if (sp.min_inliers < 1u + sp.model || sp.min_inliers > 256u || sp.zero[0] || sp.zero[1] || sp.zero[2]) return -1;
    if (n_records > 65535u) return -1;
    Engine *e = static_cast<SinkUser *>(sink->user)->e;
    return engine_call(e, stream, [&](hipStream_t st, hipEvent_t *done) {
        h264k::ModelArgs margs{ static_cast<uint8_t *>(sp.data), static_cast<const uint8_t *>(sp.matches), static_cast<const uint8_t *>(sp.kept_points),
                                static_cast<const uint8_t *>(sp.current_points), sp.max_points, sp.model, sp.tolerance, sp.max_scale, sp.min_inliers };
        void *args[] = { &margs };
        HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(&h264k::k_point_model), dim3(n_records), dim3(h264k::MODEL_THREADS), args, 0, st));
        if (stream) return 0;
        hipLaunchKernelGGL(k_err_words, dim3(1), dim3(64), 0, st, e->d_err, e->h_err.dev());
        HIP_TRY(hipGetLastError());
        if (!e->model_ev) HIP_TRY(e->model_ev.create(hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e->model_ev, st));
        *done = e->model_ev;
        return 0;
    });
}
/* JobSink.set_motion (h264bsdmiSetMotionExport): before the instance's first sequence is configured */
int sink_set_motion(void *user, int on)
{
    SinkUser *u = static_cast<SinkUser *>(user);
    std::lock_guard<std::mutex> lk(u->e->mu);
    if (u->s->n_slots) return -1;
    u->s->motion = on != 0;
    return 0;
}
} // namespace

/* ================================================================== C interface */
extern "C" {

int eng_attach(JobSink *sink)
{
    Engine *e = engine_get();
    if (!e) return -1;
    SinkUser *u = new SinkUser{ e, new StreamCtx() };
    {
        std::lock_guard<std::mutex> lk(e->mu);
        u->s->group = (int)e->group_rr++;             /* taken modulo the number of light lanes */
        e->streams.push_back(u->s);
    }
    sink->user = u;
    sink->configure = sink_configure;
    sink->acquire = sink_acquire;
    sink->submit = sink_submit;
    sink->fetch = sink_fetch;
    sink->fetch_begin = sink_fetch_begin;
    sink->fetch_end = sink_fetch_end;
    sink->fetch_converted = sink_fetch_converted;
    sink->fetch_device = sink_fetch_device;
    sink->close = sink_close;
    sink->errors = sink_errors;
    sink->tensor_out = sink_tensor_out;
    sink->tensor_regions = sink_tensor_regions;
    sink->motion_regions = sink_motion_regions;
    sink->tensor_remap = sink_tensor_remap;
    sink->region_stats = sink_region_stats;
    sink->set_motion = sink_set_motion;
    sink->keep_pictures = sink_keep_pictures;
    sink->region_change = sink_region_change;
    sink->region_shift = sink_region_shift;
    sink->cell_maps = sink_cell_maps;
    sink->cell_boxes = sink_cell_boxes;
    sink->blend_pictures = sink_blend_pictures;
    sink->kept_pictures_out = sink_kept_pictures_out;
    sink->corner_points = sink_corner_points;
    return 0;
}

/* engine.h: the entries behind the last member of JobSink, for a sink eng_attach has bound */
const EngSinkEntries *eng_sink_entries(const JobSink *sink)
{
    static const EngSinkEntries entries = { sink_cell_shift, sink_point_matches, sink_point_model, sink_warp_kept, sink_blend_spread, sink_kept_spread_out };
    return sink && sink->configure == sink_configure ? &entries : nullptr;
}

void eng_convert_host(int fmt, uint32_t width, uint32_t height, const uint8_t *data, uint32_t *out)
{
    Engine *e = engine_get();
    if (!e) {
        fprintf(stderr, "h264bsd-mi355x: h264bsdConvertTo*: no usable HIP device (this library has no CPU pixel path)\n");
        return;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t in_b = (size_t)width * height * 3 / 2, out_b = (size_t)width * height * 4;
    if (hipSetDevice(e->device) != hipSuccess) return;
    if (out_b > e->conv_cap) {
        e->conv_in.reset(); e->conv_out.reset(); e->conv_cap = 0;
        if (e->conv_in.alloc(in_b + 64) != hipSuccess || e->conv_out.alloc(out_b) != hipSuccess) return;
        e->conv_cap = out_b;
    }
    if (hipMemcpyAsync(e->conv_in, data, in_b, hipMemcpyHostToDevice, e->stream) != hipSuccess) return;
    hipLaunchKernelGGL(h264k::k_convert, dim3(1024, 1), dim3(256), 0, e->stream, e->conv_in, e->conv_out, width, height, fmt,
                       (size_t)0, (size_t)0, 0);
    if (hipMemcpyAsync(out, e->conv_out, out_b, hipMemcpyDeviceToHost, e->stream) != hipSuccess) return;
    hipStreamSynchronize(e->stream);
}

int h264bsdmiDeviceCount(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* Decoder instances and replay sets created by the calling thread from now on live on `device`; the first call also
 * sets the process default (threads that never call it).  Existing instances stay where they are. */
int h264bsdmiSetDevice(int device)
{
    int n = 0;
    if (device < 0 || device >= MAX_DEVICES || hipGetDeviceCount(&n) != hipSuccess || device >= n) return -1;
    tl_device = device;
    std::lock_guard<std::mutex> lk(g_engine_mu);
    if (g_default_device < 0) g_default_device = device;
    return 0;
}

/* the device (and with it the NUMA node: eng_device_cpus) a decoder instance lives on */
int eng_sink_device(const JobSink *sink)
{
    if (!sink || !sink->user || sink->submit != sink_submit) return -1;      /* capture-mode instances have another sink */
    return static_cast<const SinkUser *>(sink->user)->e->device;
}

/* CPUs close to a device: /sys/bus/pci/devices/<bus id>/local_cpulist ("0-63,128-191"), for pinning parser threads to
 * the NUMA node of the GPU their streams feed.  Returns the number of CPUs written to cpus[]. */
int eng_device_cpus(int device, int *cpus, int max)
{
    char bus[64], path[160], line[4096];
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return 0;
    for (char *c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bus);
    FILE *f = fopen(path, "r");
    if (!f) return 0;
    int n = 0;
    if (fgets(line, sizeof(line), f)) {
        for (char *p = line; *p && n < max;) {
            char *end;
            long a = strtol(p, &end, 10), b = a;
            if (end == p) break;
            if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); }
            for (long c = a; c <= b && n < max; c++) cpus[n++] = (int)c;
            p = *end == ',' ? end + 1 : end;
            if (*end != ',' ) break;
        }
    }
    fclose(f);
    return n;
}

/* after waiting for every device: their sticky error bits or-ed together, or (events) how often their tripwires fired; 0xFFFFFFFF = HIP error */
static unsigned poll_all_devices(bool events)
{
    unsigned all = 0;
    for (int d = 0; d < MAX_DEVICES; d++) {
        Engine *e;
        { std::lock_guard<std::mutex> lk(g_engine_mu); e = g_engines[d]; }
        if (!e) continue;
        std::lock_guard<std::mutex> lk(e->mu);
        if (hipSetDevice(e->device) != hipSuccess || poll_errors(e)) return 0xFFFFFFFFu;
        all = events ? all + e->error_events : all | e->errors;
    }
    return all;
}
unsigned h264bsdmiDeviceErrors(void) { return poll_all_devices(false); }

static int flush_all(bool wait)
{
    int rc = 0, any = 0;
    for (int d = 0; d < MAX_DEVICES; d++) {
        Engine *e;
        { std::lock_guard<std::mutex> lk(g_engine_mu); e = g_engines[d]; }
        if (!e) continue;
        any = 1;
        std::lock_guard<std::mutex> lk(e->mu);
        if (flush_locked(e, wait)) rc = -1;
    }
    if (!any && !engine_get()) return -1;
    return rc;
}

int h264bsdmiFlush(void) { return flush_all(true); }
int h264bsdmiFlushAsync(void) { return flush_all(false); }
} /* extern "C" */
#include "replay.hip.h"      /* the bench library's replay sets and debug hooks (include/h264bsd_mi355x_bench.h) */
