/* replay.hip.h — the measurement and test harness of include/h264bsd_mi355x_bench.h, exported by libh264bsd_mi355x_bench.so only: the
 * HBM-resident replay sets that bench.py and the kernel tests drive (h264bsdmiReplay*), their static launch schedules
 * (replay_schedule) and the debug hooks (h264bsdmiDebug*).  None of it is on the product's path.  Included by engine.hip at its end and
 * part of its translation unit on purpose: this code launches kernels directly (launch_tick, k_convert_tiles, k_checksum, ...), and a
 * translation unit of its own would need a second device code object or a layer of launch wrappers — more machinery than the split buys. */
extern "C" {
/* test harness (bench library): tripwire events of all devices so far, after waiting for the devices — monotonic, unlike the
 * sticky bits of h264bsdmiDeviceErrors(): a test asserts that its own pictures added none */
unsigned h264bsdmiDebugDeviceErrorEvents(void) { return poll_all_devices(true); }

/* ------------------------------------------------------------------ replay sets */
struct h264bsdmi_replay {
    Engine *e;
    uint32_t n_pics, n_streams, n_slots, wmb, hmb, frame_bytes;
    size_t blob_stride;               /* bytes of all blobs of one stream (256-aligned) */
    unsigned long long job_bytes;     /* sum of the blob sizes of one stream */
    DeviceMem<uint8_t> d_blobs;       /* n_streams * blob_stride */
    DeviceMem<uint8_t> d_frames;      /* n_streams * n_slots * frame_bytes */
    DeviceMem<uint8_t> d_dbk;         /* n_streams * n_mbs * 32 */
    DeviceMem<FrameDesc> d_desc;      /* n_pics * n_streams */
    DeviceMem<uint32_t> d_conv;       /* n_streams * w*h (lazy) */
    DeviceMem<uint8_t> d_planar;      /* one frame, planar (h264bsdmiReplayFetch) */
    DeviceMem<unsigned long long> d_sums;
    std::vector<TickShape> shapes;
    std::vector<uint8_t> cur_slot;
    std::vector<TickTimers> timers;
    uint32_t timed_first, timed_count;
    Event ev_begin, ev_end, gdone_any;
    uint32_t launches[5];
    unsigned stages;
    uint32_t n_groups;
    Stream gstream[8];
    Event gdone[8];
    bool overlap_dbk = true;
    unsigned timed_mask = 31u;
    /* desynchronised sets with heavy lanes (h264bsdmiReplayCreateDesync, lanes > 0): a static launch schedule */
    struct Launch { size_t first; TickShape shape; int lane; std::vector<int> waits; int record_ev; bool light; };
    std::vector<Launch> sched;
    std::vector<Event> sched_ev;
    static constexpr int MAX_LANES = 72;  /* lanes 0..n_light-1: one per stream group (light pictures), then the heavy lanes */
    Stream lanes[MAX_LANES];
    SideLane lane_side[MAX_LANES];        /* k_dbk next to the reconstruction kernels, per light lane */
    uint32_t n_lanes = 0, n_light = 0;
    /* HIP streams of earlier schedules of this set, reused by the next one (normal priority: light lanes and stream groups; highest: heavy
     * lanes; side-stream pairs).  A process that creates and destroys a dozen streams per schedule falls off the runtime's stream cliff after
     * a few of them (a 12-lane schedule then takes seconds per lap, the same schedule in a fresh process 0.13 s): nothing is destroyed before the set is. */
    std::vector<Stream> pool_normal, pool_high;
    std::vector<SideLane> pool_side;
    void retire_stream(Stream &st) { if (st) (st.high ? pool_high : pool_normal).push_back(std::move(st)); }
    void retire_streams()
    {
        for (uint32_t k = 0; k < (uint32_t)MAX_LANES; k++) {
            retire_stream(lanes[k]);
            if (lane_side[k].stream) pool_side.push_back(std::move(lane_side[k]));
        }
    }
    bool take_stream(Stream *st, bool high, int prio)
    {
        std::vector<Stream> &pool = high ? pool_high : pool_normal;
        if (!pool.empty()) { *st = std::move(pool.back()); pool.pop_back(); return true; }
        return (high ? st->create(prio) : st->create()) == hipSuccess;
    }
    bool take_side(SideLane *sl)
    {
        if (!pool_side.empty()) { *sl = std::move(pool_side.back()); pool_side.pop_back(); return true; }
        return sl->create(0, false);
    }
    std::vector<uint32_t> offsets;    /* first picture of every stream */
    /* what a schedule is built from (replay_schedule: at creation and again for every h264bsdmiReplayReschedule) */
    std::vector<FjHeader> heads;      /* the headers of the n_pics jobs (host copies) */
    std::vector<size_t> blob_off;     /* where job p lies inside a stream's blobs */
    size_t frames_per_stream = 0, dbk_half = 0, dbk_stride = 0;
    /* config 3 ("ARGB conversion on-GPU"): colour conversion of every produced picture inside the run, timed */
    int convert_fmt = -1;
    std::vector<Event> cev;           /* 2 per tick */
    /* ... hosted by the NEXT tick's k_frame_dbk where that is possible (kernels/convert.hip.h, conv_drain): descriptors with the
     * conversion of the stream's previous picture written in, which ticks host */
    DeviceMem<FrameDesc> d_desc_conv;
    std::vector<uint8_t> hosted;      /* tick i converts the pictures of tick i - 1 while it filters its own */
    std::vector<uint8_t> cev_on;      /* tick i was followed by a stand-alone conversion launch in the last run */
    bool host_convert = true, convert_trailing = true;
    uint32_t conv_waves = 0;
};

/* Descriptors and launch schedule of a replay set for the offsets in r->offsets: lock-step / staggered / common ticks
 * (heavy_lanes == 0, groups <= 1: tick i = picture (i + offset) mod n_pics of every stream) or the static schedule of
 * stream groups and heavy lanes (h264bsdmiReplayCreateDesync).  Called at creation and by h264bsdmiReplayReschedule,
 * which has torn the previous schedule down. */
static bool replay_schedule(h264bsdmi_replay *r, u32 heavy_lanes, u32 heavy_delay, u32 groups)
{
    Engine *e = r->e;
    const u32 n_pics = r->n_pics, n_streams = r->n_streams;
    const size_t total = r->blob_stride, frames_per_stream = r->frames_per_stream, dbk_stride = r->dbk_stride;
    const std::vector<size_t> &offs = r->blob_off;
    auto blob_of = [&](u32 p) { return reinterpret_cast<const uint8_t *>(&r->heads[p]); };     /* make_desc reads the header only */
    bool ok = true;
    r->shapes.assign(n_pics, TickShape());
    for (u32 i = 0; i < n_pics; i++) {
        TickShape s0;
        FrameDesc tmp;
        make_desc(tmp, blob_of(i), nullptr, nullptr, 0, nullptr, &s0, nullptr);
        s0.n_frames = n_streams;
        r->shapes[i] = s0;
    }
    if (ok) {
        std::vector<FrameDesc> descs((size_t)n_pics * n_streams);
        auto desc_of = [&](FrameDesc &d, u32 s, u32 p, TickShape *shape, u32 tick = 0) {
            make_desc(d, blob_of(p), r->d_blobs + (size_t)s * total + offs[p], r->d_frames + (size_t)s * frames_per_stream,
                      r->frame_bytes, r->d_dbk + (size_t)s * dbk_stride, shape, e->d_err);
        };
        if (!heavy_lanes && groups <= 1) {
            for (u32 i = 0; i < n_pics; i++) {
                TickShape shape;                          /* a tick is as large as the largest of its pictures */
                for (u32 s = 0; s < n_streams; s++) desc_of(descs[(size_t)i * n_streams + s], s, (i + r->offsets[s]) % n_pics, &shape, i);
                r->shapes[i] = shape;
            }
        } else {
            /* static schedule: every group's light ticks on its own lane, heavy pictures round-robin on the heavy lanes */
            std::vector<u32> done(n_streams, 0), ready_at(n_streams, 0);
            std::vector<int> last_ev(n_streams, -1);     /* event of the heavy launch a stream's previous picture ran in */
            size_t n_desc = 0;
            u32 left = n_streams, heavy_count = 0;
            auto is_heavy = [&](u32 p) { const FjHeader *h = reinterpret_cast<const FjHeader *>(blob_of(p)); return heavy_lanes && h->n_intra * 4u > h->n_mbs; };      /* (no heavy lanes: heavy pictures stay in their group's tick) */
            /* Cost-affine groups: a group's tick lasts as long as its slowest picture, so streams whose next pictures cost
             * about the same belong together.  Every REGROUP rounds the streams are sorted by the estimated per-picture
             * kernel time of their next REGROUP pictures (from the job headers: intra and filtered macroblock counts) and
             * dealt to the groups in that order; a stream that changes groups makes its new lane wait for the event its
             * old lane recorded after the last round before the regrouping. */
#ifndef REGROUP_ROUNDS
#define REGROUP_ROUNDS 32      /* measured: 4: 681, 8: 664, 16: 699, 32: 709-733 M MB/s (8-9 groups); every regrouping costs cross-lane waits */
#endif
            constexpr u32 REGROUP = REGROUP_ROUNDS;
            std::vector<std::vector<u32>> members(groups);
            std::vector<u32> group_of(n_streams, 0);
            std::vector<int> pre_regroup_ev(groups, -1);
            auto upcoming_cost = [&](u32 s) {
                uint64_t c = 0;
                for (u32 i = 0; i < REGROUP && done[s] + i < n_pics; i++) {
                    const FjHeader *h = &r->heads[(r->offsets[s] + done[s] + i) % n_pics];
                    c += 11u * h->n_intra + 4u * h->n_dbk;          /* ~0.55 us per intra macroblock, ~0.2 us per filtered one */
                }
                return c;
            };
            auto new_event = [&]() { r->sched_ev.emplace_back(); return (int)r->sched_ev.size() - 1; };
            for (u32 t = 0; left && t < 16u * n_pics; t++) {
                /* one heavy launch per round for the heavy pictures of all groups: it waits for the light launch of
                 * every group it takes a stream from (the previous picture of that stream ran there or earlier) */
                std::vector<u32> hs;
                std::vector<int> hwaits;
                if (t % REGROUP == 0) {
                    std::vector<std::pair<uint64_t, u32>> order;
                    for (u32 s = 0; s < n_streams; s++) if (done[s] < n_pics) order.emplace_back(upcoming_cost(s), s);
                    std::sort(order.begin(), order.end());
                    for (auto &m : members) m.clear();
                    for (size_t i = 0; i < order.size(); i++) {
                        const u32 s = order[i].second, g = (u32)(i * groups / order.size());
                        if (t && g != group_of[s] && last_ev[s] < 0) last_ev[s] = pre_regroup_ev[group_of[s]];
                        group_of[s] = g;
                        members[g].push_back(s);
                    }
                    for (auto &m : members) std::sort(m.begin(), m.end());
                }
                const bool before_regroup = (t + 1) % REGROUP == 0;
                for (u32 g = 0; g < groups; g++) {
                    h264bsdmi_replay::Launch light{ n_desc, TickShape(), (int)g, {}, -1, true };
                    bool group_has_heavy = false;
                    for (u32 s : members[g]) {
                        if (done[s] >= n_pics || ready_at[s] > t) continue;
                        const u32 p = (r->offsets[s] + done[s]) % n_pics;
                        if (is_heavy(p)) { hs.push_back(s); group_has_heavy = true; continue; }
                        if (last_ev[s] >= 0) {               /* rejoining after a heavy picture */
                            if (std::find(light.waits.begin(), light.waits.end(), last_ev[s]) == light.waits.end()) light.waits.push_back(last_ev[s]);
                            last_ev[s] = -1;
                        }
                        desc_of(descs[n_desc++], s, p, &light.shape);
                        if (++done[s] == n_pics) left--;
                    }
                    const bool have_light = light.shape.n_frames != 0;
                    if (have_light) {
                        if (group_has_heavy || before_regroup) light.record_ev = new_event();
                        if (group_has_heavy) hwaits.push_back(light.record_ev);
                        if (before_regroup) pre_regroup_ev[g] = light.record_ev;
                        light.shape.dbk_waves = LANE_DBK_WAVES;
                        r->sched.push_back(light);
                    } else {
                        if (group_has_heavy) hwaits.push_back(-2 - (int)g);        /* "everything enqueued on light lane g so far" */
                        if (before_regroup) {                                      /* an empty launch: only the event */
                            light.record_ev = pre_regroup_ev[g] = new_event();
                            r->sched.push_back(light);
                        }
                    }
                }
                if (!hs.empty()) {
                    h264bsdmi_replay::Launch heavy{ n_desc, TickShape(), (int)(groups + heavy_count++ % heavy_lanes), hwaits, -1, false };
                    for (u32 s : hs) {
                        if (last_ev[s] >= 0 && std::find(heavy.waits.begin(), heavy.waits.end(), last_ev[s]) == heavy.waits.end()) heavy.waits.push_back(last_ev[s]);
                        desc_of(descs[n_desc++], s, (r->offsets[s] + done[s]) % n_pics, &heavy.shape);
                        if (++done[s] == n_pics) left--;
                        ready_at[s] = t + 1 + heavy_delay;
                    }
                    heavy.record_ev = new_event();
                    for (u32 s : hs) last_ev[s] = heavy.record_ev;
                    r->sched.push_back(heavy);
                }
            }
            if (left || n_desc != descs.size()) ok = false;
            r->n_light = groups;
            r->n_lanes = groups + heavy_lanes;
            /* the heavy pictures' workgroups need a whole compute unit each: highest priority (measured: no
             * difference on this runtime, kept because it states the intent) */
            int prio_least = 0, prio_greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = 0;
            for (u32 k = 0; ok && k < r->n_lanes; k++) {
                if (k < groups) {
                    ok = r->take_stream(&r->lanes[k], false, 0);
                    if (ok && groups <= 2)        /* with more groups the other groups are the overlap, and busy HIP streams are scarce (Lane, above) */
                        ok = r->take_side(&r->lane_side[k]);
                } else ok = r->take_stream(&r->lanes[k], true, prio_greatest);
            }
            for (auto &ev : r->sched_ev) if (ok) ok = ev.create(hipEventDisableTiming) == hipSuccess;
        }
        if (ok) ok = hipMemcpyAsync(r->d_desc, descs.data(), descs.size() * sizeof(FrameDesc), hipMemcpyHostToDevice, e->stream) == hipSuccess &&
                     hipStreamSynchronize(e->stream) == hipSuccess;
    }
    return ok;
}

h264bsdmi_replay *h264bsdmiReplayCreate(const u8 *const *blobs, const u32 *bytes, u32 n_pics, u32 n_streams)
{
    return h264bsdmiReplayCreateDesync(blobs, bytes, n_pics, n_streams, nullptr, 0, 0);
}

/* odd_offset != 0: the "staggered" variant of SURVEY.md §8d config 4 — odd-numbered streams run picture
 * (i + odd_offset) mod n_pics in tick i (odd_offset must be the index of an IDR picture, so that both the
 * start and the wrap-around are clean decoder starts); every tick then mixes two different pictures */
h264bsdmi_replay *h264bsdmiReplayCreateStaggered(const u8 *const *blobs, const u32 *bytes, u32 n_pics, u32 n_streams, u32 odd_offset)
{
    if (odd_offset >= n_pics) return nullptr;
    std::vector<u32> offs(n_streams, 0);
    for (u32 s = 1; s < n_streams; s += 2) offs[s] = odd_offset;
    return h264bsdmiReplayCreateDesync(blobs, bytes, n_pics, n_streams, offs.data(), 0, 0);
}

/* Streams that are NOT in step: stream s starts at picture offsets[s] (nullptr = all 0) and runs n_pics pictures,
 * wrapping around (picture 0 must be an IDR picture).  heavy_lanes == 0: tick i holds picture (i + offsets[s]) mod
 * n_pics of every stream — a tick then lasts as long as its slowest picture.  heavy_lanes > 0: a static schedule of
 * what a scheduler achieves that keeps light pictures from waiting for heavy ones:
 *   - the streams are split into `groups` groups (stream s -> group s % groups), every group runs its own ticks on its
 *     own HIP stream ("light lane"): a group's tick lasts as long as ITS slowest picture, and the workgroups of the
 *     other groups fill the compute units it leaves idle (tail kernels are one workgroup per picture);
 *   - pictures that are mostly intra-coded ("heavy", more than a quarter of their macroblocks) leave their group's
 *     tick and run on one of heavy_lanes extra HIP streams; their stream of pictures rejoins its group heavy_delay
 *     ticks later (an event makes the group's tick wait if the heavy picture is not finished by then). */
h264bsdmi_replay *h264bsdmiReplayCreateDesync(const u8 *const *blobs, const u32 *bytes, u32 n_pics, u32 n_streams,
                                              const u32 *offsets, u32 heavy_lanes, u32 heavy_delay)
{
    return h264bsdmiReplayCreateSched(blobs, bytes, n_pics, n_streams, offsets, heavy_lanes, heavy_delay, 1);
}

h264bsdmi_replay *h264bsdmiReplayCreateSched(const u8 *const *blobs, const u32 *bytes, u32 n_pics, u32 n_streams,
                                             const u32 *offsets, u32 heavy_lanes, u32 heavy_delay, u32 groups)
{
    if (groups < 1) groups = 1;
    if (groups > 16 || groups > n_streams) return nullptr;
    if (heavy_lanes + groups > (u32)h264bsdmi_replay::MAX_LANES) return nullptr;
    for (u32 s = 0; offsets && s < n_streams; s++) if (offsets[s] >= n_pics) return nullptr;
    Engine *e = engine_get();
    if (!e || !n_pics || !n_streams) {
        if (!e) fprintf(stderr, "h264bsd-mi355x: h264bsdmiReplayCreate: no usable HIP device\n");
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    if (hipSetDevice(e->device) != hipSuccess) return nullptr;
    h264bsdmi_replay *r = new h264bsdmi_replay();
    r->e = e; r->n_pics = n_pics; r->n_streams = n_streams;
    r->offsets.assign(n_streams, 0);
    if (offsets) r->offsets.assign(offsets, offsets + n_streams);
    const FjHeader *h0 = reinterpret_cast<const FjHeader *>(blobs[0]);
    r->wmb = h0->width_mbs; r->hmb = h0->height_mbs; r->n_slots = h0->n_slots;
    r->frame_bytes = fj_frame_bytes(r->wmb, r->hmb);
    std::vector<size_t> offs(n_pics);
    size_t total = 0;
    r->job_bytes = 0;
    for (u32 i = 0; i < n_pics; i++) { offs[i] = total; total += ((size_t)bytes[i] + 255u) & ~(size_t)255u; r->job_bytes += bytes[i]; }
    r->blob_stride = total;
    r->blob_off = offs;
    const size_t frames_per_stream = (size_t)r->n_slots * r->frame_bytes;
    const size_t dbk_half = (DBK_SCRATCH_BYTES(h0->n_mbs) + 255) & ~(size_t)255, dbk_stride = dbk_half;
    r->frames_per_stream = frames_per_stream; r->dbk_half = dbk_half; r->dbk_stride = dbk_stride;
    bool ok = r->d_blobs.alloc(total * n_streams) == hipSuccess &&
              r->d_frames.alloc(frames_per_stream * n_streams + 256) == hipSuccess &&
              r->d_desc.alloc(sizeof(FrameDesc) * (size_t)n_pics * n_streams) == hipSuccess &&
              r->d_sums.alloc(sizeof(unsigned long long) * n_streams) == hipSuccess &&
              r->d_dbk.alloc((size_t)n_streams * dbk_stride) == hipSuccess;
    if (ok) ok = hipMemsetAsync(r->d_dbk, 0, (size_t)n_streams * dbk_stride, e->stream) == hipSuccess;
    if (ok) ok = hipMemsetAsync(r->d_frames, 0, frames_per_stream * n_streams + 256, e->stream) == hipSuccess;
    /* stream 0 from the host, the other copies device-to-device: every stream owns private jobs */
    for (u32 i = 0; ok && i < n_pics; i++) {
        ok = hipMemcpyAsync(r->d_blobs + offs[i], blobs[i], bytes[i], hipMemcpyHostToDevice, e->stream) == hipSuccess;
        const FjHeader *h = reinterpret_cast<const FjHeader *>(blobs[i]);
        if (h->width_mbs != r->wmb || h->height_mbs != r->hmb || h->n_slots != r->n_slots) ok = false;
        r->heads.push_back(*h);
        r->cur_slot.push_back(h->cur_slot);
    }
    if (ok) ok = hipStreamSynchronize(e->stream) == hipSuccess;
    for (u32 s = 1; ok && s < n_streams; s++)
        ok = hipMemcpyAsync(r->d_blobs + (size_t)s * total, r->d_blobs, total, hipMemcpyDeviceToDevice, e->stream) == hipSuccess;
    if (ok) ok = replay_schedule(r, heavy_lanes, heavy_delay, groups);
    r->timers.resize(n_pics);
    for (auto &t : r->timers) {
        for (auto &ev : t.ev) if (ok) ok = ev.create() == hipSuccess;
        for (auto &ev : t.sev) if (ok) ok = ev.create() == hipSuccess;
    }
    if (ok) ok = r->ev_begin.create() == hipSuccess && r->ev_end.create() == hipSuccess && r->gdone_any.create(hipEventDisableTiming) == hipSuccess;
    r->timed_first = r->timed_count = 0;
    r->stages = 7u;
    r->n_groups = 1;
    if (!ok) {
        fprintf(stderr, "h264bsd-mi355x: h264bsdmiReplayCreate failed (%s)\n", hipGetErrorString(hipGetLastError()));
        delete r;
        return nullptr;
    }
    return r;
}

void h264bsdmiReplayDestroy(h264bsdmi_replay *r)
{
    if (!r) return;
    std::lock_guard<std::mutex> lk(r->e->mu);
    hipSetDevice(r->e->device);
    hipStreamSynchronize(r->e->stream);           /* (every lane and stream group of the set is joined into it: h264bsdmiReplayRun) */
    delete r;
}

/* The same resident jobs and frame buffers under another schedule (other first pictures, heavy lanes, stream groups): what
 * a second h264bsdmiReplayCreate* would build, without allocating and uploading 20 GB again.  Frame buffers and deblocking
 * scratch start from zero like those of a new set.  0 = ok; after a failure the set can only be destroyed. */
int h264bsdmiReplayReschedule(h264bsdmi_replay *r, const u32 *offsets, u32 heavy_lanes, u32 heavy_delay, u32 groups)
{
    if (!r) return -1;
    if (groups < 1) groups = 1;
    if (groups > 16 || groups > r->n_streams || heavy_lanes + groups > (u32)h264bsdmi_replay::MAX_LANES) return -1;
    for (u32 s = 0; offsets && s < r->n_streams; s++) if (offsets[s] >= r->n_pics) return -1;
    Engine *e = r->e;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    /* everything the old schedule launched has to be over before its streams and events go */
    for (auto &st : r->lanes) if (st) HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < 8; g++) if (r->gstream[g]) HIP_TRY(hipStreamSynchronize(r->gstream[g]));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (poll_errors(e)) return -1;
    r->sched_ev.clear(); r->sched.clear();
    r->retire_streams();                               /* (kept for the next schedule: h264bsdmi_replay::pool_*) */
    for (auto &st : r->gstream) r->retire_stream(st);  /* h264bsdmiReplaySetGroups takes them back */
    r->n_lanes = r->n_light = 0;
    r->n_groups = 1;                                  /* (h264bsdmiReplaySetGroups: a property of the schedule it was set for) */
    r->convert_fmt = -1; r->timed_mask = 31u; r->stages = 7u;
    r->offsets.assign(r->n_streams, 0);
    if (offsets) r->offsets.assign(offsets, offsets + r->n_streams);
    HIP_TRY(hipMemsetAsync(r->d_dbk, 0, (size_t)r->n_streams * r->dbk_stride, e->stream));
    HIP_TRY(hipMemsetAsync(r->d_frames, 0, r->frames_per_stream * r->n_streams + 256, e->stream));
    if (!replay_schedule(r, heavy_lanes, heavy_delay, groups)) return -1;
    r->timed_first = r->timed_count = 0;
    return 0;
}

int h264bsdmiReplayRun(h264bsdmi_replay *r, u32 first, u32 count)
{
    if (!r || first + count > r->n_pics) return -1;
    std::lock_guard<std::mutex> lk(r->e->mu);
    HIP_TRY(hipSetDevice(r->e->device));
    r->timed_first = first; r->timed_count = count;
    for (auto &l : r->launches) l = 0;
    HIP_TRY(hipEventRecord(r->ev_begin, r->e->stream));
    if (!r->sched.empty()) {
        /* desynchronised set with lanes: one whole lap of the static schedule (first / count are ignored) */
        r->timed_count = 0;
        for (u32 k = 0; k < r->n_lanes; k++) HIP_TRY(hipStreamWaitEvent(r->lanes[k], r->ev_begin, 0));   /* the previous lap is complete */
        std::vector<hipEvent_t> lane_mark(r->n_light, nullptr);
        for (const auto &l : r->sched) {
            hipStream_t st = r->lanes[l.lane];
            for (int w : l.waits) {
                if (w >= 0) HIP_TRY(hipStreamWaitEvent(st, r->sched_ev[w], 0));
                else {                                   /* -2 - g: everything enqueued on light lane g so far */
                    HIP_TRY(hipEventRecord(r->gdone_any, r->lanes[-2 - w]));
                    HIP_TRY(hipStreamWaitEvent(st, r->gdone_any, 0));
                }
            }
            if (l.shape.n_frames && launch_tick(st, r->d_desc + l.first, [&] { TickShape sh = l.shape; sh.load = r->n_streams; return sh; }(), nullptr, r->launches, r->stages,
                                                (l.light && r->overlap_dbk && !(r->stages & 8u) && r->lane_side[l.lane].stream) ? &r->lane_side[l.lane] : nullptr)) return -1;
            if (l.record_ev >= 0) HIP_TRY(hipEventRecord(r->sched_ev[l.record_ev], st));
        }
        for (u32 k = 0; k < r->n_lanes; k++) {               /* the lap ends when every lane has drained */
            HIP_TRY(hipEventRecord(r->gdone_any, r->lanes[k]));
            HIP_TRY(hipStreamWaitEvent(r->e->stream, r->gdone_any, 0));
        }
    } else if (r->n_groups <= 1) {
        for (u32 i = first; i < first + count; i++) { r->timers[i].on = true; r->timers[i].mask = r->timed_mask; }
        r->cev_on.assign(r->n_pics, 0);
        for (u32 i = first; i < first + count; i++) {
            /* config 3: the pictures of tick i - 1 are converted by tick i's k_frame_dbk workgroups where the schedule allows it */
            const bool host = r->convert_fmt >= 0 && r->host_convert && i > first && r->hosted[i];
            TickShape shape = r->shapes[i];
            shape.conv = host; shape.conv_waves = r->conv_waves;
            if (launch_tick(r->e->stream, (host ? r->d_desc_conv : r->d_desc) + (size_t)i * r->n_streams, shape, &r->timers[i], r->launches, r->stages, (r->overlap_dbk && !(r->stages & 8u)) ? &r->e->side : nullptr, r->e->tail_prof)) return -1;
            const bool next_hosts = r->convert_fmt >= 0 && r->host_convert && i + 1 < first + count && r->hosted[i + 1];
            if (r->convert_fmt >= 0 && !next_hosts && (r->convert_trailing || i + 1 < first + count)) {
                /* the picture every stream has just produced, converted where it lies (tiles -> packed 32-bit pixels) */
                const uint32_t w = r->wmb * 16, h = r->hmb * 16;
                HIP_TRY(hipEventRecord(r->cev[2 * i], r->e->stream));
                hipLaunchKernelGGL(h264k::k_convert_tiles, CONVERT_GRID(r->n_streams), dim3(256), 0, r->e->stream,
                                   r->d_frames + (size_t)r->cur_slot[i] * r->frame_bytes, r->d_conv, r->wmb, r->hmb, r->convert_fmt,
                                   (size_t)r->n_slots * r->frame_bytes, (size_t)w * h);
                HIP_TRY(hipEventRecord(r->cev[2 * i + 1], r->e->stream));
                r->cev_on[i] = 1;
            }
        }
    } else {
        /* stream groups on separate HIP streams: the latency-bound per-picture tail of one group overlaps
         * with the throughput-bound inter reconstruction of another (pictures of different streams are
         * independent; every group still runs its own pictures strictly in order) */
        const u32 G = r->n_groups, per = (r->n_streams + G - 1) / G;
        for (u32 g = 0; g < G; g++) HIP_TRY(hipStreamWaitEvent(r->gstream[g], r->ev_begin, 0));
        for (u32 i = first; i < first + count; i++) {
            for (u32 g = 0; g < G; g++) {
                const u32 s0 = g * per, s1 = std::min(r->n_streams, s0 + per);
                if (s0 >= s1) continue;
                TickShape sh = r->shapes[i];
                sh.n_frames = s1 - s0;
                sh.load = r->n_streams;
                TickTimers &tt = r->timers[(size_t)g * r->n_pics + i];
                tt.on = true; tt.mask = r->timed_mask;
                /* (making the groups take turns at the list-driven kernels — a ring of events — works as designed in the kernel
                 * trace and loses: docs/EXPERIMENTS.md) */
                if (i == first && g > 0) HIP_TRY(hipStreamWaitEvent(r->gstream[g], r->timers[(size_t)(g - 1) * r->n_pics + i].ev[3], 0));
                if (launch_tick(r->gstream[g], r->d_desc + (size_t)i * r->n_streams + s0, sh, &tt, r->launches, r->stages)) return -1;
            }
        }
        for (u32 g = 0; g < G; g++) {
            HIP_TRY(hipEventRecord(r->gdone[g], r->gstream[g]));
            HIP_TRY(hipStreamWaitEvent(r->e->stream, r->gdone[g], 0));
        }
    }
    HIP_TRY(hipEventRecord(r->ev_end, r->e->stream));
    return 0;
}

int h264bsdmiReplaySetGroups(h264bsdmi_replay *r, u32 n_groups)
{
    if (!r || n_groups < 1 || n_groups > 8) return -1;
    std::lock_guard<std::mutex> lk(r->e->mu);
    HIP_TRY(hipSetDevice(r->e->device));
    while (r->timers.size() < (size_t)n_groups * r->n_pics) {
        TickTimers t;
        for (auto &ev : t.ev) HIP_TRY(ev.create());
        r->timers.push_back(std::move(t));
    }
    for (u32 g = 0; g < n_groups; g++) {
        if (!r->gstream[g] && !r->take_stream(&r->gstream[g], false, 0)) return -1;
        if (!r->gdone[g]) HIP_TRY(r->gdone[g].create(hipEventDisableTiming));
    }
    r->n_groups = n_groups;
    return 0;
}

int h264bsdmiReplaySync(h264bsdmi_replay *r)
{
    if (!r) return -1;
    HIP_TRY(hipSetDevice(r->e->device));
    HIP_TRY(hipStreamSynchronize(r->e->stream));
    return 0;
}

int h264bsdmiReplayTimings(h264bsdmi_replay *r, float out_ms[6], u32 launches[5])
{
    if (!r) return -1;
    HIP_TRY(hipSetDevice(r->e->device));
    HIP_TRY(hipStreamSynchronize(r->e->stream));
    for (int k = 0; k < 6; k++) out_ms[k] = 0.f;
    for (u32 g = 0; g < r->n_groups; g++)
        for (u32 i0 = r->timed_first; i0 < r->timed_first + r->timed_count; i0++) {
            const size_t i = (size_t)g * r->n_pics + i0;
            for (int k = 0; k < 5; k++) {
                float ms;
                if (!((r->timed_mask >> k) & 1u)) continue;
                HIP_TRY(hipEventElapsedTime(&ms, r->timers[i].ev[k], r->timers[i].ev[k + 1]));
                out_ms[k] += ms;
            }
            if ((r->timed_mask & 4u) && r->overlap_dbk && !(r->stages & 8u) && r->n_groups == 1 && r->timers[i].sev[0] &&
                hipEventQuery(r->timers[i].sev[2]) == hipSuccess) {
                float ms;                                /* k_dbk ran on the side stream, next to the kernels above */
                if (hipEventElapsedTime(&ms, r->timers[i].sev[1], r->timers[i].sev[2]) == hipSuccess) out_ms[2] += ms;
            }
            if (r->timers[i].copy_timed && hipEventQuery(r->timers[i].sev[4]) == hipSuccess) {
                float ms;                                /* and so did k_copy, on a stream of its own (zero when the tick had no copy to launch) */
                if (hipEventElapsedTime(&ms, r->timers[i].sev[3], r->timers[i].sev[4]) == hipSuccess) out_ms[0] += ms;
            }
        }
    if (r->timed_count || !r->sched.empty()) HIP_TRY(hipEventElapsedTime(&out_ms[5], r->ev_begin, r->ev_end));
    if (launches) for (int k = 0; k < 5; k++) launches[k] = r->launches[k];
    /* (the side-stream events of a tick that launched no k_dbk were never recorded: the elapsed-time queries above fail by design,
     * and what they leave in the runtime's last-error slot would fail the next run's launch_tick) */
    (void)hipGetLastError();
    return 0;
}

int h264bsdmiReplayFetch(h264bsdmi_replay *r, u32 stream, u32 slot, u8 *dst)
{
    if (!r || stream >= r->n_streams || slot >= r->n_slots) return -1;
    HIP_TRY(hipSetDevice(r->e->device));
    std::lock_guard<std::mutex> lk(r->e->mu);
    if (!r->d_planar) HIP_TRY(r->d_planar.alloc(r->frame_bytes));
    hipLaunchKernelGGL(h264k::k_detile, dim3(512, 1), dim3(256), 0, r->e->stream, r->d_frames + ((size_t)stream * r->n_slots + slot) * r->frame_bytes,
                       r->d_planar, r->wmb, r->hmb, (size_t)0, (size_t)0);
    HIP_TRY(hipMemcpyAsync(dst, r->d_planar, r->frame_bytes, hipMemcpyDeviceToHost, r->e->stream));
    HIP_TRY(hipStreamSynchronize(r->e->stream));
    return 0;
}

/* k_dbk alone for the descriptors of tick `picture`, then what it left in the deblocking scratch of `stream`: the n_mbs 48-byte records
 * and the n4 flag bytes behind them (DBK_SCRATCH_BYTES).  The flag bytes of every stream of the tick are zeroed again afterwards: "flags are
 * zero between pictures" is what k_frame_dbk's last band normally restores.  Lock-step sets with one group only. */
int h264bsdmiReplayDbkRecords(h264bsdmi_replay *r, u32 picture, u32 stream, u8 *dst, u32 bytes)
{
    if (!r || picture >= r->n_pics || stream >= r->n_streams || !r->sched.empty() || r->n_groups > 1) return -1;
    const size_t n_mbs = (size_t)r->wmb * r->hmb, n4 = (n_mbs + 3u) & ~(size_t)3u;
    if (!dst || bytes != n_mbs * DBK_REC_BYTES + n4) return -1;
    Engine *e = r->e;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const TickShape &s = r->shapes[picture];
    if (s.any_deblock && s.max_dbk) {
        launch_kdbk(e->stream, r->d_desc + (size_t)picture * r->n_streams, s, nullptr);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(dst, r->d_dbk + (size_t)stream * r->dbk_stride, bytes, hipMemcpyDeviceToHost, e->stream));
    for (u32 k = 0; k < r->n_streams; k++)
        HIP_TRY(hipMemsetAsync(r->d_dbk + (size_t)k * r->dbk_stride + n_mbs * DBK_REC_BYTES, 0, n4, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

int h264bsdmiReplayChecksums(h264bsdmi_replay *r, u32 slot, unsigned long long *sums)
{
    if (!r || slot >= r->n_slots) return -1;
    std::lock_guard<std::mutex> lk(r->e->mu);
    HIP_TRY(hipSetDevice(r->e->device));
    hipLaunchKernelGGL(h264k::k_checksum, dim3(r->n_streams), dim3(256), 0, r->e->stream,
                       r->d_frames + (size_t)slot * r->frame_bytes, (size_t)r->n_slots * r->frame_bytes, r->wmb, r->hmb, r->d_sums);
    HIP_TRY(hipMemcpyAsync(sums, r->d_sums, sizeof(unsigned long long) * r->n_streams, hipMemcpyDeviceToHost, r->e->stream));
    if (poll_errors(r->e)) return -1;
    return 0;
}

int h264bsdmiReplayConvert(h264bsdmi_replay *r, u32 slot, int fmt)
{
    if (!r || slot >= r->n_slots || fmt < 0 || fmt > 2) return -1;
    std::lock_guard<std::mutex> lk(r->e->mu);
    HIP_TRY(hipSetDevice(r->e->device));
    const uint32_t w = r->wmb * 16, h = r->hmb * 16;
    if (!r->d_conv) HIP_TRY(r->d_conv.alloc((size_t)w * h * 4 * r->n_streams));
    hipLaunchKernelGGL(h264k::k_convert_tiles, CONVERT_GRID(r->n_streams), dim3(256), 0, r->e->stream,
                       r->d_frames + (size_t)slot * r->frame_bytes, r->d_conv, r->wmb, r->hmb, fmt,
                       (size_t)r->n_slots * r->frame_bytes, (size_t)w * h);
    HIP_TRY(hipGetLastError());
    return 0;
}

int h264bsdmiReplayFetchConverted(h264bsdmi_replay *r, u32 stream, u32 *dst)
{
    if (!r || stream >= r->n_streams || !r->d_conv) return -1;
    HIP_TRY(hipSetDevice(r->e->device));
    HIP_TRY(hipStreamSynchronize(r->e->stream));
    const size_t n = (size_t)r->wmb * 16 * r->hmb * 16;
    HIP_TRY(hipMemcpy(dst, r->d_conv + (size_t)stream * n, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* fmt 0..2: every h264bsdmiReplayRun() tick (lock-step sets, one group) is followed by the colour conversion of the
 * pictures it produced, inside the timed region; fmt < 0: off.  h264bsdmiReplayConvertTimings: k_convert time of the last run. */
int h264bsdmiReplaySetConvert(h264bsdmi_replay *r, int fmt_and_flags)
{
    /* flags (tests and A/B runs): 0x100 = no conversion launch behind the LAST tick of a run (what the conversion buffer then holds
     * is the work of the last tick's hosts), 0x200 = no hosting (every tick followed by its own conversion launch) */
    const int fmt = fmt_and_flags < 0 ? -1 : (fmt_and_flags & 0xFF);
    const bool no_trailing = fmt_and_flags >= 0 && (fmt_and_flags & 0x100), no_hosting = fmt_and_flags >= 0 && (fmt_and_flags & 0x200);
    if (!r || fmt > 2 || !r->sched.empty()) return -1;
    std::lock_guard<std::mutex> lk(r->e->mu);
    HIP_TRY(hipSetDevice(r->e->device));
    if (fmt >= 0) {
        const size_t n = (size_t)r->wmb * 16 * r->hmb * 16;
        if (!r->d_conv) HIP_TRY(r->d_conv.alloc(n * 4 * r->n_streams));
        while (r->cev.size() < 2 * (size_t)r->n_pics) { Event ev; HIP_TRY(ev.create()); r->cev.push_back(std::move(ev)); }
        /* Hosting.  Tick i can
         * convert the pictures of tick i - 1 while it decodes its own if no stream decodes INTO the frame buffer its previous
         * picture lies in (an IDR picture may); the stand-alone launch converts one frame buffer number for all streams, so the
         * streams have to be in step. */
        HIP_TRY(hipStreamSynchronize(r->e->stream));
        r->host_convert = !no_hosting;
        r->convert_trailing = !no_trailing;
        r->conv_waves = ((uint32_t)fmt_and_flags >> 16) & 15u;
        bool in_step = true;
        for (u32 s = 1; s < r->n_streams; s++) if (r->offsets[s] != r->offsets[0]) in_step = false;
        r->hosted.assign(r->n_pics, 0);
        for (u32 i = 1; in_step && i < r->n_pics; i++) r->hosted[i] = r->cur_slot[i] != r->cur_slot[i - 1];
        const size_t n_desc = (size_t)r->n_pics * r->n_streams;
        if (!r->d_desc_conv) HIP_TRY(r->d_desc_conv.alloc(sizeof(FrameDesc) * n_desc));
        std::vector<FrameDesc> descs(n_desc);
        HIP_TRY(hipMemcpy(descs.data(), r->d_desc, sizeof(FrameDesc) * n_desc, hipMemcpyDeviceToHost));
        for (u32 i = 1; i < r->n_pics; i++)
            for (u32 s = 0; s < r->n_streams && r->hosted[i]; s++) {
                FrameDesc &d = descs[(size_t)i * r->n_streams + s];
                d.conv_src = r->d_frames + (size_t)s * r->frames_per_stream + (size_t)r->cur_slot[i - 1] * r->frame_bytes;
                d.conv_dst = r->d_conv + (size_t)s * n;
                d.conv_fmt = (uint32_t)fmt;
            }
        HIP_TRY(hipMemcpy(r->d_desc_conv, descs.data(), sizeof(FrameDesc) * n_desc, hipMemcpyHostToDevice));
    }
    r->convert_fmt = fmt;
    return 0;
}

int h264bsdmiReplayConvertTimings(h264bsdmi_replay *r, float *ms, u32 *launches)
{
    if (!r || r->convert_fmt < 0) return -1;
    HIP_TRY(hipSetDevice(r->e->device));
    HIP_TRY(hipStreamSynchronize(r->e->stream));
    *ms = 0.f; *launches = 0;
    for (u32 i = r->timed_first; i < r->timed_first + r->timed_count; i++) {
        float t;
        if (i >= r->cev_on.size() || !r->cev_on[i]) continue;      /* converted by the next tick's k_frame_dbk: no launch of its own */
        HIP_TRY(hipEventElapsedTime(&t, r->cev[2 * i], r->cev[2 * i + 1]));
        *ms += t; (*launches)++;
    }
    return 0;
}

int h264bsdmiReplaySetTimedKernels(h264bsdmi_replay *r, unsigned mask)
{
    if (!r) return -1;
    r->timed_mask = mask & 31u;     /* bit k: HIP events around kernel k (k_copy, k_recon_inter, k_dbk, k_frame_intra, k_frame_dbk) */
    return 0;
}

int h264bsdmiReplaySetStages(h264bsdmi_replay *r, unsigned mask)
{
    if (!r) return -1;
    r->stages = mask & 15u;        /* bit 3: keep k_dbk on the main stream (no overlap) */
    return 0;
}

/* Debug hook: cycle accounting of k_frame_tail's deblocking loop (workgroup 0 of the next launches).
 * out[16][8]: per wave {pick, filter, extra rounds, own-memory wait, filtered count, barrier wait}. */
int h264bsdmiDebugTailProfile(int enable, unsigned long long *out)
{
    Engine *e = engine_get();
    if (!e) return -1;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    if (enable) {
        if (!e->tail_prof) HIP_TRY(e->tail_prof.alloc((16 * 16 + 16 * 8) * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(e->tail_prof, 0, (16 * 16 + 16 * 8) * sizeof(unsigned long long)));
        HIP_TRY(hipDeviceSynchronize());
    } else if (e->tail_prof) {
        if (out) HIP_TRY(hipMemcpy(out, e->tail_prof, (16 * 16 + 16 * 8) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        e->tail_prof.reset();
    }
    return 0;
}

/* Test / tuning hook: how the per-picture kernels split pictures from now on (TailConfig; descriptors built earlier keep their
 * bands): rows per band for light and heavy pictures (0 = one band) and wavefronts per workgroup, for k_frame_dbk and
 * k_frame_intra.  A value of 0xFFFFFFFF leaves that setting alone. */
int h264bsdmiDebugSetTail(u32 dbk_rows_light, u32 dbk_rows_heavy, u32 dbk_waves, u32 intra_rows_light, u32 intra_rows_heavy, u32 intra_waves, u32 band_budget)
{
    (void)tail_config();                                     /* the environment first, once */
    std::lock_guard<std::mutex> lk(g_tail_mu);
    if (dbk_rows_light != 0xFFFFFFFFu) g_tail.dbk_rows_light = dbk_rows_light;
    if (dbk_rows_heavy != 0xFFFFFFFFu) g_tail.dbk_rows_heavy = dbk_rows_heavy;
    if (dbk_waves != 0xFFFFFFFFu && dbk_waves >= 1) g_tail.dbk_waves = dbk_waves;
    if (intra_rows_light != 0xFFFFFFFFu) g_tail.intra_rows_light = intra_rows_light;
    if (intra_rows_heavy != 0xFFFFFFFFu) g_tail.intra_rows_heavy = intra_rows_heavy;
    if (intra_waves != 0xFFFFFFFFu && intra_waves >= 1) g_tail.intra_waves = intra_waves;
    if (band_budget != 0xFFFFFFFFu) g_tail.band_budget = band_budget;
    return 0;
}

unsigned long long h264bsdmiReplayJobBytes(h264bsdmi_replay *r) { return r ? r->job_bytes : 0; }
u32 h264bsdmiReplayFrameBytes(h264bsdmi_replay *r) { return r ? r->frame_bytes : 0; }
} /* extern "C" */
