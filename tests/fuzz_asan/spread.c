/* What the host path of the background spread (api.c: h264bsdmiBlendCurrentPicturesSpread, h264bsdmiOutputKeptSpread, and the SPREAD
 * mode of h264bsdmiOutputCellMaps / h264bsdmiOutputCellBoxes) hands to the engine, without a GPU: bound to tests/fuzz_asan/mock_engine.c
 * as it stands and to the eng_sink_entries below, a table with all SIX entries behind the last member of JobSink (engine.h), whose
 * blend_spread and kept_spread_out record what they are given (the four older entries only say that they were called: nothing here may
 * reach them).  A sink is left without the two new entries by naming it in f_without: its table has the first four members only, as a
 * table written before them has.  Prints per call "#name", rc, the entry's record and the sink's, or "sink: not called", then the
 * output arrays, which start as a sentinel.  tests/test_spread_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: spread <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A (640x360 in a coded 640x368, picIds from 100) and B (1920x1080 in 1920x1088, from 200) fed and popped; C never fed
 * anything; D as A, picIds from 500, which keeps nothing before its first spread blend; O on a sink whose table lacks the entries; G capture
 * mode. */
#include <stdarg.h>
#include "host_harness.h"
#include "engine.h"

static const void *f_without;                   /* JobSink.user of the sink named above */
static char f_rec[4096];
static size_t f_len;
static int f_fail;
static void *const *f_users;
static u32 f_n;
static void frec(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (f_len < sizeof(f_rec) - 1) {
        const int w = vsnprintf(f_rec + f_len, sizeof(f_rec) - f_len, fmt, ap);
        if (w > 0) f_len = f_len + (size_t)w < sizeof(f_rec) ? f_len + (size_t)w : sizeof(f_rec) - 1;
    }
    va_end(ap);
}
static int f_inst(const SinkTensorPic *p)
{
    for (u32 j = 0; j < f_n; j++) if (f_users[j] == p->sink->user) return (int)j;
    return -1;
}
static int f_cell_shift(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const struct h264bsdmi_cell_shift_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    frec("flow m=%u k=%u\n", n, k);
    return -1;
}
static int f_point_matches(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const struct h264bsdmi_matches_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    frec("matches m=%u k=%u\n", n, k);
    return -1;
}
static int f_point_model(const JobSink *sink, uint32_t n_records, const struct h264bsdmi_model_spec *s, void *stream)
{
    (void)sink; (void)s; (void)stream;
    frec("model records=%u\n", n_records);
    return -1;
}
static int f_warp_kept(uint32_t n, const SinkTensorPic *p, const struct h264bsdmi_warp_map *m, const struct h264bsdmi_warp_spec *s, uint32_t n_count,
                       void *stream)
{
    (void)p; (void)m; (void)s; (void)stream;
    frec("warp m=%u n_count=%u\n", n, n_count);
    return -1;
}
/* the two entries under test: the pictures (each sink named by its instance's place in the call) with their flags, both specs, the stream */
static int f_blend_spread(uint32_t n, const SinkTensorPic *p, const uint32_t *flags, const struct h264bsdmi_blend_spec *s,
                          const struct h264bsdmi_spread_spec *v, uint32_t n_moving, void *stream)
{
    frec("blend_spread m=%u n_moving=%u stream=0x%llx\n", n, n_moving, (unsigned long long)(uintptr_t)stream);
    for (uint32_t i = 0; i < n; i++)
        frec(" pic %d index=%u slot=%u win=%u,%u,%u,%u fresh=%u unset=%u\n", f_inst(&p[i]), p[i].index, p[i].slot, p[i].x0, p[i].y0, p[i].w, p[i].h,
             flags[i] & ENG_SPREAD_FRESH ? 1u : 0u, flags[i] & ENG_SPREAD_UNSET ? 1u : 0u);
    frec(" spec shift=%u hold=%u moving_shift=%u moving=0x%llx\n", s->shift, s->hold, s->moving_shift, (unsigned long long)(uintptr_t)s->moving);
    frec(" spread gain=%u lowest=%u highest=%u update=%u\n", v->gain, v->lowest, v->highest, v->update);
    return f_fail ? -1 : 0;
}
static int f_kept_spread_out(uint32_t n, const SinkTensorPic *p, void *const *spread, void *stream)
{
    frec("spread_out m=%u stream=0x%llx\n", n, (unsigned long long)(uintptr_t)stream);
    for (uint32_t i = 0; i < n; i++) frec(" inst %d spread=0x%llx\n", f_inst(&p[i]), (unsigned long long)(uintptr_t)spread[i]);
    return f_fail ? -1 : 0;
}
const EngSinkEntries *eng_sink_entries(const JobSink *sink)
{
    static const EngSinkEntries with = { f_cell_shift, f_point_matches, f_point_model, f_warp_kept, f_blend_spread, f_kept_spread_out },
                                without = { f_cell_shift, f_point_matches, f_point_model, f_warp_kept };
    return sink->user == f_without ? &without : &with;
}

static void begin(u32 n, Inst *const *inst, storage_t **dec, void **users, int fail)
{
    aim(n, inst, dec, users, 0);
    f_fail = fail; f_users = users; f_n = n; f_len = 0; f_rec[0] = 0;
}
static void print_head(const char *name, int rc)
{
    printf("#%s\nrc=%d\n%s%s%s", name, rc, f_rec, mock_record(), *f_rec || *mock_record() ? "" : "sink: not called\n");
}
/* flags: 1 a stream is named; 2 the blend spec is NULL; 4 the instance array is NULL; 16 the entry fails; 32 kept is NULL; 64 the spread
 * spec is NULL; 128 the plain blend (no spread spec in the signature) */
static void blend(const char *name, u32 n, Inst *const *inst, const h264bsdmi_blend_spec *spec, const h264bsdmi_spread_spec *spread, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 kept[4] = { SENT, SENT, SENT, SENT }, blended[4] = { SENT, SENT, SENT, SENT }, ids[4] = { SENT, SENT, SENT, SENT };
    void *const stream = flags & 1 ? (void *)(uintptr_t)0x5000 : NULL;
    begin(n, inst, dec, users, (flags & 16) != 0);
    const int rc = flags & 128 ? h264bsdmiBlendCurrentPictures(n, dec, spec, stream, kept, blended, ids)
                               : h264bsdmiBlendCurrentPicturesSpread(n, flags & 4 ? NULL : dec, flags & 2 ? NULL : spec, flags & 64 ? NULL : spread, stream,
                                                                     flags & 32 ? NULL : kept, blended, ids);
    print_head(name, rc);
    show("kept", kept, n, 1); show("blended", blended, n, 1); show("picId", ids, n, 1);
}
/* flags: 1 a stream is named; 16 the entry fails */
static void spread_out(const char *name, u32 n, Inst *const *inst, void *const *bufs, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[4] = { SENT, SENT, SENT, SENT }, ids[4] = { SENT, SENT, SENT, SENT };
    begin(n, inst, dec, users, (flags & 16) != 0);
    const int rc = h264bsdmiOutputKeptSpread(n, dec, bufs, flags & 1 ? (void *)(uintptr_t)0x5000 : NULL, got, ids);
    print_head(name, rc);
    show("got", got, n, 1); show("keptPicId", ids, n, 1);
}
/* the cell maps (boxes NULL) or the cell boxes over whole windows, one region per instance */
static void cells(const char *name, u32 n, Inst *const *inst, const h264bsdmi_cells_spec *spec, const h264bsdmi_boxes_spec *boxes)
{
    storage_t *dec[4]; void *users[4];
    u32 got[4] = { SENT, SENT, SENT, SENT }, arr[4][4];
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    begin(n, inst, dec, users, 0);
    const int rc = boxes ? h264bsdmiOutputCellBoxes(n, dec, n, NULL, spec, boxes, NULL, got, arr[0], arr[1], arr[2], arr[3])
                         : h264bsdmiOutputCellMaps(n, dec, n, NULL, spec, NULL, got, arr[0], arr[1], arr[2], arr[3]);
    print_head(name, rc);
    show("got", got, n, 1); show("current", arr[0], n, 1); show("kept", arr[1], n, 1); show("picId", arr[2], n, 1); show("keptPicId", arr[3], n, 1);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    Inst A, B, C, D, O, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    memset(&C, 0, sizeof(C));                   /* bound to the engine and nothing else: never fed, no sequence, no picture */
    C.s = h264bsdAlloc();
    if (h264bsdInit(C.s, 1) != HANTRO_OK) return 2;
    C.user = mock_last_attached();
    make(&D, 0, sa, len_a, 500);
    make(&O, 0, sa, len_a, 400);
    f_without = O.user;
    make(&G, 1, sa, len_a, 300);
    Inst *const abc[] = { &A, &B, &C }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const o[] = { &O }, *const ao[] = { &A, &O },
         *const a[] = { &A }, *const d[] = { &D };
    const h264bsdmi_blend_spec gated = { 3, 12, H264BSDMI_BLEND_FROZEN, (void *)(uintptr_t)0x3000 }, plain = { 4, 255, 4, NULL };
    const h264bsdmi_spread_spec all = { 2, 2, 255, H264BSDMI_SPREAD_ALL }, still = { 8, 0, 40, H264BSDMI_SPREAD_STILL };
    void *const bufs[3] = { (void *)(uintptr_t)0x10000, (void *)(uintptr_t)0x20000, (void *)(uintptr_t)0x30001 };     /* C's is never looked at */
    const h264bsdmi_cells_spec mode2 = { (void *)(uintptr_t)0x1000, 40, 23, 16, H264BSDMI_STATS_YCBCR, 1, H264BSDMI_CELLS_SPREAD,
                                         H264BSDMI_CELL_COUNT | H264BSDMI_CELL_FORE | H264BSDMI_CELL_EXCESS | H264BSDMI_CELL_SPREADSUM, { 6, 3, 2 }, 0 };
    const h264bsdmi_boxes_spec fore = { (void *)(uintptr_t)0x2000, 16, H264BSDMI_CELL_SPREADSUM, 2, H264BSDMI_BOXES_ABOVE, 5, 8, 1 };
    h264bsdmi_cells_spec bad_cells;
    pop("A", &A); pop("B", &B); pop("D", &D); pop("O", &O);

    /* refused: -1, nothing called, nothing written */
    blend("refused_spread_null", 3, abc, &gated, &all, 64);
    {
        static const char *const names[] = { "refused_gain_0", "refused_gain_9", "refused_lowest_above_highest", "refused_highest_256", "refused_lowest_256",
                                             "refused_update_3", "refused_gain_max" };
        const h264bsdmi_spread_spec bad[] = { { 0, 2, 255, 1 }, { 9, 2, 255, 1 }, { 2, 6, 5, 1 }, { 2, 0, 256, 1 }, { 2, 256, 256, 1 }, { 2, 2, 255, 3 },
                                              { 0xFFFFFFFFu, 2, 255, 1 } };
        for (int k = 0; k < 7; k++) blend(names[k], 3, abc, &gated, &bad[k], 0);
    }
    blend("refused_spec_null", 3, abc, &gated, &all, 2);
    {
        const h264bsdmi_blend_spec bad[] = { { 8, 0, 0, NULL }, { 0, 256, 0, NULL }, { 0, 0, 9, NULL } };
        static const char *const names[] = { "refused_shift_8", "refused_hold_256", "refused_moving_shift_9" };
        for (int k = 0; k < 3; k++) blend(names[k], 3, abc, &bad[k], &all, 0);
    }
    blend("refused_instances_null", 3, abc, &gated, &all, 4);
    blend("refused_kept_null", 3, abc, &gated, &all, 32);
    blend("refused_repeated", 2, aa, &gated, &all, 0);
    blend("refused_capture", 2, ag, &gated, &all, 0);
    blend("refused_sink_without_entry", 1, o, &gated, &all, 0);
    blend("refused_sink_without_entry_second", 2, ao, &gated, &all, 1);
    blend("nothing_to_do", 0, abc, &gated, &all, 0);

    /* nothing has a spread yet: nothing to hand out, nothing for mode 2 to read */
    spread_out("out_nothing_yet", 3, abc, bufs, 0);
    keep("keep_ab_first", 2, abc, 0, 0);
    cells("cells_kept_but_no_spread", 3, abc, &mode2, NULL);

    /* the first spread blend after a plain keep: a kept picture, no valid spread; a failing entry marks nothing */
    next_picture(&A);
    blend("first_fails", 3, abc, &gated, &all, 16);
    spread_out("out_after_a_failed_blend", 3, abc, bufs, 0);
    blend("first", 3, abc, &gated, &all, 0);
    spread_out("out", 3, abc, bufs, 1);
    spread_out("out_fails", 3, abc, bufs, 16);
    next_picture(&A);
    blend("second", 3, abc, &plain, &still, 1);
    blend("model_starts", 1, d, &gated, &still, 0);                    /* D keeps nothing yet: no kept picture, no valid spread */
    spread_out("out_of_a_started_model", 1, d, bufs, 0);

    /* mode 2 names the instances that have a current picture, a kept picture and a valid spread */
    cells("cells_ab", 3, abc, &mode2, NULL);
    cells("boxes_ab", 3, abc, &mode2, &fore);

    /* a plain blend leaves the spread as it is; a plain keep invalidates it */
    next_picture(&A);
    blend("plain_blend", 1, a, &plain, NULL, 128);
    spread_out("out_after_a_plain_blend", 3, abc, bufs, 0);
    next_picture(&A);
    keep("keep_a", 1, a, 0, 0);
    spread_out("out_after_a_keep", 3, abc, bufs, 0);
    cells("cells_after_a_keep", 3, abc, &mode2, NULL);                 /* B alone */
    next_picture(&A);
    blend("after_a_keep", 3, abc, &gated, &all, 0);                    /* A: unset, not fresh */
    spread_out("out_again", 3, abc, bufs, 0);

    /* a keep_after of a sibling is a plain keep too */
    {
        storage_t *dec[1]; void *users[1];
        u32 got[1] = { SENT };
        const h264bsdmi_change_spec change = { (void *)(uintptr_t)0x1000, H264BSDMI_STATS_Y, 0, 1, { 0, 0, 0 }, 1 };
        begin(1, a, dec, users, 0);
        const int rc = h264bsdmiOutputRegionChange(1, dec, 1, NULL, &change, NULL, got, NULL, NULL, NULL, NULL);
        print_head("change_with_keep_after", rc);
        show("got", got, 1, 1);
    }
    spread_out("out_after_keep_after", 3, abc, bufs, 0);

    /* the refusals of mode 2 and of the readback */
    bad_cells = mode2; bad_cells.keep_after = 1;
    cells("cells_refused_keep_after", 3, abc, &bad_cells, NULL);
    cells("boxes_refused_keep_after", 3, abc, &bad_cells, &fore);
    bad_cells = mode2; bad_cells.source = H264BSDMI_STATS_RGB;
    cells("cells_refused_rgb", 3, abc, &bad_cells, NULL);
    bad_cells = mode2; bad_cells.planes = 16;
    cells("cells_refused_plane_16", 3, abc, &bad_cells, NULL);
    bad_cells = mode2; bad_cells.mode = 3;
    cells("cells_refused_mode_3", 3, abc, &bad_cells, NULL);
    cells("cells_refused_sink_without_entry", 2, ao, &mode2, NULL);
    cells("boxes_refused_sink_without_entry", 1, o, &mode2, &fore);
    {
        void *const unaligned[3] = { (void *)(uintptr_t)0x10000, (void *)(uintptr_t)0x20008, NULL }, *const no_buf[3] = { (void *)(uintptr_t)0x10000, NULL, NULL };
        spread_out("out_refused_unaligned", 3, abc, unaligned, 0);
        spread_out("out_refused_no_buffer", 3, abc, no_buf, 0);
        spread_out("out_refused_repeated", 2, aa, bufs, 0);
        spread_out("out_refused_capture", 2, ag, bufs, 0);
        spread_out("out_refused_sink_without_entry", 2, ao, bufs, 0);
    }

    Inst *all_of[] = { &A, &B, &C, &D, &O, &G };
    for (int i = 0; i < 6; i++) unmake(all_of[i]);
    free(sa); free(sb);
    return 0;
}
