/* What the host path of the point matches (api.c: h264bsdmiOutputPointMatches) hands to the engine and writes back, without a GPU: bound
 * to tests/fuzz_asan/mock_engine.c, whose entries record all they are given, and to the eng_sink_entries below, a table with BOTH
 * entries behind the last member of JobSink (engine.h), whose point_matches records in the same form (cell_shift only says that it was
 * called: nothing here may reach it); a sink is left without the point_matches entry by naming it in f_without — its table has the
 * first member only, as a table written before this entry has.  Drives a fixed sequence of named calls and prints per call "#name", rc,
 * the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when none of it was written,
 * "null" when NULL was passed).  tests/test_point_matches_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: point_matches <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), B the 1920x1080 stream, each popped once; O as A on a sink without the
 * point_matches entry; N as A on a sink that cannot keep pictures; G capture mode. */
#include <stdarg.h>
#include "host_harness.h"
#include "engine.h"

#define MATCH_FAILS (1u << 31)                  /* in `fail`: the point_matches entry returns -1 (after recording) */
static const void *f_without;                   /* JobSink.user of the sink that has no point_matches entry */
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
static int f_cell_shift(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const struct h264bsdmi_cell_shift_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    frec("flow m=%u k=%u\n", n, k);
    return -1;
}
/* the engine's entry, recording what mock_engine.c records of the sibling entries: the pictures (a sink named by its instance's place
 * in the call), the regions, the spec */
static int f_point_matches(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const struct h264bsdmi_matches_spec *s, void *stream)
{
    frec("matches m=%u k=%u stream=0x%llx\n", n, k, (unsigned long long)(uintptr_t)stream);
    for (uint32_t i = 0; i < n; i++) {
        int inst = -1;
        for (u32 j = 0; j < f_n; j++) if (f_users[j] == p[i].sink->user) inst = (int)j;
        frec(" pic %d slot=%u win=%u,%u,%u,%u mr=%u,%u\n", inst, p[i].slot, p[i].x0, p[i].y0, p[i].w, p[i].h, p[i].matrix, p[i].range);
    }
    for (uint32_t i = 0; i < k; i++) frec(" reg %u index=%u %d,%d,%u,%u\n", r[i].pic, r[i].index, r[i].x, r[i].y, r[i].w, r[i].h);
    frec(" spec 0x%llx kept=0x%llx current=0x%llx K=%u distance=%u ratio=%u move=%u mutual=%u crop=%u keep_after=%u zero=%u\n",
         (unsigned long long)(uintptr_t)s->data, (unsigned long long)(uintptr_t)s->kept_points, (unsigned long long)(uintptr_t)s->current_points,
         s->max_points, s->max_distance, s->ratio, s->max_move, s->mutual_only, s->crop, s->keep_after, s->zero);
    return f_fail ? -1 : 0;
}
const EngSinkEntries *eng_sink_entries(const JobSink *sink)
{
    static const EngSinkEntries with = { f_cell_shift, f_point_matches }, without = { f_cell_shift };
    return sink->user == f_without ? &without : &with;
}

/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named; 64 the spec is NULL */
static void match(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_matches_spec *spec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail & ~MATCH_FAILS);
    f_fail = (fail & MATCH_FAILS) != 0; f_users = users; f_n = n; f_len = 0; f_rec[0] = 0;
    const int rc = h264bsdmiOutputPointMatches(n, dec, nr, regs, flags & 64 ? NULL : spec, flags & 32 ? (void *)(uintptr_t)0x5000 : NULL, flags & 1 ? NULL : got,
                                               flags & 2 ? NULL : arr[0], flags & 4 ? NULL : arr[1], flags & 8 ? NULL : arr[2], flags & 16 ? NULL : arr[3]);
    printf("#%s\nrc=%d\n%s%s%s", name, rc, f_rec, mock_record(), *f_rec || *mock_record() ? "" : "sink: not called\n");      /* the matching, then the keep behind it */
    show("got", got, nr, !(flags & 1));
    show("current", arr[0], n, !(flags & 2));
    show("kept", arr[1], n, !(flags & 4));
    show("picId", arr[2], n, !(flags & 8));
    show("keptPicId", arr[3], n, !(flags & 16));
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    Inst A, B, O, N, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    make(&O, 0, sa, len_a, 400);
    f_without = O.user;
    mock_without = MOCK_KEEP_PICTURES;
    make(&N, 0, sa, len_a, 500);
    mock_without = 0;
    make(&G, 1, sa, len_a, 300);
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const a[] = { &A }, *const o[] = { &O },
         *const an[] = { &A, &N };
    /*                                      data                       kept_points                current_points        K  dist ratio move mutual crop keep_after zero */
    const h264bsdmi_matches_spec plain = { (void *)(uintptr_t)0x1000, (void *)(uintptr_t)0x2000, (void *)(uintptr_t)0x3000, 64, 64, 205, 0, 1, 1, 0, 0 };
    const h264bsdmi_matches_spec frame = { (void *)(uintptr_t)0x1008, (void *)(uintptr_t)0x2000, (void *)(uintptr_t)0x2000, 1, 0, 1, 1, 0, 0, 0, 0 };
    const h264bsdmi_matches_spec chain = { (void *)(uintptr_t)0x4000, (void *)(uintptr_t)0x2008, (void *)(uintptr_t)0x3008, 256, 256, 256, 65535, 0, 1, 1, 0 };
    h264bsdmi_matches_spec bad;
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, -10, 4096, 4096 }, { 0, 0, 0, 640, 360 } };
    pop("A", &A); pop("B", &B); pop("O", &O); pop("N", &N);

    /* nobody has kept anything: the matching finds no pair of pictures and calls no sink */
    match("nothing_kept", 2, ab, 2, NULL, &plain, 0, 0);
    keep("keep_a_only", 1, a, 0, 0);
    match("a_has_both", 2, ab, 2, NULL, &plain, 0, 0);            /* B: current, nothing kept -> got 1,0 */
    match("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);           /* crop = 0: 640 x 368; K = 1, the same records on both sides */
    match("boxes_mixed_order", 2, ba, 4, boxes, &plain, 0, 32);   /* B first in the call; boxes name A as instance 1; a side of 4096 passes */
    match("null_arrays", 2, ab, 2, NULL, &plain, 0, 2 | 4 | 8 | 16);
    match("no_regions", 2, ab, 0, boxes, &plain, 0, 1);           /* nRegions == 0: 0, nothing launched, got may be NULL */
    match("matches_fail", 2, ab, 2, NULL, &chain, MATCH_FAILS, 0);                 /* -2: nothing written, and keep_after marked nothing */
    match("keep_after_fails", 2, ab, 2, NULL, &chain, MOCK_KEEP_PICTURES, 0);      /* the matching went, the keep behind it failed: -2 all the same */
    match("b_still_not_kept", 2, ab, 2, NULL, &plain, 0, 0);
    match("keep_after", 2, ab, 2, NULL, &chain, 0, 0);            /* reports what the matching saw (1,0), then keeps A and B */
    match("both_kept", 2, ab, 2, NULL, &plain, 0, 0);

    /* refused: -1, no sink, nothing written */
    match("refused_spec_null", 2, ab, 2, NULL, &plain, 0, 64);
    bad = plain; bad.data = NULL;
    match("refused_data_null", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.data = (void *)(uintptr_t)0x1004;
    match("refused_data_alignment", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.kept_points = NULL;
    match("refused_kept_points_null", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.kept_points = (void *)(uintptr_t)0x2004;
    match("refused_kept_points_alignment", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.current_points = NULL;
    match("refused_current_points_null", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.current_points = (void *)(uintptr_t)0x3001;
    match("refused_current_points_alignment", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.max_points = 0;
    match("refused_points_zero", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.max_points = 257;
    match("refused_points", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.max_distance = 257;
    match("refused_distance", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.ratio = 0;
    match("refused_ratio_zero", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.ratio = 257;
    match("refused_ratio", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.max_move = 65536;
    match("refused_move", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.mutual_only = 2;
    match("refused_mutual", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.crop = 2;
    match("refused_crop", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.keep_after = 2;
    match("refused_keep_after", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.zero = 1;
    match("refused_zero", 2, ab, 2, NULL, &bad, 0, 0);
    match("refused_repeated", 2, aa, 2, NULL, &plain, 0, 0);
    match("refused_capture", 2, ag, 2, NULL, &plain, 0, 0);
    match("refused_got_null", 2, ab, 2, NULL, &plain, 0, 1);
    match("refused_regions_count", 2, ab, 3, NULL, &plain, 0, 0);             /* regions == NULL with nRegions != n */
    match("refused_side", 2, ab, 1, (const h264bsdmi_region[]){ { 1, 0, 0, 4097, 8 } }, &plain, 0, 0);      /* the region shift's limit */
    match("refused_stream_and_bad_region", 2, ab, 1, (const h264bsdmi_region[]){ { 2, 0, 0, 8, 8 } }, &plain, 0, 32);
    keep("keep_other_sink", 1, o, 0, 0);                          /* a sink with the keep entry and a table of the first member only */
    match("refused_sink_without_entry", 1, o, 1, NULL, &plain, 0, 0);
    match("refused_sink_without_keep", 2, an, 2, NULL, &plain, 0, 0);

    /* A decodes on: no current picture, the kept one stays; then the next picture against it */
    feed(&A);
    match("a_not_current", 1, a, 1, NULL, &plain, 0, 0);
    pop("A", &A);
    match("a_next_picture", 1, a, 1, NULL, &plain, 0, 0);         /* picId 101 against the kept 100 */

    Inst *all[] = { &A, &B, &O, &N, &G };
    for (int i = 0; i < 5; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
