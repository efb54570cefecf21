/* What the host path of the cell shift (api.c: h264bsdmiOutputCellShift) hands to the engine and writes back, without a GPU: bound to
 * tests/fuzz_asan/mock_engine.c, whose entries record all they are given, and to the eng_sink_entries below, whose cell_shift records
 * in the same form: the entries behind the last member of JobSink are a per-sink table of the engine (engine.h), to which api.c refers
 * weakly, so the stand-in of the other drivers links without it and this program brings its own (cell_shift_absent.c is the program
 * without one); a sink is left without the entry by naming it in f_without.  Drives a fixed sequence of named calls and prints per call
 * "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when none of it
 * was written, "null" when NULL was passed).  tests/test_cell_shift_host.py builds it, plain and under sanitizers, and checks every
 * record.       usage: cell_shift <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), B the 1920x1080 stream, each popped once; O as A on a sink without the
 * cell_shift entry; N as A on a sink that cannot keep pictures; G capture mode. */
#include <stdarg.h>
#include "host_harness.h"
#include "engine.h"

#define FLOW_FAILS (1u << 31)                   /* in `fail`: the cell_shift entry returns -1 (after recording) */
static const void *f_without;                   /* JobSink.user of the sink that has no cell_shift entry */
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
/* the engine's entry, recording what mock_engine.c records of the sibling entries: the pictures (a sink named by its instance's place
 * in the call), the regions, the spec */
static int f_cell_shift(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const struct h264bsdmi_cell_shift_spec *s, void *stream)
{
    frec("flow m=%u k=%u stream=0x%llx\n", n, k, (unsigned long long)(uintptr_t)stream);
    for (uint32_t i = 0; i < n; i++) {
        int inst = -1;
        for (u32 j = 0; j < f_n; j++) if (f_users[j] == p[i].sink->user) inst = (int)j;
        frec(" pic %d slot=%u win=%u,%u,%u,%u mr=%u,%u\n", inst, p[i].slot, p[i].x0, p[i].y0, p[i].w, p[i].h, p[i].matrix, p[i].range);
    }
    for (uint32_t i = 0; i < k; i++) frec(" reg %u index=%u %d,%d,%u,%u\n", r[i].pic, r[i].index, r[i].x, r[i].y, r[i].w, r[i].h);
    frec(" spec 0x%llx grid=%ux%u cell=%u radius=%u planes=%u crop=%u keep_after=%u\n", (unsigned long long)(uintptr_t)s->data, s->rows, s->cols,
         s->cell, s->radius, s->planes, s->crop, s->keep_after);
    return f_fail ? -1 : 0;
}
const EngSinkEntries *eng_sink_entries(const JobSink *sink)
{
    static const EngSinkEntries with = { f_cell_shift }, without = { NULL };
    return sink->user == f_without ? &without : &with;
}

/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named; 64 the spec is NULL */
static void flow(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_cell_shift_spec *spec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail & ~FLOW_FAILS);
    f_fail = (fail & FLOW_FAILS) != 0; f_users = users; f_n = n; f_len = 0; f_rec[0] = 0;
    const int rc = h264bsdmiOutputCellShift(n, dec, nr, regs, flags & 64 ? NULL : spec, flags & 32 ? (void *)(uintptr_t)0x5000 : NULL, flags & 1 ? NULL : got,
                                            flags & 2 ? NULL : arr[0], flags & 4 ? NULL : arr[1], flags & 8 ? NULL : arr[2], flags & 16 ? NULL : arr[3]);
    printf("#%s\nrc=%d\n%s%s%s", name, rc, f_rec, mock_record(), *f_rec || *mock_record() ? "" : "sink: not called\n");      /* the search, then the keep behind it */
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
    /*                                         data                       cols rows cell radius planes crop keep_after */
    const h264bsdmi_cell_shift_spec plain = { (void *)(uintptr_t)0x1000, 40, 23, 16, 4, 14, 1, 0 };
    const h264bsdmi_cell_shift_spec frame = { (void *)(uintptr_t)0x1004, 10, 6, 64, 0, 63, 0, 0 };
    const h264bsdmi_cell_shift_spec chain = { (void *)(uintptr_t)0x2000, 80, 45, 8, 16, 32, 1, 1 };
    h264bsdmi_cell_shift_spec bad;
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, -10, 16384, 16384 }, { 0, 0, 0, 640, 360 } };
    pop("A", &A); pop("B", &B); pop("O", &O); pop("N", &N);

    /* nobody has kept anything: the search finds no pair and calls no sink */
    flow("nothing_kept", 2, ab, 2, NULL, &plain, 0, 0);
    keep("keep_a_only", 1, a, 0, 0);
    flow("a_has_both", 2, ab, 2, NULL, &plain, 0, 0);            /* B: current, nothing kept -> got 1,0 */
    flow("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);           /* crop = 0: 640 x 368; radius 0, cell 64, all planes */
    flow("boxes_mixed_order", 2, ba, 4, boxes, &plain, 0, 32);   /* B first in the call; boxes name A as instance 1; a side of 16384 passes */
    flow("null_arrays", 2, ab, 2, NULL, &plain, 0, 2 | 4 | 8 | 16);
    flow("no_regions", 2, ab, 0, boxes, &plain, 0, 1);           /* nRegions == 0: 0, nothing launched, got may be NULL */
    flow("flow_fails", 2, ab, 2, NULL, &chain, FLOW_FAILS, 0);                    /* -2: nothing written, and keep_after marked nothing */
    flow("keep_after_fails", 2, ab, 2, NULL, &chain, MOCK_KEEP_PICTURES, 0);      /* the search went, the keep behind it failed: -2 all the same */
    flow("b_still_not_kept", 2, ab, 2, NULL, &plain, 0, 0);
    flow("keep_after", 2, ab, 2, NULL, &chain, 0, 0);            /* reports what the search saw (1,0), then keeps A and B */
    flow("both_kept", 2, ab, 2, NULL, &plain, 0, 0);

    /* refused: -1, no sink, nothing written */
    flow("refused_spec_null", 2, ab, 2, NULL, &plain, 0, 64);
    bad = plain; bad.data = NULL;
    flow("refused_data_null", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.data = (void *)(uintptr_t)0x1002;
    flow("refused_alignment", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.cols = 0;
    flow("refused_cols_zero", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.cols = 4097;
    flow("refused_cols", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.rows = 0;
    flow("refused_rows_zero", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.rows = 4097;
    flow("refused_rows", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.cell = 4;
    flow("refused_cell_4", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.cell = 12;
    flow("refused_cell_12", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.cell = 128;
    flow("refused_cell_128", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.radius = 17;
    flow("refused_radius", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.planes = 0;
    flow("refused_planes_zero", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.planes = 64;
    flow("refused_planes", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.crop = 2;
    flow("refused_crop", 2, ab, 2, NULL, &bad, 0, 0);
    bad = plain; bad.keep_after = 2;
    flow("refused_keep_after", 2, ab, 2, NULL, &bad, 0, 0);
    flow("refused_repeated", 2, aa, 2, NULL, &plain, 0, 0);
    flow("refused_capture", 2, ag, 2, NULL, &plain, 0, 0);
    flow("refused_got_null", 2, ab, 2, NULL, &plain, 0, 1);
    flow("refused_regions_count", 2, ab, 3, NULL, &plain, 0, 0);             /* regions == NULL with nRegions != n */
    flow("refused_stream_and_bad_region", 2, ab, 1, (const h264bsdmi_region[]){ { 2, 0, 0, 8, 8 } }, &plain, 0, 32);
    keep("keep_other_sink", 1, o, 0, 0);                         /* a sink with the keep entry and without the cell_shift entry */
    flow("refused_sink_without_entry", 1, o, 1, NULL, &plain, 0, 0);
    flow("refused_sink_without_keep", 2, an, 2, NULL, &plain, 0, 0);

    /* A decodes on: no current picture, the kept one stays; then the next picture against it */
    feed(&A);
    flow("a_not_current", 1, a, 1, NULL, &plain, 0, 0);
    pop("A", &A);
    flow("a_next_picture", 1, a, 1, NULL, &plain, 0, 0);         /* picId 101 against the kept 100 */

    Inst *all[] = { &A, &B, &O, &N, &G };
    for (int i = 0; i < 5; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
