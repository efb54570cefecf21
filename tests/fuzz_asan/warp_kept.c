/* What the host path of the warped kept pictures (api.c: h264bsdmiWarpKeptPictures) hands to the engine, without a GPU: bound to
 * tests/fuzz_asan/mock_engine.c and to the eng_sink_entries below, a table with all FOUR entries behind the last member of JobSink
 * (engine.h), whose warp_kept records what it is given (the three older entries only say that they were called: nothing here may reach
 * them).  A sink is left without the warp_kept entry by naming it in f_without — its table has the first three members only, as a table
 * written before this entry has — and without any table by naming it in f_tableless.  Drives a fixed sequence of named calls and prints
 * per call "#name", rc, the entry's record and the sink's, or "sink: not called", then the output arrays, which start as a sentinel.
 * tests/test_warp_kept_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: warp_kept <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A (640x360 in a coded 640x368, picIds from 100) and B (1920x1080 in 1920x1088, from 200) fed and popped; C never fed
 * anything; O on a sink whose table lacks the entry; X on a sink without a table; G capture mode. */
#include <limits.h>
#include <stdarg.h>
#include "host_harness.h"
#include "engine.h"

static const void *f_without, *f_tableless;     /* JobSink.user of the sinks named above */
static char f_rec[4096];
static size_t f_len;
static int f_fail;
static void *const *f_users;
static u32 f_n;
static const h264bsdmi_warp_spec *f_spec;       /* the caller's */
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
/* the engine's entry: the pictures (each sink named by its instance's place in the call) with their maps, the spec and the stream */
static int f_warp_kept(uint32_t n, const SinkTensorPic *p, const struct h264bsdmi_warp_map *m, const struct h264bsdmi_warp_spec *s, uint32_t n_count,
                       void *stream)
{
    frec("warp m=%u n_count=%u stream=0x%llx\n", n, n_count, (unsigned long long)(uintptr_t)stream);
    for (uint32_t i = 0; i < n; i++) {
        int inst = -1;
        for (u32 j = 0; j < f_n; j++) if (f_users[j] == p[i].sink->user) inst = (int)j;
        frec(" pic %d slot=%u index=%u win=%u,%u,%u,%u map=%d,%d,%d,%d,%d,%d\n", inst, p[i].slot, p[i].index, p[i].x0, p[i].y0, p[i].w, p[i].h,
             m[i].a, m[i].b, m[i].c, m[i].d, m[i].e, m[i].f);
    }
    frec(" spec %s outside=%u crop=%u count=0x%llx\n", s == f_spec ? "the caller's" : "another", s->outside, s->crop, (unsigned long long)(uintptr_t)s->count);
    return f_fail ? -1 : 0;
}
const EngSinkEntries *eng_sink_entries(const JobSink *sink)
{
    static const EngSinkEntries with = { f_cell_shift, f_point_matches, f_point_model, f_warp_kept },
                                without = { f_cell_shift, f_point_matches, f_point_model };
    if (sink->user == f_tableless) return NULL;
    return sink->user == f_without ? &without : &with;
}

/* flags: 1 a stream is named; 2 the spec is NULL; 4 the instance array is NULL; 8 instance 0 is NULL; 16 the entry fails; 32 warped is
 * NULL; 64 keptPicId is NULL */
static void warp(const char *name, u32 n, Inst *const *inst, const h264bsdmi_warp_spec *spec, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 warped[4] = { SENT, SENT, SENT, SENT }, ids[4] = { SENT, SENT, SENT, SENT };
    aim(n, inst, dec, users, 0);
    if (flags & 8) dec[0] = NULL;
    f_fail = (flags & 16) != 0; f_users = users; f_n = n; f_len = 0; f_rec[0] = 0; f_spec = spec;
    const int rc = h264bsdmiWarpKeptPictures(n, flags & 4 ? NULL : dec, flags & 2 ? NULL : spec, flags & 1 ? (void *)(uintptr_t)0x5000 : NULL,
                                             flags & 32 ? NULL : warped, flags & 64 ? NULL : ids);
    printf("#%s\nrc=%d\n%s%s%s", name, rc, f_rec, mock_record(), *f_rec || *mock_record() ? "" : "sink: not called\n");
    show("warped", warped, n, !(flags & 32));
    show("keptPicId", ids, n, !(flags & 64));
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    Inst A, B, C, O, X, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    memset(&C, 0, sizeof(C));                   /* bound to the engine and nothing else: never fed, no sequence, no picture */
    C.s = h264bsdAlloc();
    if (h264bsdInit(C.s, 1) != HANTRO_OK) return 2;
    C.user = mock_last_attached();
    make(&O, 0, sa, len_a, 400);
    f_without = O.user;
    make(&X, 0, sa, len_a, 500);
    f_tableless = X.user;
    make(&G, 1, sa, len_a, 300);
    Inst *const abc[] = { &A, &B, &C }, *const cba[] = { &C, &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const ga[] = { &G, &A },
         *const o[] = { &O }, *const ao[] = { &A, &O }, *const x[] = { &X }, *const ax[] = { &A, &X }, *const ab[] = { &A, &B };
    const int top = H264BSDMI_WARP_MAX_COEFFICIENT;
    const h264bsdmi_warp_map maps[3] = { { 65536, 0, 5 << 16, 0, 65536, -(3 << 16) }, { top, -top, INT_MAX, -top, top, INT_MIN }, { 1, 2, 3, 4, 5, 6 } };
    const h264bsdmi_warp_spec plain = { maps, H264BSDMI_WARP_REPLICATE, 0, NULL }, cropped = { maps, H264BSDMI_WARP_CURRENT, 1, (void *)(uintptr_t)0x3000 };
    h264bsdmi_warp_spec bad;
    h264bsdmi_warp_map wrong[3];
    pop("A", &A); pop("B", &B);

    /* nothing is kept yet: nothing to warp, the entry is not called */
    warp("nothing_kept", 3, abc, &plain, 0);
    warp("nothing_to_do", 0, abc, &plain, 0);
    keep("keep_ab", 2, ab, 0, 0);

    /* accepted: a picture per instance with a kept picture, its window, its map beside it; the caller's spec and stream */
    warp("replicate_coded_frame", 3, abc, &plain, 0);
    warp("current_cropped_with_stream", 3, abc, &cropped, 1);
    warp("other_order", 3, cba, &plain, 1);                        /* C has none: B and A, with maps 1 and 2 */
    warp("optional_kept_pic_id", 2, ab, &plain, 64);
    warp("entry_fails", 3, abc, &cropped, 16);                     /* -2, nothing is written */
    warp("entry_fails_with_stream", 2, ab, &plain, 16 | 1);

    /* A decodes on and shows nothing: it has a kept picture and no current one */
    feed(&A);
    warp("replicate_without_a_current_picture", 3, abc, &plain, 0);
    warp("current_without_a_current_picture", 3, abc, &cropped, 0);      /* B alone */
    take(&A);
    warp("current_again", 3, abc, &cropped, 0);                    /* the kept picId is still the kept picture's */

    /* refused: -1, nothing called, nothing written */
    warp("refused_spec_null", 3, abc, &plain, 2);
    bad = plain; bad.maps = NULL;
    warp("refused_maps_null", 3, abc, &bad, 0);
    bad = plain; bad.outside = 2;
    warp("refused_outside", 3, abc, &bad, 0);
    bad = plain; bad.crop = 2;
    warp("refused_crop", 3, abc, &bad, 0);
    for (int k = 0; k < 8; k++) {
        static const char *const names[] = { "refused_a_high", "refused_a_low", "refused_b_high", "refused_b_low", "refused_d_high", "refused_d_low",
                                             "refused_e_high", "refused_e_low" };
        memcpy(wrong, maps, sizeof(wrong));
        int *const field[4] = { &wrong[2].a, &wrong[2].b, &wrong[2].d, &wrong[2].e };      /* the map of C, which has no kept picture: refused all the same */
        *field[k >> 1] = k & 1 ? -top - 1 : top + 1;
        bad = plain; bad.maps = wrong;
        warp(names[k], 3, abc, &bad, 0);
    }
    warp("refused_instances_null", 3, abc, &plain, 4);
    warp("refused_instance_null", 3, abc, &plain, 8);
    warp("refused_warped_null", 3, abc, &plain, 32);
    warp("refused_repeated", 2, aa, &plain, 0);
    warp("refused_capture", 2, ag, &plain, 0);
    warp("refused_capture_first", 2, ga, &plain, 1);
    warp("refused_sink_without_entry", 1, o, &plain, 0);
    warp("refused_sink_without_entry_second", 2, ao, &plain, 0);
    warp("refused_sink_without_table", 1, x, &plain, 0);
    warp("refused_sink_without_table_second", 2, ax, &plain, 1);

    Inst *all[] = { &A, &B, &C, &O, &X, &G };
    for (int i = 0; i < 6; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
