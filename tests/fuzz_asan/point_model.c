/* What the host path of the point model (api.c: h264bsdmiOutputPointModel) hands to the engine, without a GPU: bound to
 * tests/fuzz_asan/mock_engine.c and to the eng_sink_entries below, a table with all THREE entries behind the last member of JobSink
 * (engine.h), whose point_model records what it is given (the two older entries only say that they were called: nothing here may reach
 * them).  A sink is left without the point_model entry by naming it in f_without — its table has the first two members only, as a table
 * written before this entry has — and without any table by naming it in f_tableless.  Drives a fixed sequence of named calls and prints
 * per call "#name", rc, and the entry's record or "sink: not called".  The call has no output arrays and writes nothing on the host.
 * tests/test_point_model_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: point_model <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A and B fed and popped; U never fed anything; O on a sink whose table lacks the entry; X on a sink without a table;
 * G capture mode. */
#include <stdarg.h>
#include "host_harness.h"
#include "engine.h"

static const void *f_without, *f_tableless;     /* JobSink.user of the sinks named above */
static char f_rec[2048];
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
static int f_point_matches(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const struct h264bsdmi_matches_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    frec("matches m=%u k=%u\n", n, k);
    return -1;
}
/* the engine's entry: the sink (named by its instance's place in the call), the count, the stream and the spec, verbatim */
static int f_point_model(const JobSink *sink, uint32_t n_records, const struct h264bsdmi_model_spec *s, void *stream)
{
    int inst = -1;
    for (u32 j = 0; j < f_n; j++) if (f_users[j] == sink->user) inst = (int)j;
    frec("model sink=%d records=%u stream=0x%llx\n", inst, n_records, (unsigned long long)(uintptr_t)stream);
    frec(" spec 0x%llx matches=0x%llx kept=0x%llx current=0x%llx K=%u model=%u tolerance=%u scale=%u inliers=%u zero=%u,%u,%u\n",
         (unsigned long long)(uintptr_t)s->data, (unsigned long long)(uintptr_t)s->matches, (unsigned long long)(uintptr_t)s->kept_points,
         (unsigned long long)(uintptr_t)s->current_points, s->max_points, s->model, s->tolerance, s->max_scale, s->min_inliers,
         s->zero[0], s->zero[1], s->zero[2]);
    return f_fail ? -1 : 0;
}
const EngSinkEntries *eng_sink_entries(const JobSink *sink)
{
    static const EngSinkEntries with = { f_cell_shift, f_point_matches, f_point_model }, without = { f_cell_shift, f_point_matches };
    if (sink->user == f_tableless) return NULL;
    return sink->user == f_without ? &without : &with;
}

/* flags: 1 a stream is named; 2 the spec is NULL; 4 the instance array is NULL; 8 instance 0 is NULL; 16 the entry fails */
static void model(const char *name, u32 n, Inst *const *inst, u32 records, const h264bsdmi_model_spec *spec, int flags)
{
    storage_t *dec[4]; void *users[4];
    aim(n, inst, dec, users, 0);
    if (flags & 8) dec[0] = NULL;
    f_fail = (flags & 16) != 0; f_users = users; f_n = n; f_len = 0; f_rec[0] = 0;
    const int rc = h264bsdmiOutputPointModel(n, flags & 4 ? NULL : dec, records, flags & 2 ? NULL : spec, flags & 1 ? (void *)(uintptr_t)0x5000 : NULL);
    printf("#%s\nrc=%d\n%s%s%s", name, rc, f_rec, mock_record(), *f_rec || *mock_record() ? "" : "sink: not called\n");
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    Inst A, B, U, O, X, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    memset(&U, 0, sizeof(U));                   /* bound to the engine and nothing else: never fed, no sequence, no picture */
    U.s = h264bsdAlloc();
    if (h264bsdInit(U.s, 1) != HANTRO_OK) return 2;
    U.user = mock_last_attached();
    make(&O, 0, sa, len_a, 400);
    f_without = O.user;
    make(&X, 0, sa, len_a, 500);
    f_tableless = X.user;
    make(&G, 1, sa, len_a, 300);
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const ga[] = { &G, &A },
         *const u[] = { &U }, *const o[] = { &O }, *const ao[] = { &A, &O }, *const x[] = { &X }, *const ax[] = { &A, &X }, *const uab[] = { &U, &A, &B };
    /*                                    data                       matches                    kept_points                current_points           K  model tol scale inliers zero */
    const h264bsdmi_model_spec plain = { (void *)(uintptr_t)0x1000, (void *)(uintptr_t)0x2000, (void *)(uintptr_t)0x3000, (void *)(uintptr_t)0x4000, 64, 1, 2, 0, 2, { 0, 0, 0 } };
    const h264bsdmi_model_spec shift = { (void *)(uintptr_t)0x1008, (void *)(uintptr_t)0x2008, (void *)(uintptr_t)0x3008, (void *)(uintptr_t)0x3008, 1, 0, 0, 0, 1, { 0, 0, 0 } };
    const h264bsdmi_model_spec gated = { (void *)(uintptr_t)0x6000, (void *)(uintptr_t)0x2000, (void *)(uintptr_t)0x3000, (void *)(uintptr_t)0x4000, 256, 1, 255, 4096, 256, { 0, 0, 0 } };
    const h264bsdmi_model_spec floor_ = { (void *)(uintptr_t)0x6000, (void *)(uintptr_t)0x2000, (void *)(uintptr_t)0x3000, (void *)(uintptr_t)0x4000, 256, 0, 255, 0, 256, { 0, 0, 0 } };
    h264bsdmi_model_spec bad;
    pop("A", &A); pop("B", &B);

    /* accepted: the entry gets the sink of instance 0, the count, the spec and the stream; no picture is needed */
    model("two_instances", 2, ab, 2, &plain, 0);
    model("other_order_and_stream", 2, ba, 300, &plain, 1);
    model("never_fed", 1, u, 65535, &shift, 0);
    model("never_fed_first_of_three", 3, uab, 1, &gated, 1);
    model("translation_limits", 2, ab, 7, &floor_, 0);
    bad = plain; bad.max_scale = 256;
    model("scale_floor", 2, ab, 1, &bad, 0);
    model("no_records", 2, ab, 0, &plain, 1);                      /* 0, the entry is not called */
    model("no_records_no_instances", 0, ab, 0, &plain, 0);
    model("entry_fails", 2, ab, 2, &plain, 16);                    /* -2 */
    model("entry_fails_with_stream", 1, u, 2, &gated, 16 | 1);

    /* refused: -1, no entry called */
    model("refused_spec_null", 2, ab, 2, &plain, 2);
    bad = plain; bad.data = NULL;
    model("refused_data_null", 2, ab, 2, &bad, 0);
    bad = plain; bad.data = (void *)(uintptr_t)0x1004;
    model("refused_data_alignment", 2, ab, 2, &bad, 0);
    bad = plain; bad.matches = NULL;
    model("refused_matches_null", 2, ab, 2, &bad, 0);
    bad = plain; bad.matches = (void *)(uintptr_t)0x2001;
    model("refused_matches_alignment", 2, ab, 2, &bad, 0);
    bad = plain; bad.kept_points = NULL;
    model("refused_kept_points_null", 2, ab, 2, &bad, 0);
    bad = plain; bad.kept_points = (void *)(uintptr_t)0x3004;
    model("refused_kept_points_alignment", 2, ab, 2, &bad, 0);
    bad = plain; bad.current_points = NULL;
    model("refused_current_points_null", 2, ab, 2, &bad, 0);
    bad = plain; bad.current_points = (void *)(uintptr_t)0x4002;
    model("refused_current_points_alignment", 2, ab, 2, &bad, 0);
    bad = plain; bad.max_points = 0;
    model("refused_points_zero", 2, ab, 2, &bad, 0);
    bad = plain; bad.max_points = 257;
    model("refused_points", 2, ab, 2, &bad, 0);
    bad = plain; bad.model = 2;
    model("refused_model", 2, ab, 2, &bad, 0);
    bad = plain; bad.tolerance = 256;
    model("refused_tolerance", 2, ab, 2, &bad, 0);
    bad = plain; bad.max_scale = 255;
    model("refused_scale_low", 2, ab, 2, &bad, 0);
    bad = plain; bad.max_scale = 4097;
    model("refused_scale_high", 2, ab, 2, &bad, 0);
    bad = shift; bad.max_scale = 256;
    model("refused_scale_for_translation", 2, ab, 2, &bad, 0);
    bad = shift; bad.min_inliers = 0;
    model("refused_inliers_zero", 2, ab, 2, &bad, 0);
    bad = plain; bad.min_inliers = 1;
    model("refused_inliers_one_for_similarity", 2, ab, 2, &bad, 0);
    bad = plain; bad.min_inliers = 257;
    model("refused_inliers", 2, ab, 2, &bad, 0);
    for (int k = 0; k < 3; k++) {
        static const char *const names[] = { "refused_zero_0", "refused_zero_1", "refused_zero_2" };
        bad = plain; bad.zero[k] = 1;
        model(names[k], 2, ab, 2, &bad, 0);
    }
    model("refused_no_instances", 0, ab, 2, &plain, 0);
    model("refused_instances_null", 2, ab, 2, &plain, 4);
    model("refused_instance_null", 2, ab, 2, &plain, 8);
    model("refused_repeated", 2, aa, 2, &plain, 0);
    model("refused_records", 2, ab, 65536, &plain, 0);
    model("refused_capture", 2, ag, 2, &plain, 0);
    model("refused_capture_first", 2, ga, 2, &plain, 1);
    model("refused_capture_no_records", 2, ag, 0, &plain, 0);
    model("refused_sink_without_entry", 1, o, 1, &plain, 0);
    model("refused_sink_without_entry_second", 2, ao, 1, &plain, 0);
    model("refused_sink_without_table", 1, x, 1, &plain, 0);
    model("refused_sink_without_table_second", 2, ax, 1, &plain, 1);

    Inst *all[] = { &A, &B, &U, &O, &X, &G };
    for (int i = 0; i < 6; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
