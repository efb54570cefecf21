/* The host path of the background model (api.c: h264bsdmiBlendCurrentPictures, h264bsdmiOutputKeptPictures) without a GPU: bound to
 * tests/fuzz_asan/mock_engine.c, whose entries record what they are handed.  Prints per call "#<name>", rc, the sink's record or
 * "sink: not called", and the output arrays, which start as a sentinel ("untouched" when none of it was written).
 * tests/test_background_host.py builds it, plain and under sanitizers, and reads the records.
 * usage: background <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (picIds from 100), B the 1920x1080 stream (from 200), each popped once; C initialised and never fed. */
#include "host_harness.h"

/* an instance over the bytes of one stream, or of two, one after the other; pictures: how many it decodes and pops at once */
static void make_joined(Inst *t, const u8 *a, u32 len_a, const u8 *b, u32 len_b, u32 id, int pictures)
{
    memset(t, 0, sizeof(*t));
    t->s = h264bsdAlloc();
    t->id = id;
    if (h264bsdInit(t->s, 1) != HANTRO_OK) exit(2);
    t->user = mock_last_attached();
    t->len = len_a + len_b;
    t->buf = malloc(t->len ? t->len : 1);
    if (len_a) memcpy(t->buf, a, len_a);
    if (len_b) memcpy(t->buf + len_a, b, len_b);
    for (int k = 0; k < pictures; k++) next_picture(t);
}

#define MAXN 4
/* one blend over t[0 .. n); spec NULL: the call gets none; dec_null / kept_null: those arguments NULL */
static void blend(const char *name, u32 n, Inst *const *t, const h264bsdmi_blend_spec *spec, void *stream, unsigned fail, int dec_null, int kept_null)
{
    storage_t *dec[MAXN]; void *users[MAXN];
    u32 kept[MAXN], blended[MAXN], ids[MAXN];
    for (u32 i = 0; i < n; i++) kept[i] = blended[i] = ids[i] = SENT;
    aim(n, t, dec, users, fail);
    const int rc = h264bsdmiBlendCurrentPictures(n, dec_null ? NULL : dec, spec, stream, kept_null ? NULL : kept, blended, ids);
    head(name, rc);
    show("kept", kept, n, 1); show("blended", blended, n, 1); show("picId", ids, n, 1);
}
static void kept_out(const char *name, u32 n, Inst *const *t, void *const *picture, void *const *fraction, void *stream, unsigned fail)
{
    storage_t *dec[MAXN]; void *users[MAXN];
    u32 got[MAXN], ids[MAXN];
    for (u32 i = 0; i < n; i++) got[i] = ids[i] = SENT;
    aim(n, t, dec, users, fail);
    const int rc = h264bsdmiOutputKeptPictures(n, dec, picture, fraction, stream, got, ids);
    head(name, rc);
    show("got", got, n, 1); show("keptPicId", ids, n, 1);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    Inst A, B, C, D, E;
    make_joined(&A, sa, len_a, NULL, 0, 100, 1);
    make_joined(&B, sb, len_b, NULL, 0, 200, 1);
    make_joined(&C, NULL, 0, NULL, 0, 300, 0);
    Inst *const abc[3] = { &A, &B, &C }, *const aa[2] = { &A, &A };
    const h264bsdmi_blend_spec plain = { 4, 255, 4, NULL }, gated = { 3, 12, H264BSDMI_BLEND_FROZEN, (void *)(uintptr_t)0x3000 };
    void *const stream = (void *)(uintptr_t)0x77;

    /* every refusal: nothing is called, nothing is written */
    blend("refused_no_spec", 3, abc, NULL, NULL, 0, 0, 0);
    const h264bsdmi_blend_spec bad[5] = { { 8, 0, 0, NULL }, { 0, 256, 0, NULL }, { 0, 0, 9, NULL }, { 0, 0, 0xFFFFFFFFu, NULL }, { 0xFFFFFFFFu, 0, 0, NULL } };
    const char *const bad_name[5] = { "refused_shift_8", "refused_hold_256", "refused_moving_shift_9", "refused_moving_shift_max", "refused_shift_max" };
    for (int k = 0; k < 5; k++) blend(bad_name[k], 3, abc, &bad[k], NULL, 0, 0, 0);
    blend("refused_no_instances", 3, abc, &plain, NULL, 0, 1, 0);
    blend("refused_no_kept_array", 3, abc, &plain, NULL, 0, 0, 1);
    blend("refused_repeated_instance", 2, aa, &plain, NULL, 0, 0, 0);
    {
        Inst cap;
        memset(&cap, 0, sizeof(cap));
        cap.s = h264bsdAlloc();
        if (h264bsdmiInitCapture(cap.s, 1, no_job, NULL) != HANTRO_OK) return 3;
        Inst *const ac[2] = { &A, &cap };
        void *const pic2[2] = { (void *)(uintptr_t)0x10000, (void *)(uintptr_t)0x20000 };
        blend("refused_capture_mode", 2, ac, &plain, NULL, 0, 0, 0);
        kept_out("kept_out_refused_capture_mode", 2, ac, pic2, NULL, NULL, 0);
        unmake(&cap);
    }
    blend("nothing_to_do", 0, abc, &plain, NULL, 0, 0, 0);

    /* the model starts, is blended into, and a failing sink marks nothing */
    void *const pics[3] = { (void *)(uintptr_t)0x10000, (void *)(uintptr_t)0x20000, (void *)(uintptr_t)0x30000 };
    void *const fracs[3] = { (void *)(uintptr_t)0x40000, NULL, (void *)(uintptr_t)0x50000 };
    kept_out("kept_out_nothing_kept", 3, abc, pics, fracs, NULL, 0);
    blend("first_fails", 3, abc, &plain, NULL, MOCK_BLEND_PICTURES, 0, 0);
    blend("first", 3, abc, &plain, NULL, 0, 0, 0);                 /* ... which marked nothing: both start now */
    next_picture(&A);
    blend("second", 3, abc, &gated, stream, 0, 0, 0);
    next_picture(&A);
    blend("third_fails", 3, abc, &gated, stream, MOCK_BLEND_PICTURES, 0, 0);
    kept_out("kept_out", 3, abc, pics, fracs, stream, 0);          /* A still holds 101 */
    kept_out("kept_out_no_fractions", 3, abc, pics, NULL, NULL, 0);
    kept_out("kept_out_fails", 3, abc, pics, fracs, NULL, MOCK_KEPT_PICTURES_OUT);
    {
        void *const unaligned[3] = { (void *)(uintptr_t)0x10008, (void *)(uintptr_t)0x20000, NULL };
        void *const no_pic[3] = { (void *)(uintptr_t)0x10000, NULL, NULL };
        void *const only_c_bad[3] = { (void *)(uintptr_t)0x10000, (void *)(uintptr_t)0x20000, (void *)(uintptr_t)0x30001 };
        kept_out("kept_out_refused_unaligned", 3, abc, unaligned, NULL, NULL, 0);
        kept_out("kept_out_refused_unaligned_fraction", 3, abc, pics, unaligned, NULL, 0);
        kept_out("kept_out_refused_no_buffer", 3, abc, no_pic, NULL, NULL, 0);
        kept_out("kept_out_ignores_buffers_of_instances_without", 3, abc, only_c_bad, NULL, NULL, 0);
        kept_out("kept_out_refused_repeated_instance", 2, aa, pics, NULL, NULL, 0);
    }

    /* a plain keep and a blend share what is known of the kept picture */
    {
        Inst *const a[1] = { &A };
        storage_t *dec[1]; void *users[1];
        u32 kept[1];
        aim(1, a, dec, users, 0);
        if (h264bsdmiKeepCurrentPictures(1, dec, NULL, kept, NULL) != 0 || kept[0] != 1) return 3;      /* A keeps 102 */
        next_picture(&A);
        blend("after_a_keep", 1, a, &plain, NULL, 0, 0, 0);
    }

    /* blended and picId may be NULL */
    {
        Inst *const b[1] = { &B };
        storage_t *dec[1]; void *users[1];
        u32 kept[1] = { SENT };
        aim(1, b, dec, users, 0);
        const int rc = h264bsdmiBlendCurrentPictures(1, dec, &plain, NULL, kept, NULL, NULL);
        head("optional_arrays", rc);
        show("kept", kept, 1, 1);
    }

    /* a sink without the new entries */
    mock_without = MOCK_BLEND_PICTURES | MOCK_KEPT_PICTURES_OUT;
    make_joined(&D, sa, len_a, NULL, 0, 400, 1);
    mock_without = 0;
    {
        Inst *const ad[2] = { &A, &D };
        blend("refused_sink_without_the_entry", 2, ad, &plain, NULL, 0, 0, 0);
        kept_out("kept_out_refused_sink_without_the_entry", 2, ad, pics, NULL, NULL, 0);
    }

    /* a kept picture of another coded size counts as none */
    make_joined(&E, sa, len_a, sb, len_b, 500, 1);
    {
        Inst *const e[1] = { &E };
        blend("size_a_first", 1, e, &plain, NULL, 0, 0, 0);
        next_picture(&E);
        blend("size_a_second", 1, e, &plain, NULL, 0, 0, 0);
        while (h264bsdPicWidth(E.s) == 40) next_picture(&E);
        kept_out("kept_out_of_another_size", 1, e, pics, NULL, NULL, 0);
        blend("size_b_first", 1, e, &plain, NULL, 0, 0, 0);
        next_picture(&E);
        blend("size_b_second", 1, e, &plain, NULL, 0, 0, 0);
    }
    unmake(&A); unmake(&B); unmake(&C); unmake(&D); unmake(&E);
    free(sa); free(sb);
    return 0;
}
