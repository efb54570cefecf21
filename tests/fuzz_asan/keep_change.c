/* What the host path of kept pictures and change statistics (api.c: h264bsdmiKeepCurrentPictures, h264bsdmiOutputRegionChange) hands to
 * the engine and writes back, without a GPU: bound to tests/fuzz_asan/mock_engine.c, whose two entries record all they are given.
 * Drives a fixed sequence of named calls and prints per call "#name", rc, the sink's record or "sink: not called", and the output
 * arrays, which start as a sentinel ("untouched" when none of it was written, "null" when NULL was passed); at the end what the
 * output queues of B and of its untouched twin T give.  tests/test_keep_change_host.py builds it, plain and under sanitizers, and checks
 * every record.       usage: keep_change <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), popped once; B the 1920x1080 stream, fed to its first picture and popped
 * later; T as B, never named in a call; G capture mode. */
#include "host_harness.h"

/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named */
static void change(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_change_spec *spec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail);
    const int rc = h264bsdmiOutputRegionChange(n, dec, nr, regs, spec, flags & 32 ? (void *)(uintptr_t)0x5000 : NULL, flags & 1 ? NULL : got,
                                               flags & 2 ? NULL : arr[0], flags & 4 ? NULL : arr[1], flags & 8 ? NULL : arr[2], flags & 16 ? NULL : arr[3]);
    head(name, rc);
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
    Inst A, B, T, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    make(&T, 0, sb, len_b, 200);
    make(&G, 1, sa, len_a, 300);
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const a[] = { &A };
    const h264bsdmi_change_spec plain = { (void *)(uintptr_t)0x1000, 1, 256, 1, { 3, 2, 1 }, 0 }, frame = { (void *)(uintptr_t)0x1000, 0, 0, 0, { 0, 0, 0 }, 0 };
    const h264bsdmi_change_spec chain = { (void *)(uintptr_t)0x2000, 2, 16, 1, { 0, 0, 255 }, 1 }, high = { (void *)(uintptr_t)0x1000, 1, 256, 1, { 0, 256, 0 }, 0 };
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, 10, 8, 8 }, { 0, 0, 0, 640, 360 } };
    pop_sized("A", &A);

    /* nobody has kept anything: a comparison finds no pair and calls no sink; B has no current picture yet */
    change("nothing_kept", 2, ab, 2, NULL, &plain, 0, 0);
    keep("keep_fails", 2, ab, MOCK_KEEP_PICTURES, 0);             /* the sink fails: -2, nothing written, nothing marked */
    change("still_nothing_kept", 2, ab, 2, NULL, &plain, 0, 0);
    keep("keep_a_only", 2, ab, 0, 0);                             /* B has no current picture: kept = 1,0 */
    pop_sized("B", &B); pop_sized("T", &T);
    change("a_has_both", 2, ab, 2, NULL, &plain, 0, 0);           /* B: current, nothing kept -> got 1,0 */
    change("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);          /* crop = 0: 640 x 368 */
    change("boxes_mixed_order", 2, ba, 4, boxes, &plain, 0, 32);  /* B first in the call; boxes name A as instance 1 */
    change("null_arrays", 2, ab, 2, NULL, &plain, 0, 2 | 4 | 8 | 16);
    change("change_fails", 2, ab, 2, NULL, &chain, MOCK_REGION_CHANGE, 0);     /* -2: nothing written, and keep_after marked nothing */
    change("keep_after_fails", 2, ab, 2, NULL, &chain, MOCK_KEEP_PICTURES, 0); /* the comparison went, the keep behind it failed: -2 all the same */
    change("b_still_not_kept", 2, ab, 2, NULL, &plain, 0, 0);
    change("keep_after", 2, ab, 2, NULL, &chain, 0, 0);           /* reports what the comparison saw (1,0), then keeps A and B */
    change("both_kept", 2, ab, 2, NULL, &plain, 0, 0);
    keep("keep_null_ids", 2, ab, 0, 2);

    /* refused: -1, no sink, nothing written */
    change("refused_repeated", 2, aa, 2, NULL, &plain, 0, 0);
    change("refused_capture", 2, ag, 2, NULL, &plain, 0, 0);
    change("refused_threshold", 2, ab, 2, NULL, &high, 0, 0);
    change("refused_got_null", 2, ab, 2, NULL, &plain, 0, 1);
    keep("refused_keep_repeated", 2, aa, 0, 0);
    keep("refused_keep_capture", 2, ag, 0, 0);
    keep("refused_keep_null", 2, ab, 0, 1);

    /* A decodes on: no current picture, the kept one stays */
    feed(&A);
    change("a_not_current", 1, a, 1, NULL, &plain, 0, 0);
    keep("keep_without_current", 1, a, 0, 0);
    pop_sized("A", &A);
    change("a_next_picture", 1, a, 1, NULL, &plain, 0, 0);        /* picId 101 against the kept 100 */

    /* a sequence of another coded size between keep and compare: the kept picture is gone */
    give(&A, sb, len_b);
    feed(&A);
    pop_sized("A", &A);
    change("other_size", 1, a, 1, NULL, &plain, 0, 0);
    keep("keep_other_size", 1, a, 0, 0);
    change("other_size_kept", 1, a, 1, NULL, &plain, 0, 0);

    printf("#final\n");
    u32 idb = SENT, idt = SENT;
    const int slot_b = h264bsdmiNextOutputInfo(B.s, &idb, NULL, NULL), slot_t = h264bsdmiNextOutputInfo(T.s, &idt, NULL, NULL);
    printf("B next=%d,%u\nT next=%d,%u\ntwin=%d\n", slot_b, idb, slot_t, idt, slot_b == slot_t && idb == idt);
    Inst *all[] = { &A, &B, &T, &G };
    for (int i = 0; i < 4; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
