/* What the host path of the region shift (api.c: h264bsdmiOutputRegionShift) hands to the engine and writes back, without a GPU: bound
 * to tests/fuzz_asan/mock_engine.c, whose entries record all they are given.  Drives a fixed sequence of named calls and prints
 * per call "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when
 * none of it was written, "null" when NULL was passed).  tests/test_region_shift_host.py builds it, plain and under sanitizers, and
 * checks every record.       usage: region_shift <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), B the 1920x1080 stream, each popped once; O as A on a sink without the
 * region_shift entry; G capture mode. */
#include "host_harness.h"

/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named */
static void shift(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_shift_spec *spec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail);
    const int rc = h264bsdmiOutputRegionShift(n, dec, nr, regs, spec, flags & 32 ? (void *)(uintptr_t)0x5000 : NULL, flags & 1 ? NULL : got,
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
    Inst A, B, O, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    mock_without = MOCK_REGION_SHIFT;
    make(&O, 0, sa, len_a, 400);
    mock_without = 0;
    make(&G, 1, sa, len_a, 300);
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const a[] = { &A }, *const o[] = { &O };
    const h264bsdmi_shift_spec plain = { (void *)(uintptr_t)0x1000, 4, 1, 1, 0 }, frame = { (void *)(uintptr_t)0x1000, 0, 0, 0, 0 };
    const h264bsdmi_shift_spec chain = { (void *)(uintptr_t)0x2000, 16, 0, 1, 1 };
    const h264bsdmi_shift_spec wide = { (void *)(uintptr_t)0x1000, 17, 1, 1, 0 }, odd = { (void *)(uintptr_t)0x1004, 4, 1, 1, 0 };
    const h264bsdmi_shift_spec surf = { (void *)(uintptr_t)0x1000, 4, 2, 1, 0 }, crop = { (void *)(uintptr_t)0x1000, 4, 1, 2, 0 }, after = { (void *)(uintptr_t)0x1000, 4, 1, 1, 2 };
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, -10, 4096, 4096 }, { 0, 0, 0, 640, 360 } };
    const h264bsdmi_region side[] = { { 0, 0, 0, 4096, 4096 } }, too_wide[] = { { 0, 0, 0, 4097, 16 } }, too_tall[] = { { 0, 0, 0, 16, 4097 } };
    pop("A", &A); pop("B", &B); pop("O", &O);

    /* nobody has kept anything: the search finds no pair and calls no sink */
    shift("nothing_kept", 2, ab, 2, NULL, &plain, 0, 0);
    keep("keep_a_only", 1, a, 0, 0);
    shift("a_has_both", 2, ab, 2, NULL, &plain, 0, 0);           /* B: current, nothing kept -> got 1,0 */
    shift("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);          /* crop = 0: 640 x 368; radius 0 */
    shift("boxes_mixed_order", 2, ba, 4, boxes, &plain, 0, 32);  /* B first in the call; boxes name A as instance 1 */
    shift("side_4096", 1, a, 1, side, &plain, 0, 0);             /* the largest side passes */
    shift("null_arrays", 2, ab, 2, NULL, &plain, 0, 2 | 4 | 8 | 16);
    shift("shift_fails", 2, ab, 2, NULL, &chain, MOCK_REGION_SHIFT, 0);           /* -2: nothing written, and keep_after marked nothing */
    shift("keep_after_fails", 2, ab, 2, NULL, &chain, MOCK_KEEP_PICTURES, 0);     /* the search went, the keep behind it failed: -2 all the same */
    shift("b_still_not_kept", 2, ab, 2, NULL, &plain, 0, 0);
    shift("keep_after", 2, ab, 2, NULL, &chain, 0, 0);           /* reports what the search saw (1,0), then keeps A and B */
    shift("both_kept", 2, ab, 2, NULL, &plain, 0, 0);

    /* refused: -1, no sink, nothing written */
    shift("refused_radius", 2, ab, 2, NULL, &wide, 0, 0);
    shift("refused_surface", 2, ab, 2, NULL, &surf, 0, 0);
    shift("refused_crop", 2, ab, 2, NULL, &crop, 0, 0);
    shift("refused_keep_after", 2, ab, 2, NULL, &after, 0, 0);
    shift("refused_alignment", 2, ab, 2, NULL, &odd, 0, 0);
    shift("refused_width", 1, a, 1, too_wide, &plain, 0, 0);
    shift("refused_height", 1, a, 1, too_tall, &plain, 0, 0);
    shift("refused_repeated", 2, aa, 2, NULL, &plain, 0, 0);
    shift("refused_capture", 2, ag, 2, NULL, &plain, 0, 0);
    shift("refused_got_null", 2, ab, 2, NULL, &plain, 0, 1);
    keep("keep_other_sink", 1, o, 0, 0);                         /* a sink with the keep entry and without the shift entry */
    shift("refused_sink_without_entry", 1, o, 1, NULL, &plain, 0, 0);

    /* A decodes on: no current picture, the kept one stays; then the next picture against it */
    feed(&A);
    shift("a_not_current", 1, a, 1, NULL, &plain, 0, 0);
    pop("A", &A);
    shift("a_next_picture", 1, a, 1, NULL, &plain, 0, 0);        /* picId 101 against the kept 100 */

    Inst *all[] = { &A, &B, &O, &G };
    for (int i = 0; i < 4; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
