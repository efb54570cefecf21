/* What the host path of the cell maps (api.c: h264bsdmiOutputCellMaps) hands to the engine and writes back, without a GPU: bound to
 * tests/fuzz_asan/mock_engine.c, whose entries record all they are given.  Drives a fixed sequence of named calls and prints per
 * call "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when none
 * of it was written, "null" when NULL was passed); at the end what the output queues of B and of its untouched twin T give.
 * tests/test_cell_maps_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: cell_maps <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), popped once; B the 1920x1080 stream, fed to its first picture and popped
 * later; T as B, never named in a call; G capture mode; N as A, bound to a sink that cannot keep pictures. */
#include "host_harness.h"

/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named */
static void cells(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_cells_spec *spec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail);
    const int rc = h264bsdmiOutputCellMaps(n, dec, nr, regs, spec, flags & 32 ? (void *)(uintptr_t)0x5000 : NULL, flags & 1 ? NULL : got,
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
    Inst A, B, T, G, N;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    make(&T, 0, sb, len_b, 200);
    make(&G, 1, sa, len_a, 300);
    mock_without = MOCK_KEEP_PICTURES;
    make(&N, 0, sa, len_a, 400);
    mock_without = 0;
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const an[] = { &A, &N };
    /*                                  data                        cols rows cell source crop mode planes threshold keep_after */
    const h264bsdmi_cells_spec picture = { (void *)(uintptr_t)0x1000, 40, 23, 16, 1, 1, H264BSDMI_CELLS_PICTURE, 31, { 0, 0, 0 }, 0 };
    const h264bsdmi_cells_spec change = { (void *)(uintptr_t)0x1004, 120, 68, 8, 0, 1, H264BSDMI_CELLS_CHANGE, 35, { 3, 2, 1 }, 0 };
    const h264bsdmi_cells_spec frame = { (void *)(uintptr_t)0x1000, 1, 1, 64, 2, 0, H264BSDMI_CELLS_CHANGE, 1, { 0, 0, 0 }, 0 };
    const h264bsdmi_cells_spec chain = { (void *)(uintptr_t)0x2000, 6, 5, 4, 2, 1, H264BSDMI_CELLS_CHANGE, 63, { 0, 0, 255 }, 1 };
    h264bsdmi_cells_spec bad;
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, 10, 8, 8 }, { 0, 0, 0, 640, 360 } };
    pop_sized("A", &A); pop_sized("N", &N);

    /* PICTURE needs no kept picture: A has a current one, B none yet */
    cells("picture_a_only", 2, ab, 2, NULL, &picture, 0, 0);
    /* CHANGE: nobody has kept anything: no pair, no sink */
    cells("nothing_kept", 2, ab, 2, NULL, &change, 0, 0);
    keep("keep_a_only", 2, ab, 0, 0);
    pop_sized("B", &B); pop_sized("T", &T);
    cells("a_has_both", 2, ab, 2, NULL, &change, 0, 0);           /* B: current, nothing kept -> got 1,0 */
    cells("picture_both", 2, ab, 2, NULL, &picture, 0, 0);        /* PICTURE does not ask for a kept picture: got 1,1 */
    cells("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);           /* crop = 0: 640 x 368 */
    cells("boxes_mixed_order", 2, ba, 4, boxes, &change, 0, 32);  /* B first in the call; boxes name A as instance 1 */
    cells("picture_boxes", 2, ba, 4, boxes, &picture, 0, 32);     /* ... and PICTURE takes all four */
    cells("null_arrays", 2, ab, 2, NULL, &change, 0, 2 | 4 | 8 | 16);
    cells("no_regions", 2, ab, 0, boxes, &change, 0, 1);          /* nRegions == 0: 0, nothing launched, got may be NULL */
    cells("cells_fail", 2, ab, 2, NULL, &chain, MOCK_CELL_MAPS, 0);             /* -2: nothing written, and keep_after marked nothing */
    cells("picture_fails", 2, ab, 2, NULL, &picture, MOCK_CELL_MAPS, 0);
    cells("keep_after_fails", 2, ab, 2, NULL, &chain, MOCK_KEEP_PICTURES, 0);   /* the maps went, the keep behind them failed: -2 all the same */
    cells("b_still_not_kept", 2, ab, 2, NULL, &change, 0, 0);
    cells("keep_after", 2, ab, 2, NULL, &chain, 0, 0);            /* reports what the comparison saw (1,0), then keeps A and B */
    cells("both_kept", 2, ab, 2, NULL, &change, 0, 0);

    /* refused: -1, no sink, nothing written */
    cells("refused_repeated", 2, aa, 2, NULL, &change, 0, 0);
    cells("refused_capture", 2, ag, 2, NULL, &picture, 0, 0);
    cells("refused_got_null", 2, ab, 2, NULL, &change, 0, 1);
    bad = change; bad.threshold[1] = 256;
    cells("refused_threshold", 2, ab, 2, NULL, &bad, 0, 0);
    bad = change; bad.cell = 12;
    cells("refused_cell", 2, ab, 2, NULL, &bad, 0, 0);
    bad = change; bad.cols = 4097;
    cells("refused_grid", 2, ab, 2, NULL, &bad, 0, 0);
    bad = change; bad.planes = 64;
    cells("refused_planes", 2, ab, 2, NULL, &bad, 0, 0);
    bad = picture; bad.keep_after = 1;
    cells("refused_picture_keeps", 2, ab, 2, NULL, &bad, 0, 0);
    bad = picture; bad.planes = 32;
    cells("refused_picture_above", 2, ab, 2, NULL, &bad, 0, 0);
    /* a sink that cannot keep pictures serves PICTURE and refuses CHANGE */
    cells("no_keep_picture", 2, an, 2, NULL, &picture, 0, 0);
    cells("refused_no_keep_change", 2, an, 2, NULL, &change, 0, 0);

    /* A decodes on: no current picture, the kept one stays */
    feed(&A);
    cells("a_not_current", 1, ab, 1, NULL, &change, 0, 0);
    cells("a_not_current_picture", 1, ab, 1, NULL, &picture, 0, 0);
    pop_sized("A", &A);
    cells("a_next_picture", 1, ab, 1, NULL, &change, 0, 0);       /* picId 101 against the kept 100 */

    printf("#final\n");
    u32 idb = SENT, idt = SENT;
    const int slot_b = h264bsdmiNextOutputInfo(B.s, &idb, NULL, NULL), slot_t = h264bsdmiNextOutputInfo(T.s, &idt, NULL, NULL);
    printf("B next=%d,%u\nT next=%d,%u\ntwin=%d\n", slot_b, idb, slot_t, idt, slot_b == slot_t && idb == idt);
    Inst *all[] = { &A, &B, &T, &G, &N };
    for (int i = 0; i < 5; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
