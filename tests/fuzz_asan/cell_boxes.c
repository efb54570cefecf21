/* What the host path of the cell boxes (api.c: h264bsdmiOutputCellBoxes) hands to the engine and writes back, without a GPU: bound to
 * tests/fuzz_asan/mock_engine.c, whose entries record all they are given.  Drives a fixed sequence of named calls and prints per
 * call "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when none
 * of it was written, "null" when NULL was passed); at the end what the output queues of B and of its untouched twin T give.
 * tests/test_cell_boxes_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: cell_boxes <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), popped once; B the 1920x1080 stream, fed to its first picture and popped
 * later; T as B, never named in a call; G capture mode; N as A, bound to a sink that cannot keep pictures; X as A, bound to a sink
 * that has cell_maps but no cell_boxes. */
#include "host_harness.h"

/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named; 64 the boxes spec is NULL; 128 the maps' entry
 * instead (h264bsdmiOutputCellMaps: boxes is not used) */
static void boxes(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_cells_spec *spec,
                  const h264bsdmi_boxes_spec *bspec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail);
    void *stream = flags & 32 ? (void *)(uintptr_t)0x5000 : NULL;
    u32 *a0 = flags & 2 ? NULL : arr[0], *a1 = flags & 4 ? NULL : arr[1], *a2 = flags & 8 ? NULL : arr[2], *a3 = flags & 16 ? NULL : arr[3];
    const int rc = flags & 128 ? h264bsdmiOutputCellMaps(n, dec, nr, regs, spec, stream, flags & 1 ? NULL : got, a0, a1, a2, a3)
                               : h264bsdmiOutputCellBoxes(n, dec, nr, regs, spec, flags & 64 ? NULL : bspec, stream, flags & 1 ? NULL : got, a0, a1, a2, a3);
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
    Inst A, B, T, G, N, X;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    make(&T, 0, sb, len_b, 200);
    make(&G, 1, sa, len_a, 300);
    mock_without = MOCK_KEEP_PICTURES;
    make(&N, 0, sa, len_a, 400);
    mock_without = MOCK_CELL_BOXES;
    make(&X, 0, sa, len_a, 500);
    mock_without = 0;
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const an[] = { &A, &N },
         *const ax[] = { &A, &X };
    /*                                  data                        cols rows cell source crop mode planes threshold keep_after */
    const h264bsdmi_cells_spec picture = { (void *)(uintptr_t)0x1000, 40, 23, 16, 1, 1, H264BSDMI_CELLS_PICTURE, 31, { 0, 0, 0 }, 0 };
    const h264bsdmi_cells_spec change = { (void *)(uintptr_t)0x1004, 120, 68, 16, 0, 1, H264BSDMI_CELLS_CHANGE, 35, { 3, 2, 1 }, 0 };
    const h264bsdmi_cells_spec chain = { (void *)(uintptr_t)0x2000, 6, 5, 4, 2, 1, H264BSDMI_CELLS_CHANGE, 63, { 0, 0, 255 }, 1 };
    const h264bsdmi_cells_spec cap = { (void *)(uintptr_t)0x1000, 128, 128, 4, 0, 1, H264BSDMI_CELLS_PICTURE, 16, { 0, 0, 0 }, 0 };
    /*                                 data                        max plane channel sense level connectivity min_cells */
    const h264bsdmi_boxes_spec above = { (void *)(uintptr_t)0x3000, 64, H264BSDMI_CELL_SAD, 0, H264BSDMI_BOXES_ABOVE, 700, 8, 2 };
    const h264bsdmi_boxes_spec below = { (void *)(uintptr_t)0x3004, 512, H264BSDMI_CELL_MAX, 2, H264BSDMI_BOXES_BELOW, 40, 4, 1 };
    const h264bsdmi_boxes_spec count = { (void *)(uintptr_t)0x3000, 1, H264BSDMI_CELL_COUNT, 0, H264BSDMI_BOXES_ABOVE, 0, 8, 1 };
    const h264bsdmi_boxes_spec peak = { (void *)(uintptr_t)0x3000, 7, H264BSDMI_CELL_MAX, 0, H264BSDMI_BOXES_ABOVE, 0, 8, 1 };
    h264bsdmi_cells_spec bad;
    h264bsdmi_boxes_spec badb;
    const h264bsdmi_region regs[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, 10, 8, 8 }, { 0, 0, 0, 640, 360 } };
    pop_sized("A", &A); pop_sized("N", &N); pop_sized("X", &X);

    /* PICTURE needs no kept picture: A has a current one, B none yet */
    boxes("picture_a_only", 2, ab, 2, NULL, &picture, &below, 0, 0);
    /* CHANGE: nobody has kept anything: no pair, no sink */
    boxes("nothing_kept", 2, ab, 2, NULL, &change, &above, 0, 0);
    keep("keep_a_only", 2, ab, 0, 0);
    pop_sized("B", &B); pop_sized("T", &T);
    boxes("a_has_both", 2, ab, 2, NULL, &change, &above, 0, 0);           /* B: current, nothing kept -> got 1,0 */
    boxes("picture_both", 2, ab, 2, NULL, &picture, &below, 0, 0);
    boxes("count_plane", 2, ab, 2, NULL, &picture, &count, 0, 0);
    boxes("at_the_cap", 2, ab, 2, NULL, &cap, &peak, 0, 0);               /* 128 x 128 cells */
    boxes("boxes_mixed_order", 2, ba, 4, regs, &change, &above, 0, 32);   /* B first in the call; regions name A as instance 1 */
    boxes("picture_boxes", 2, ba, 4, regs, &picture, &below, 0, 32);
    boxes("null_arrays", 2, ab, 2, NULL, &change, &above, 0, 2 | 4 | 8 | 16);
    boxes("no_regions", 2, ab, 0, regs, &change, &above, 0, 1);           /* nRegions == 0: 0, nothing launched, got may be NULL */
    boxes("boxes_fail", 2, ab, 2, NULL, &chain, &above, MOCK_CELL_BOXES, 0);            /* -2: nothing written, and keep_after marked nothing */
    boxes("picture_fails", 2, ab, 2, NULL, &picture, &below, MOCK_CELL_BOXES, 0);
    boxes("keep_after_fails", 2, ab, 2, NULL, &chain, &above, MOCK_KEEP_PICTURES, 0);   /* the boxes went, the keep behind them failed: -2 all the same */
    boxes("b_still_not_kept", 2, ab, 2, NULL, &change, &above, 0, 0);
    boxes("keep_after", 2, ab, 2, NULL, &chain, &above, 0, 0);            /* reports what the comparison saw (1,0), then keeps A and B */
    boxes("both_kept", 2, ab, 2, NULL, &change, &above, 0, 0);
    boxes("maps_entry_still_calls_cell_maps", 2, ab, 2, NULL, &change, NULL, 0, 128);

    /* refused: -1, no sink, nothing written */
    boxes("refused_repeated", 2, aa, 2, NULL, &change, &above, 0, 0);
    boxes("refused_capture", 2, ag, 2, NULL, &picture, &below, 0, 0);
    boxes("refused_got_null", 2, ab, 2, NULL, &change, &above, 0, 1);
    boxes("refused_boxes_null", 2, ab, 2, NULL, &change, &above, 0, 64);
    bad = change; bad.threshold[1] = 256;
    boxes("refused_cells_threshold", 2, ab, 2, NULL, &bad, &above, 0, 0);
    bad = cap; bad.cols = 129;
    boxes("refused_above_the_cap", 2, ab, 2, NULL, &bad, &peak, 0, 0);
    badb = above; badb.data = NULL;
    boxes("refused_data_null", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.data = (void *)(uintptr_t)0x3002;
    boxes("refused_data_misaligned", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.max_boxes = 513;
    boxes("refused_max_boxes", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.max_boxes = 0;
    boxes("refused_no_boxes", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.plane = H264BSDMI_CELL_SSD;                          /* not in planes = 35 */
    boxes("refused_plane_not_asked", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.plane = H264BSDMI_CELL_SAD | H264BSDMI_CELL_COUNT;
    boxes("refused_two_planes", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.plane = H264BSDMI_CELL_DSUM;
    boxes("refused_dsum", 2, ab, 2, NULL, &chain, &badb, 0, 0);
    badb = above; badb.channel = 1;                                        /* change is luma only */
    boxes("refused_channel", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.sense = 2;
    boxes("refused_sense", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.connectivity = 6;
    boxes("refused_connectivity", 2, ab, 2, NULL, &change, &badb, 0, 0);
    badb = above; badb.min_cells = 0;
    boxes("refused_min_cells", 2, ab, 2, NULL, &change, &badb, 0, 0);
    /* a sink that cannot keep pictures serves PICTURE and refuses CHANGE; one without cell_boxes is refused, but serves the maps */
    boxes("no_keep_picture", 2, an, 2, NULL, &picture, &below, 0, 0);
    boxes("refused_no_keep_change", 2, an, 2, NULL, &change, &above, 0, 0);
    boxes("refused_sink_without_boxes", 2, ax, 2, NULL, &picture, &below, 0, 0);
    boxes("sink_without_boxes_serves_maps", 2, ax, 2, NULL, &picture, NULL, 0, 128);

    /* A decodes on: no current picture, the kept one stays */
    feed(&A);
    boxes("a_not_current", 1, ab, 1, NULL, &change, &above, 0, 0);
    pop_sized("A", &A);
    boxes("a_next_picture", 1, ab, 1, NULL, &change, &above, 0, 0);       /* picId 101 against the kept 100 */

    printf("#final\n");
    u32 idb = SENT, idt = SENT;
    const int slot_b = h264bsdmiNextOutputInfo(B.s, &idb, NULL, NULL), slot_t = h264bsdmiNextOutputInfo(T.s, &idt, NULL, NULL);
    printf("B next=%d,%u\nT next=%d,%u\ntwin=%d\n", slot_b, idb, slot_t, idt, slot_b == slot_t && idb == idt);
    Inst *all[] = { &A, &B, &T, &G, &N, &X };
    for (int i = 0; i < 6; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
