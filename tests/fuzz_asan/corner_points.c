/* What the host path of the corner points (api.c: h264bsdmiOutputCornerPoints) hands to the engine and writes back, without a GPU:
 * bound to tests/fuzz_asan/mock_engine.c, whose entry records all it is given.  Drives a fixed sequence of named calls and
 * prints per call "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched"
 * when none of it was written, "null" when NULL was passed).  tests/test_corner_points_host.py builds it, plain and under sanitizers,
 * and checks every record.       usage: corner_points <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), B the 1920x1080 stream, each popped once; O as A on a sink without the
 * corner_points entry; G capture mode. */
#include "host_harness.h"

/* flags: 1 got, 2 current, 4 picId are NULL; 8 a stream is named; 16 dec is NULL */
static void corners(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_corners_spec *spec, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[2][4];
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 2; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    aim(n, inst, dec, users, fail);
    const int rc = h264bsdmiOutputCornerPoints(n, flags & 16 ? NULL : dec, nr, regs, spec, flags & 8 ? (void *)(uintptr_t)0x5000 : NULL,
                                               flags & 1 ? NULL : got, flags & 2 ? NULL : arr[0], flags & 4 ? NULL : arr[1]);
    head(name, rc);
    show("got", got, nr < 8 ? nr : 8, !(flags & 1));
    show("current", arr[0], n, !(flags & 2));
    show("picId", arr[1], n, !(flags & 4));
}

#define DATA ((void *)(uintptr_t)0x1000)
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    Inst A, B, O, G;
    make(&A, 0, sa, len_a, 100);
    make(&B, 0, sb, len_b, 200);
    mock_without = MOCK_CORNER_POINTS;
    make(&O, 0, sa, len_a, 400);
    mock_without = 0;
    make(&G, 1, sa, len_a, 300);
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const a[] = { &A }, *const o[] = { &O };
    /*                                    data  score block nms K  crop zero min_score */
    const h264bsdmi_corners_spec plain = { DATA, 0, 3, 3, 64, 1, 0, 0 }, frame = { DATA, 1, 5, 7, 256, 0, 0, 0x7FFFFFFFFFFFFFFFull };
    const h264bsdmi_corners_spec least = { (void *)(uintptr_t)0x2008, 0, 5, 1, 1, 1, 0, 0xFFFFFFFFFFFFFFFFull };      /* MIN_EIGEN: any u64 passes */
    const h264bsdmi_corners_spec no_data = { NULL, 0, 3, 3, 64, 1, 0, 0 }, odd = { (void *)(uintptr_t)0x1004, 0, 3, 3, 64, 1, 0, 0 };
    const h264bsdmi_corners_spec score2 = { DATA, 2, 3, 3, 64, 1, 0, 0 };
    const h264bsdmi_corners_spec block0 = { DATA, 0, 0, 3, 64, 1, 0, 0 }, block4 = { DATA, 0, 4, 3, 64, 1, 0, 0 }, block7 = { DATA, 0, 7, 3, 64, 1, 0, 0 };
    const h264bsdmi_corners_spec nms0 = { DATA, 0, 3, 0, 64, 1, 0, 0 }, nms8 = { DATA, 0, 3, 8, 64, 1, 0, 0 };
    const h264bsdmi_corners_spec k0 = { DATA, 0, 3, 3, 0, 1, 0, 0 }, k257 = { DATA, 0, 3, 3, 257, 1, 0, 0 };
    const h264bsdmi_corners_spec crop2 = { DATA, 0, 3, 3, 64, 2, 0, 0 }, zero1 = { DATA, 0, 3, 3, 64, 1, 1, 0 };
    const h264bsdmi_corners_spec harris63 = { DATA, 1, 3, 3, 64, 1, 0, 0x8000000000000000ull };
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, -10, 16384, 16384 }, { 0, 0, 0, 640, 360 } };
    const h264bsdmi_region empty_w[] = { { 0, 0, 0, 0, 16 } }, far[] = { { 0, 16385, 0, 16, 16 } }, huge[] = { { 0, 0, 0, 16385, 16 } }, nobody[] = { { 2, 0, 0, 16, 16 } };
    pop("A", &A); pop("B", &B); pop("O", &O);

    /* accepted: what the sink is handed, what comes back */
    corners("whole_windows", 2, ab, 2, NULL, &plain, 0, 0);
    corners("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);              /* crop = 0: 640 x 368 and 1920 x 1088; every field at its largest */
    corners("boxes_mixed_order", 2, ba, 4, boxes, &plain, 0, 8);       /* B first in the call; boxes name A as instance 1 */
    corners("least", 1, a, 1, NULL, &least, 0, 0);
    corners("null_arrays", 2, ab, 2, NULL, &plain, 0, 2 | 4);
    corners("no_regions", 2, ab, 0, boxes, &plain, 0, 1);              /* nRegions == 0: 0, nothing called, got may be NULL */
    corners("engine_fails", 2, ab, 2, NULL, &plain, MOCK_CORNER_POINTS, 0);            /* -2: nothing written */

    /* refused: -1, no sink, nothing written */
    corners("refused_spec_null", 2, ab, 2, NULL, NULL, 0, 0);
    corners("refused_data_null", 2, ab, 2, NULL, &no_data, 0, 0);
    corners("refused_alignment", 2, ab, 2, NULL, &odd, 0, 0);
    corners("refused_score", 2, ab, 2, NULL, &score2, 0, 0);
    corners("refused_block_0", 2, ab, 2, NULL, &block0, 0, 0);
    corners("refused_block_4", 2, ab, 2, NULL, &block4, 0, 0);
    corners("refused_block_7", 2, ab, 2, NULL, &block7, 0, 0);
    corners("refused_nms_0", 2, ab, 2, NULL, &nms0, 0, 0);
    corners("refused_nms_8", 2, ab, 2, NULL, &nms8, 0, 0);
    corners("refused_points_0", 2, ab, 2, NULL, &k0, 0, 0);
    corners("refused_points_257", 2, ab, 2, NULL, &k257, 0, 0);
    corners("refused_crop", 2, ab, 2, NULL, &crop2, 0, 0);
    corners("refused_zero", 2, ab, 2, NULL, &zero1, 0, 0);
    corners("refused_harris_min_score", 2, ab, 2, NULL, &harris63, 0, 0);
    /* ... and what the region statistics refuse */
    corners("refused_repeated", 2, aa, 2, NULL, &plain, 0, 0);
    corners("refused_capture", 2, ag, 2, NULL, &plain, 0, 0);
    corners("refused_got_null", 2, ab, 2, NULL, &plain, 0, 1);
    corners("refused_dec_null", 2, ab, 2, NULL, &plain, 0, 16);
    corners("refused_window_count", 2, ab, 1, NULL, &plain, 0, 0);     /* regions == NULL wants nRegions == n */
    corners("refused_empty_region", 1, a, 1, empty_w, &plain, 0, 0);
    corners("refused_far_region", 1, a, 1, far, &plain, 0, 0);
    corners("refused_huge_region", 1, a, 1, huge, &plain, 0, 0);
    corners("refused_instance", 2, ab, 1, nobody, &plain, 0, 0);
    corners("refused_sink_without_entry", 1, o, 1, NULL, &plain, 0, 0);

    /* A decodes on: no current picture, no sink; then the next picture */
    feed(&A);
    corners("a_not_current", 2, ab, 2, NULL, &plain, 0, 0);
    pop("A", &A);
    corners("a_next_picture", 1, a, 1, NULL, &plain, 0, 0);

    Inst *all[] = { &A, &B, &O, &G };
    for (int i = 0; i < 4; i++) unmake(all[i]);
    free(sa); free(sb);
    return 0;
}
