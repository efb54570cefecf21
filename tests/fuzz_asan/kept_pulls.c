/* The ONE host path of the four pulls that may compare against kept pictures and may keep afterwards (api.c: kept_pull), driven through
 * each of its entries — h264bsdmiOutputRegionChange, h264bsdmiOutputRegionShift, h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes
 * (both in CHANGE mode) — with the same scenarios, without a GPU: bound to tests/fuzz_asan/mock_engine.c, whose entries record what
 * they are given in the order they are called.  Prints per call "#<entry>_<scenario>", rc, the sink's record or "sink: not called",
 * and the output arrays, which start as a sentinel ("untouched" when none of it was written).  tests/test_kept_pulls_host.py builds
 * it, plain and under sanitizers, and holds the header lines of the four entries' records to one sequence.
 *       usage: kept_pulls <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream, B the 1920x1080 stream, each popped once; per entry A keeps its picture first, B has kept nothing. */
#include "host_harness.h"

enum { CHANGE, SHIFT, CELLS, BOXES, ENTRIES };
static const char *const ENTRY[ENTRIES] = { "change", "shift", "cells", "boxes" };
static const unsigned ENTRY_BIT[ENTRIES] = { MOCK_REGION_CHANGE, MOCK_REGION_SHIFT, MOCK_CELL_MAPS, MOCK_CELL_BOXES };

/* one call of `entry` over A and B, one whole window each; keep_after as given; fail: the entries that do */
static void pull(int entry, const char *scenario, Inst *const *ab, u32 keep_after, unsigned fail)
{
    const h264bsdmi_change_spec change = { (void *)(uintptr_t)0x1000, H264BSDMI_STATS_Y, 0, 1, { 0, 0, 0 }, keep_after };
    const h264bsdmi_shift_spec shift = { (void *)(uintptr_t)0x1000, 4, 0, 1, keep_after };
    const h264bsdmi_cells_spec cells = { (void *)(uintptr_t)0x1000, 120, 68, 16, H264BSDMI_STATS_Y, 1, H264BSDMI_CELLS_CHANGE, H264BSDMI_CELL_SAD,
                                         { 0, 0, 0 }, keep_after };
    const h264bsdmi_boxes_spec boxes = { (void *)(uintptr_t)0x2000, 8, H264BSDMI_CELL_SAD, 0, H264BSDMI_BOXES_ABOVE, 0, 8, 1 };
    storage_t *dec[2]; void *users[2];
    u32 got[2] = { SENT, SENT }, arr[4][2];
    int rc = -3;
    for (int k = 0; k < 4; k++) arr[k][0] = arr[k][1] = SENT;
    aim(2, ab, dec, users, fail);
    switch (entry) {
    case CHANGE: rc = h264bsdmiOutputRegionChange(2, dec, 2, NULL, &change, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    case SHIFT:  rc = h264bsdmiOutputRegionShift(2, dec, 2, NULL, &shift, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    case CELLS:  rc = h264bsdmiOutputCellMaps(2, dec, 2, NULL, &cells, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    case BOXES:  rc = h264bsdmiOutputCellBoxes(2, dec, 2, NULL, &cells, &boxes, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    }
    char name[64];
    snprintf(name, sizeof(name), "%s_%s", ENTRY[entry], scenario);
    head(name, rc);
    show("got", got, 2, 1);
    show("current", arr[0], 2, 1);
    show("kept", arr[1], 2, 1);
    show("picId", arr[2], 2, 1);
    show("keptPicId", arr[3], 2, 1);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    for (int entry = 0; entry < ENTRIES; entry++) {
        Inst A, B;
        make(&A, 0, sa, len_a, 100); take(&A);
        make(&B, 0, sb, len_b, 200); take(&B);
        Inst *const ab[2] = { &A, &B };
        const unsigned it = ENTRY_BIT[entry];
        storage_t *dec[1]; void *users[1];
        u32 kept[1];
        pull(entry, "nothing_kept", ab, 1, it | MOCK_KEEP_PICTURES);     /* no pair: no sink entry; keep_after keeps, and fails: -2 */
        pull(entry, "still_nothing_kept", ab, 0, 0);                     /* ... which marked nothing */
        aim(1, ab, dec, users, 0);
        if (h264bsdmiKeepCurrentPictures(1, dec, NULL, kept, NULL) != 0 || kept[0] != 1) return 3;      /* A keeps picture 100 */
        next_picture(&A);                                                /* A's current picture is 101 */
        pull(entry, "plain", ab, 0, 0);                                  /* the entry alone */
        pull(entry, "entry_fails", ab, 1, it);                           /* the entry, and nothing behind a failure */
        pull(entry, "keep_fails", ab, 1, MOCK_KEEP_PICTURES);            /* the entry, then the keep, which fails */
        pull(entry, "marked_nothing", ab, 0, 0);                         /* A still holds 100, B nothing */
        pull(entry, "keep_after", ab, 1, 0);                             /* the entry, then the keep: reports what the comparison saw */
        pull(entry, "both_kept", ab, 0, 0);                              /* A holds 101, B 200 */
        unmake(&A); unmake(&B);
    }
    free(sa); free(sb);
    return 0;
}
