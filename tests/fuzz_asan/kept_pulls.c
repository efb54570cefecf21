/* The ONE host path of the four pulls that may compare against kept pictures and may keep afterwards (api.c: kept_pull), driven through
 * each of its entries — h264bsdmiOutputRegionChange, h264bsdmiOutputRegionShift, h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes
 * (both in CHANGE mode) — with the same scenarios, without a GPU: bound to tests/fuzz_asan/mock_engine_kept.c, whose entries record
 * their names in the order they are called.  Prints per call "#<entry>_<scenario>", rc, the sink's record or "sink: not called", and
 * the output arrays, which start as a sentinel ("untouched" when none of it was written).  tests/test_kept_pulls_host.py builds it,
 * plain and under sanitizers, and holds the four entries to one sequence.   usage: kept_pulls <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream, B the 1920x1080 stream, each popped once; per entry A keeps its picture first, B has kept nothing. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
void mock_call(void);
const char *mock_record(void);
extern int mock_fail;

#define SENT 0xA5A5A5A5u
typedef struct Inst { storage_t *s; u8 *buf; u32 len, off, id; } Inst;      /* id: the picId its next picture carries */

static u8 *load(const char *path, u32 *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    u8 *p = malloc((size_t)n);
    if (!p || fread(p, 1, (size_t)n, f) != (size_t)n) exit(2);
    fclose(f);
    *len = (u32)n;
    return p;
}
/* one more picture decoded, and popped: it is the current picture */
static void next_picture(Inst *t)
{
    int stalls = 0;
    while (t->off < t->len && stalls <= 3) {
        u32 rb = 0;
        const u32 r = h264bsdDecode(t->s, t->buf + t->off, t->len - t->off, t->id, &rb);
        t->off += rb;
        stalls = rb ? 0 : stalls + 1;
        if (r == H264BSD_PIC_RDY) {
            t->id++;
            if (h264bsdmiNextOutputInfo(t->s, NULL, NULL, NULL) < 0) break;
            return;
        }
    }
    fprintf(stderr, "stream ended before a picture\n"); exit(2);
}
static void make(Inst *t, const u8 *stream, u32 len, u32 id)
{
    memset(t, 0, sizeof(*t));
    t->s = h264bsdAlloc();
    t->id = id;
    if (h264bsdInit(t->s, 1) != HANTRO_OK) exit(2);
    t->buf = malloc(len); memcpy(t->buf, stream, len); t->len = len;
    next_picture(t);
}

static void show(const char *name, const u32 *a, size_t n)
{
    int touched = 0;
    for (size_t i = 0; i < n; i++) touched |= a[i] != SENT;
    printf("%s=", name);
    if (!touched) printf("untouched");
    else for (size_t i = 0; i < n; i++) { if (a[i] == SENT) printf("%sS", i ? "," : ""); else printf("%s%u", i ? "," : "", a[i]); }
    printf("\n");
}

enum { CHANGE, SHIFT, CELLS, BOXES, ENTRIES };
static const char *const ENTRY[ENTRIES] = { "change", "shift", "cells", "boxes" };

/* one call of `entry` over A and B, one whole window each; keep_after as given; fail: mock_fail */
static void pull(int entry, const char *scenario, storage_t *const *dec, u32 keep_after, int fail)
{
    const h264bsdmi_change_spec change = { (void *)(uintptr_t)0x1000, H264BSDMI_STATS_Y, 0, 1, { 0, 0, 0 }, keep_after };
    const h264bsdmi_shift_spec shift = { (void *)(uintptr_t)0x1000, 4, 0, 1, keep_after };
    const h264bsdmi_cells_spec cells = { (void *)(uintptr_t)0x1000, 120, 68, 16, H264BSDMI_STATS_Y, 1, H264BSDMI_CELLS_CHANGE, H264BSDMI_CELL_SAD,
                                         { 0, 0, 0 }, keep_after };
    const h264bsdmi_boxes_spec boxes = { (void *)(uintptr_t)0x2000, 8, H264BSDMI_CELL_SAD, 0, H264BSDMI_BOXES_ABOVE, 0, 8, 1 };
    u32 got[2] = { SENT, SENT }, arr[4][2];
    int rc = -3;
    for (int k = 0; k < 4; k++) arr[k][0] = arr[k][1] = SENT;
    mock_fail = fail;
    mock_call();
    switch (entry) {
    case CHANGE: rc = h264bsdmiOutputRegionChange(2, dec, 2, NULL, &change, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    case SHIFT:  rc = h264bsdmiOutputRegionShift(2, dec, 2, NULL, &shift, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    case CELLS:  rc = h264bsdmiOutputCellMaps(2, dec, 2, NULL, &cells, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    case BOXES:  rc = h264bsdmiOutputCellBoxes(2, dec, 2, NULL, &cells, &boxes, NULL, got, arr[0], arr[1], arr[2], arr[3]); break;
    }
    printf("#%s_%s\nrc=%d\n%s", ENTRY[entry], scenario, rc, *mock_record() ? mock_record() : "sink: not called\n");
    show("got", got, 2);
    show("current", arr[0], 2);
    show("kept", arr[1], 2);
    show("picId", arr[2], 2);
    show("keptPicId", arr[3], 2);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    u32 len_a = 0, len_b = 0;
    u8 *sa = load(argv[1], &len_a), *sb = load(argv[2], &len_b);
    for (int entry = 0; entry < ENTRIES; entry++) {
        Inst A, B;
        make(&A, sa, len_a, 100);
        make(&B, sb, len_b, 200);
        storage_t *const dec[2] = { A.s, B.s };
        u32 kept[2];
        pull(entry, "nothing_kept", dec, 1, 1 | 2);              /* no pair: no sink entry; keep_after keeps, and fails: -2 */
        pull(entry, "still_nothing_kept", dec, 0, 0);            /* ... which marked nothing */
        mock_fail = 0;
        if (h264bsdmiKeepCurrentPictures(1, dec, NULL, kept, NULL) != 0 || kept[0] != 1) return 3;      /* A keeps picture 100 */
        next_picture(&A);                                        /* A's current picture is 101 */
        pull(entry, "plain", dec, 0, 0);                         /* the entry alone */
        pull(entry, "entry_fails", dec, 1, 1);                   /* the entry, and nothing behind a failure */
        pull(entry, "keep_fails", dec, 1, 2);                    /* the entry, then the keep, which fails */
        pull(entry, "marked_nothing", dec, 0, 0);                /* A still holds 100, B nothing */
        pull(entry, "keep_after", dec, 1, 0);                    /* the entry, then the keep: reports what the comparison saw */
        pull(entry, "both_kept", dec, 0, 0);                     /* A holds 101, B 200 */
        h264bsdShutdown(A.s); h264bsdFree(A.s); free(A.buf);
        h264bsdShutdown(B.s); h264bsdFree(B.s); free(B.buf);
    }
    free(sa); free(sb);
    return 0;
}
