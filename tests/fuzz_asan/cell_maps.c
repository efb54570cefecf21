/* What the host path of the cell maps (api.c: h264bsdmiOutputCellMaps) hands to the engine and writes back, without a GPU: bound to
 * tests/fuzz_asan/mock_engine_cells.c, whose entries record all they are given.  Drives a fixed sequence of named calls and prints per
 * call "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when none
 * of it was written, "null" when NULL was passed); at the end what the output queues of B and of its untouched twin T give.
 * tests/test_cell_maps_host.py builds it, plain and under sanitizers, and checks every record.
 *       usage: cell_maps <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), popped once; B the 1920x1080 stream, fed to its first picture and popped
 * later; T as B, never named in a call; G capture mode; N as A, bound to a sink that cannot keep pictures. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
void mock_call(uint32_t n, void *const *users);
const char *mock_record(void);
void *mock_last_attached(void);
uint32_t mock_configured(const void *user);
extern int mock_fail, mock_without_keep;

#define SENT 0xA5A5A5A5u
typedef struct Inst { storage_t *s; void *user; u8 *buf; u32 len, off, id; } Inst;      /* id: the picId its next picture carries */

static void no_job(void *user, const u8 *blob, u32 bytes) { (void)user; (void)blob; (void)bytes; }
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
/* one more picture decoded */
static void feed(Inst *t)
{
    int stalls = 0;
    while (t->off < t->len && stalls <= 3) {
        u32 rb = 0;
        const u32 r = h264bsdDecode(t->s, t->buf + t->off, t->len - t->off, t->id, &rb);
        t->off += rb;
        stalls = rb ? 0 : stalls + 1;
        if (r == H264BSD_PIC_RDY) { t->id++; return; }
    }
    fprintf(stderr, "stream ended before a picture\n"); exit(2);
}
static void give(Inst *t, const u8 *stream, u32 len)
{
    free(t->buf);
    t->buf = malloc(len); memcpy(t->buf, stream, len); t->len = len; t->off = 0;
}
static void make(Inst *t, int capture, const u8 *stream, u32 len, u32 id)
{
    memset(t, 0, sizeof(*t));
    t->s = h264bsdAlloc();
    t->id = id;
    if (capture) { if (h264bsdmiInitCapture(t->s, 0, no_job, NULL) != HANTRO_OK) exit(2); }
    else { if (h264bsdInit(t->s, 1) != HANTRO_OK) exit(2); t->user = mock_last_attached(); }
    give(t, stream, len);
    feed(t);
}
static void pop(const char *name, Inst *t)
{
    u32 id = SENT;
    const int slot = h264bsdmiNextOutputInfo(t->s, &id, NULL, NULL);
    printf("pop %s slot=%d picId=%u size=%ux%u configured=%u\n", name, slot, id, h264bsdPicWidth(t->s), h264bsdPicHeight(t->s), t->user ? mock_configured(t->user) : 0);
}

static void show(const char *name, const u32 *a, size_t n, int passed)
{
    int touched = 0;
    for (size_t i = 0; i < n; i++) touched |= a[i] != SENT;
    printf("%s=", name);
    if (!passed) printf("null");
    else if (!touched) printf("untouched");
    else for (size_t i = 0; i < n; i++) { if (a[i] == SENT) printf("%sS", i ? "," : ""); else printf("%s%u", i ? "," : "", a[i]); }
    printf("\n");
}
static void head(const char *name, int rc) { printf("#%s\nrc=%d\n%s", name, rc, *mock_record() ? mock_record() : "sink: not called\n"); }

/* flags: 1 kept NULL, 2 picId NULL */
static void keep(const char *name, u32 n, Inst *const *inst, int fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 kept[4] = { SENT, SENT, SENT, SENT }, ids[4] = { SENT, SENT, SENT, SENT };
    for (u32 i = 0; i < n; i++) { dec[i] = inst[i]->s; users[i] = inst[i]->user; }
    mock_fail = fail;
    mock_call(n, users);
    const int rc = h264bsdmiKeepCurrentPictures(n, dec, NULL, flags & 1 ? NULL : kept, flags & 2 ? NULL : ids);
    head(name, rc);
    show("kept", kept, n, !(flags & 1));
    show("picId", ids, n, !(flags & 2));
}
/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named */
static void cells(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_cells_spec *spec, int fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (u32 i = 0; i < n; i++) { dec[i] = inst[i]->s; users[i] = inst[i]->user; }
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    mock_fail = fail;
    mock_call(n, users);
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
    mock_without_keep = 1;
    make(&N, 0, sa, len_a, 400);
    mock_without_keep = 0;
    Inst *const ab[] = { &A, &B }, *const ba[] = { &B, &A }, *const aa[] = { &A, &A }, *const ag[] = { &A, &G }, *const an[] = { &A, &N };
    /*                                  data                        cols rows cell source crop mode planes threshold keep_after */
    const h264bsdmi_cells_spec picture = { (void *)(uintptr_t)0x1000, 40, 23, 16, 1, 1, H264BSDMI_CELLS_PICTURE, 31, { 0, 0, 0 }, 0 };
    const h264bsdmi_cells_spec change = { (void *)(uintptr_t)0x1004, 120, 68, 8, 0, 1, H264BSDMI_CELLS_CHANGE, 35, { 3, 2, 1 }, 0 };
    const h264bsdmi_cells_spec frame = { (void *)(uintptr_t)0x1000, 1, 1, 64, 2, 0, H264BSDMI_CELLS_CHANGE, 1, { 0, 0, 0 }, 0 };
    const h264bsdmi_cells_spec chain = { (void *)(uintptr_t)0x2000, 6, 5, 4, 2, 1, H264BSDMI_CELLS_CHANGE, 63, { 0, 0, 255 }, 1 };
    h264bsdmi_cells_spec bad;
    const h264bsdmi_region boxes[] = { { 1, 0, 0, 64, 64 }, { 0, -5, 7, 100, 30 }, { 1, 700, 10, 8, 8 }, { 0, 0, 0, 640, 360 } };
    pop("A", &A); pop("N", &N);

    /* PICTURE needs no kept picture: A has a current one, B none yet */
    cells("picture_a_only", 2, ab, 2, NULL, &picture, 0, 0);
    /* CHANGE: nobody has kept anything: no pair, no sink */
    cells("nothing_kept", 2, ab, 2, NULL, &change, 0, 0);
    keep("keep_a_only", 2, ab, 0, 0);
    pop("B", &B); pop("T", &T);
    cells("a_has_both", 2, ab, 2, NULL, &change, 0, 0);           /* B: current, nothing kept -> got 1,0 */
    cells("picture_both", 2, ab, 2, NULL, &picture, 0, 0);        /* PICTURE does not ask for a kept picture: got 1,1 */
    cells("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);           /* crop = 0: 640 x 368 */
    cells("boxes_mixed_order", 2, ba, 4, boxes, &change, 0, 32);  /* B first in the call; boxes name A as instance 1 */
    cells("picture_boxes", 2, ba, 4, boxes, &picture, 0, 32);     /* ... and PICTURE takes all four */
    cells("null_arrays", 2, ab, 2, NULL, &change, 0, 2 | 4 | 8 | 16);
    cells("no_regions", 2, ab, 0, boxes, &change, 0, 1);          /* nRegions == 0: 0, nothing launched, got may be NULL */
    cells("cells_fail", 2, ab, 2, NULL, &chain, 1, 0);            /* -2: nothing written, and keep_after marked nothing */
    cells("picture_fails", 2, ab, 2, NULL, &picture, 1, 0);
    cells("keep_after_fails", 2, ab, 2, NULL, &chain, 2, 0);      /* the maps went, the keep behind them failed: -2 all the same */
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
    pop("A", &A);
    cells("a_next_picture", 1, ab, 1, NULL, &change, 0, 0);       /* picId 101 against the kept 100 */

    printf("#final\n");
    u32 idb = SENT, idt = SENT;
    const int slot_b = h264bsdmiNextOutputInfo(B.s, &idb, NULL, NULL), slot_t = h264bsdmiNextOutputInfo(T.s, &idt, NULL, NULL);
    printf("B next=%d,%u\nT next=%d,%u\ntwin=%d\n", slot_b, idb, slot_t, idt, slot_b == slot_t && idb == idt);
    Inst *all[] = { &A, &B, &T, &G, &N };
    for (int i = 0; i < 5; i++) { h264bsdShutdown(all[i]->s); h264bsdFree(all[i]->s); free(all[i]->buf); }
    free(sa); free(sb);
    return 0;
}
