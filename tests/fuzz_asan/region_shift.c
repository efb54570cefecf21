/* What the host path of the region shift (api.c: h264bsdmiOutputRegionShift) hands to the engine and writes back, without a GPU: bound
 * to tests/fuzz_asan/mock_engine_shift.c, whose entries record all they are given.  Drives a fixed sequence of named calls and prints
 * per call "#name", rc, the sink's record or "sink: not called", and the output arrays, which start as a sentinel ("untouched" when
 * none of it was written, "null" when NULL was passed).  tests/test_region_shift_host.py builds it, plain and under sanitizers, and
 * checks every record.       usage: region_shift <test_640x360.h264> <test_1920x1080.h264>
 * Instances: A the 640x360 stream (640x368 coded, cropped), B the 1920x1080 stream, each popped once; O as A on a sink without the
 * region_shift entry; G capture mode. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
void mock_call(uint32_t n, void *const *users);
const char *mock_record(void);
void *mock_last_attached(void);
extern int mock_fail, mock_no_shift;

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
static void make(Inst *t, int capture, const u8 *stream, u32 len, u32 id)
{
    memset(t, 0, sizeof(*t));
    t->s = h264bsdAlloc();
    t->id = id;
    if (capture) { if (h264bsdmiInitCapture(t->s, 0, no_job, NULL) != HANTRO_OK) exit(2); }
    else { if (h264bsdInit(t->s, 1) != HANTRO_OK) exit(2); t->user = mock_last_attached(); }
    t->buf = malloc(len); memcpy(t->buf, stream, len); t->len = len;
    feed(t);
}
static void pop(const char *name, Inst *t)
{
    u32 id = SENT;
    const int slot = h264bsdmiNextOutputInfo(t->s, &id, NULL, NULL);
    printf("pop %s slot=%d picId=%u\n", name, slot, id);
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

static void keep(const char *name, u32 n, Inst *const *inst)
{
    storage_t *dec[4]; void *users[4];
    u32 kept[4] = { SENT, SENT, SENT, SENT }, ids[4] = { SENT, SENT, SENT, SENT };
    for (u32 i = 0; i < n; i++) { dec[i] = inst[i]->s; users[i] = inst[i]->user; }
    mock_fail = 0;
    mock_call(n, users);
    const int rc = h264bsdmiKeepCurrentPictures(n, dec, NULL, kept, ids);
    head(name, rc);
    show("kept", kept, n, 1);
    show("picId", ids, n, 1);
}
/* flags: 1 got, 2 current, 4 kept, 8 picId, 16 keptPicId are NULL; 32 a stream is named */
static void shift(const char *name, u32 n, Inst *const *inst, u32 nr, const h264bsdmi_region *regs, const h264bsdmi_shift_spec *spec, int fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 got[8], arr[4][4];
    for (u32 i = 0; i < n; i++) { dec[i] = inst[i]->s; users[i] = inst[i]->user; }
    for (int i = 0; i < 8; i++) got[i] = SENT;
    for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) arr[k][i] = SENT;
    mock_fail = fail;
    mock_call(n, users);
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
    mock_no_shift = 1;
    make(&O, 0, sa, len_a, 400);
    mock_no_shift = 0;
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
    keep("keep_a_only", 1, a);
    shift("a_has_both", 2, ab, 2, NULL, &plain, 0, 0);           /* B: current, nothing kept -> got 1,0 */
    shift("coded_frame", 2, ab, 2, NULL, &frame, 0, 0);          /* crop = 0: 640 x 368; radius 0 */
    shift("boxes_mixed_order", 2, ba, 4, boxes, &plain, 0, 32);  /* B first in the call; boxes name A as instance 1 */
    shift("side_4096", 1, a, 1, side, &plain, 0, 0);             /* the largest side passes */
    shift("null_arrays", 2, ab, 2, NULL, &plain, 0, 2 | 4 | 8 | 16);
    shift("shift_fails", 2, ab, 2, NULL, &chain, 1, 0);          /* -2: nothing written, and keep_after marked nothing */
    shift("keep_after_fails", 2, ab, 2, NULL, &chain, 2, 0);     /* the search went, the keep behind it failed: -2 all the same */
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
    keep("keep_other_sink", 1, o);                               /* a sink with the keep entry and without the shift entry */
    shift("refused_sink_without_entry", 1, o, 1, NULL, &plain, 0, 0);

    /* A decodes on: no current picture, the kept one stays; then the next picture against it */
    feed(&A);
    shift("a_not_current", 1, a, 1, NULL, &plain, 0, 0);
    pop("A", &A);
    shift("a_next_picture", 1, a, 1, NULL, &plain, 0, 0);        /* picId 101 against the kept 100 */

    Inst *all[] = { &A, &B, &O, &G };
    for (int i = 0; i < 4; i++) { h264bsdShutdown(all[i]->s); h264bsdFree(all[i]->s); free(all[i]->buf); }
    free(sa); free(sb);
    return 0;
}
