/* What the driver programs of the host-path tests share (current_pulls.c, keep_change.c, kept_pulls.c, background.c, region_shift.c,
 * cell_maps.c, cell_boxes.c, corner_points.c): instances of the decoder bound to the recording stand-in (mock_engine.c) over the bytes
 * of a stream, and the print of one named call — "#name", rc, the sink's record or "sink: not called", then the output arrays, which
 * start as a sentinel.  tests/host_program.py builds a driver, runs it and reads those records back.  TEST INFRASTRUCTURE. */
#ifndef HOST_HARNESS_H
#define HOST_HARNESS_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
#include "mock_engine.h"

#define SENT 0xA5A5A5A5u
typedef struct Inst { storage_t *s; void *user; u8 *buf; u32 len, off, id; } Inst;      /* id: the picId its next picture carries */

static inline void no_job(void *user, const u8 *blob, u32 bytes) { (void)user; (void)blob; (void)bytes; }
static inline u8 *load(const char *path, u32 *len)
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
static inline void feed(Inst *t)
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
/* the instance reads these bytes from now on */
static inline void give(Inst *t, const u8 *stream, u32 len)
{
    free(t->buf);
    t->buf = malloc(len); memcpy(t->buf, stream, len); t->len = len; t->off = 0;
}
/* an instance over a stream, fed to its first picture; capture: in capture mode, bound to no sink */
static inline void make(Inst *t, int capture, const u8 *stream, u32 len, u32 id)
{
    memset(t, 0, sizeof(*t));
    t->s = h264bsdAlloc();
    t->id = id;
    if (capture) { if (h264bsdmiInitCapture(t->s, 0, no_job, NULL) != HANTRO_OK) exit(2); }
    else { if (h264bsdInit(t->s, 1) != HANTRO_OK) exit(2); t->user = mock_last_attached(); }
    give(t, stream, len);
    feed(t);
}
static inline void unmake(Inst *t) { h264bsdShutdown(t->s); h264bsdFree(t->s); free(t->buf); }
/* the decoded picture becomes the current one: shown (pop, pop_sized) or not (take) */
static inline void pop(const char *name, Inst *t)
{
    u32 id = SENT;
    const int slot = h264bsdmiNextOutputInfo(t->s, &id, NULL, NULL);
    printf("pop %s slot=%d picId=%u\n", name, slot, id);
}
static inline void pop_sized(const char *name, Inst *t)
{
    u32 id = SENT;
    const int slot = h264bsdmiNextOutputInfo(t->s, &id, NULL, NULL);
    printf("pop %s slot=%d picId=%u size=%ux%u configured=%u\n", name, slot, id, h264bsdPicWidth(t->s), h264bsdPicHeight(t->s), t->user ? mock_configured(t->user) : 0);
}
static inline void take(Inst *t)
{
    if (h264bsdmiNextOutputInfo(t->s, NULL, NULL, NULL) < 0) { fprintf(stderr, "no picture to pop\n"); exit(2); }
}
static inline void next_picture(Inst *t) { feed(t); take(t); }

/* before a call over inst[0 .. n): its decoders and sinks into dec[] and users[], the entries that fail, the record emptied.  No driver
 * but current_pulls.c expects tensor_regions: it fails for all others, so that a stray call fails the API call and shows in the record */
static inline void aim(u32 n, Inst *const *inst, storage_t **dec, void **users, unsigned fail)
{
    for (u32 i = 0; i < n; i++) { dec[i] = inst[i]->s; users[i] = inst[i]->user; }
    mock_fail = fail | MOCK_TENSOR_REGIONS;
    mock_call(n, users);
}
static inline void head(const char *name, int rc) { printf("#%s\nrc=%d\n%s", name, rc, *mock_record() ? mock_record() : "sink: not called\n"); }
/* an output array of n words: "null" when NULL was passed, "untouched" when none of it was written, S where a word is still the sentinel */
static inline void show(const char *name, const u32 *a, size_t n, int passed)
{
    int touched = 0;
    for (size_t i = 0; i < n; i++) touched |= a[i] != SENT;
    printf("%s=", name);
    if (!passed) printf("null");
    else if (!touched) printf("untouched");
    else for (size_t i = 0; i < n; i++) { if (a[i] == SENT) printf("%sS", i ? "," : ""); else printf("%s%u", i ? "," : "", a[i]); }
    printf("\n");
}
/* h264bsdmiKeepCurrentPictures over inst[0 .. n), as a named call; flags: 1 kept NULL, 2 picId NULL */
static inline void keep(const char *name, u32 n, Inst *const *inst, unsigned fail, int flags)
{
    storage_t *dec[4]; void *users[4];
    u32 kept[4] = { SENT, SENT, SENT, SENT }, ids[4] = { SENT, SENT, SENT, SENT };
    aim(n, inst, dec, users, fail);
    const int rc = h264bsdmiKeepCurrentPictures(n, dec, NULL, flags & 1 ? NULL : kept, flags & 2 ? NULL : ids);
    head(name, rc);
    show("kept", kept, n, !(flags & 1));
    show("picId", ids, n, !(flags & 2));
}
#endif
