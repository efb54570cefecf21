/* A recording device stand-in for the host path of the corner points (api.c: h264bsdmiOutputCornerPoints), for
 * tests/fuzz_asan/corner_points.c: h264bsdInit() binds to it like to the HIP engine, frame jobs are swallowed, and the sink entry writes
 * all it is given into one text, which the harness takes after the call.  An instance attached while mock_no_corners is set gets a sink
 * WITHOUT the corner_points entry, as the older stand-ins are.  No pixels, no GPU.  TEST INFRASTRUCTURE; the product links engine.hip
 * instead. */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
#include "engine.h"
#include "framejob.h"

typedef struct Mock { uint32_t wmb, hmb, n_slots, configured; } Mock;

static int m_configure(void *u, uint32_t wmb, uint32_t hmb, uint32_t n_slots)
{
    Mock *m = (Mock *)u;
    m->wmb = wmb; m->hmb = hmb; m->n_slots = n_slots; m->configured++;
    return 0;
}
static int m_submit(void *u, const uint8_t *blob, uint32_t bytes)
{
    const Mock *m = (const Mock *)u;
    const FjHeader *h = (const FjHeader *)blob;
    return bytes < sizeof(FjHeader) || h->cur_slot >= m->n_slots ? -1 : 0;
}
static void m_close(void *u) { free(u); }
static uint32_t m_errors(void *u) { (void)u; return 0; }

static char g_rec[1 << 14];
static size_t g_rec_len;
static void *const *g_call_user;
static uint32_t g_call_n;
#define PTR(p) ((unsigned long long)(uintptr_t)(p))
int mock_fail;                  /* corner_points returns -1 (after recording) */
int mock_no_corners;            /* eng_attach leaves JobSink.corner_points unset */
static void rec(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (g_rec_len < sizeof(g_rec) - 1) {
        const int w = vsnprintf(g_rec + g_rec_len, sizeof(g_rec) - g_rec_len, fmt, ap);
        if (w > 0) g_rec_len = g_rec_len + (size_t)w < sizeof(g_rec) ? g_rec_len + (size_t)w : sizeof(g_rec) - 1;
    }
    va_end(ap);
}
/* the instances of the call about to be made, so that a sink can be named by its place among them */
void mock_call(uint32_t n, void *const *users) { g_call_n = n; g_call_user = users; g_rec_len = 0; g_rec[0] = 0; }
const char *mock_record(void) { return g_rec; }
static void *g_last;
void *mock_last_attached(void) { return g_last; }

static int m_tensor_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                            const h264bsdmi_resize_spec *z, void *stream)
{
    (void)n; (void)p; (void)k; (void)r; (void)s; (void)chroma; (void)z; (void)stream;
    rec("regions: not expected\n");
    return -1;
}
static int m_corner_points(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_corners_spec *s, void *stream)
{
    rec("corners m=%u k=%u stream=0x%llx\n", n, k, PTR(stream));
    for (uint32_t i = 0; i < n; i++) {
        int inst = -1;
        for (uint32_t j = 0; j < g_call_n; j++) if (g_call_user[j] == p[i].sink->user) inst = (int)j;
        rec(" pic %d slot=%u win=%u,%u,%u,%u mr=%u,%u\n", inst, p[i].slot, p[i].x0, p[i].y0, p[i].w, p[i].h, p[i].matrix, p[i].range);
    }
    for (uint32_t i = 0; i < k; i++) rec(" reg %u index=%u %d,%d,%u,%u\n", r[i].pic, r[i].index, r[i].x, r[i].y, r[i].w, r[i].h);
    rec(" spec 0x%llx score=%u block=%u nms=%u max_points=%u crop=%u zero=%u min_score=%llu\n", PTR(s->data), s->score, s->block, s->nms,
        s->max_points, s->crop, s->zero, s->min_score);
    return mock_fail ? -1 : 0;
}

int eng_attach(JobSink *s)
{
    Mock *m = (Mock *)calloc(1, sizeof(Mock));
    if (!m) return -1;
    s->user = m; s->configure = m_configure; s->submit = m_submit; s->close = m_close; s->errors = m_errors;
    s->tensor_regions = m_tensor_regions;
    if (!mock_no_corners) s->corner_points = m_corner_points;
    g_last = m;
    return 0;
}
void eng_convert_host(int f, uint32_t w, uint32_t h, const uint8_t *d, uint32_t *o) { (void)f; (void)w; (void)h; (void)d; (void)o; }
int eng_sink_device(const JobSink *s) { (void)s; return 0; }
int eng_device_cpus(int d, int *c, int m) { (void)d; (void)c; (void)m; return 0; }
