/* A device stand-in for sanitizer runs of the host side's THREADED paths (api.c: parser pool, batch calls, two-step pulls): h264bsdInit()
 * binds to it like to the HIP engine, frame jobs are swallowed, and a "picture" is eight bytes — the running picture number of the
 * job that was decoded into the frame buffer — so that a harness can tell which picture a pull handed out.  No pixels, no GPU.
 * The pulls of current pictures are recorded instead (below), for tests/fuzz_asan/current_pulls.c.
 * TEST INFRASTRUCTURE (tests/fuzz_asan/batch_tsan.c, current_pulls.c); the product links engine.hip instead. */
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
#include "engine.h"
#include "framejob.h"

typedef struct Mock { uint64_t *mirror[FJ_MAX_SLOTS + 1]; uint32_t n_slots; int out_slot; long submitted; } Mock;
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;     /* stands for the engine's lock */
static long g_jobs;

static int m_configure(void *u, uint32_t wmb, uint32_t hmb, uint32_t n_slots)
{
    Mock *m = (Mock *)u; (void)wmb; (void)hmb;
    pthread_mutex_lock(&g_mu);
    for (uint32_t i = 0; i <= FJ_MAX_SLOTS; i++) { free(m->mirror[i]); m->mirror[i] = NULL; }
    m->n_slots = n_slots;
    for (uint32_t i = 0; i < n_slots && i <= FJ_MAX_SLOTS; i++) m->mirror[i] = (uint64_t *)calloc(1, sizeof(uint64_t));
    pthread_mutex_unlock(&g_mu);
    return 0;
}
static int m_submit(void *u, const uint8_t *blob, uint32_t bytes)
{
    Mock *m = (Mock *)u;
    const FjHeader *h = (const FjHeader *)blob;
    if (bytes < sizeof(FjHeader) || h->cur_slot >= m->n_slots || !m->mirror[h->cur_slot]) return -1;
    if (!h->dbk_only) *m->mirror[h->cur_slot] = h->pic_seq;
    m->submitted++;
    pthread_mutex_lock(&g_mu); g_jobs++; pthread_mutex_unlock(&g_mu);
    return 0;
}
static int m_fetch_begin(void *u, uint32_t slot)
{
    Mock *m = (Mock *)u;
    m->out_slot = -1;
    if (slot >= m->n_slots || !m->mirror[slot]) return -1;
    pthread_mutex_lock(&g_mu); pthread_mutex_unlock(&g_mu);
    m->out_slot = (int)slot;
    return 0;
}
static uint8_t *m_fetch_end(void *u) { Mock *m = (Mock *)u; return m->out_slot < 0 ? NULL : (uint8_t *)m->mirror[m->out_slot]; }
static uint8_t *m_fetch(void *u, uint32_t slot) { return m_fetch_begin(u, slot) ? NULL : m_fetch_end(u); }
static void m_close(void *u)
{
    Mock *m = (Mock *)u;
    for (uint32_t i = 0; i <= FJ_MAX_SLOTS; i++) free(m->mirror[i]);
    free(m);
}
static uint32_t m_errors(void *u) { (void)u; return 0; }
static int m_set_motion(void *u, int on) { (void)u; (void)on; return 0; }

/* ---- the pulls of CURRENT pictures (api.c), recorded: every entry writes all it was given into one text, which the harness
 * (tests/fuzz_asan/current_pulls.c) takes after the call.  A sink is named by its instance's place in the call (mock_call). ---- */
static char g_rec[1 << 16];
static size_t g_rec_len;
static void *const *g_call_user;
static uint32_t g_call_n;
#define PTR(p) ((unsigned long long)(uintptr_t)(p))
int mock_fail;                  /* the recording entries return -1 (after recording) */
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
void mock_call(uint32_t n, void *const *users) { g_call_n = n; g_call_user = users; g_rec_len = 0; g_rec[0] = 0; }
const char *mock_record(void) { return g_rec; }
static void *g_last;
void *mock_last_attached(void) { return g_last; }
static void rec_pics(const char *who, uint32_t n, const SinkTensorPic *p, uint32_t k, void *stream)
{
    rec("%s m=%u k=%u stream=0x%llx\n", who, n, k, PTR(stream));
    for (uint32_t i = 0; i < n; i++) {
        int inst = -1;
        for (uint32_t j = 0; j < g_call_n; j++) if (g_call_user[j] == p[i].sink->user) inst = (int)j;
        rec(" pic %d slot=%u index=%u win=%u,%u,%u,%u mr=%u,%u box=%u,%u,%u,%u\n", inst, p[i].slot, p[i].index, p[i].x0, p[i].y0, p[i].w, p[i].h,
            p[i].matrix, p[i].range, p[i].box[0], p[i].box[1], p[i].box[2], p[i].box[3]);
    }
}
static void rec_regions(uint32_t k, const SinkRegion *r)
{
    for (uint32_t i = 0; i < k; i++)
        rec(" reg %u index=%u %d,%d,%u,%u box=%u,%u,%u,%u\n", r[i].pic, r[i].index, r[i].x, r[i].y, r[i].w, r[i].h, r[i].box[0], r[i].box[1], r[i].box[2], r[i].box[3]);
}
static void rec_tensor_spec(const h264bsdmi_tensor_spec *s, uint32_t chroma)
{
    rec(" spec 0x%llx %ux%u l=%u d=%u ch=%u crop=%u resize=%u mean=%.9g,%.9g,%.9g std=%.9g,%.9g,%.9g chroma=%u\n", PTR(s->data), s->width, s->height, s->layout,
        s->dtype, s->channels, s->crop, s->resize, s->mean[0], s->mean[1], s->mean[2], s->std[0], s->std[1], s->std[2], chroma);
}
static int m_tensor_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                            const h264bsdmi_resize_spec *z, void *stream)
{
    rec_pics("regions", n, p, k, stream);
    rec_regions(k, r);
    rec_tensor_spec(s, chroma);
    if (z) rec(" resize %u %u pad=%.9g,%.9g,%.9g\n", z->filter, z->fit, z->pad[0], z->pad[1], z->pad[2]);
    else rec(" resize null\n");
    return mock_fail ? -1 : 0;
}
static int m_tensor_remap(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRemap *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                          const h264bsdmi_remap_spec *z, void *stream)
{
    rec_pics("remap", n, p, k, stream);
    for (uint32_t i = 0; i < k; i++) rec(" map %u index=%u 0x%llx\n", r[i].pic, r[i].index, PTR(r[i].map));
    rec_tensor_spec(s, chroma);
    if (z) rec(" remap %u %u pad=%.9g,%.9g,%.9g\n", z->filter, z->border, z->pad[0], z->pad[1], z->pad[2]);
    else rec(" remap null\n");
    return mock_fail ? -1 : 0;
}
static int m_motion_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_motion_spec *s, void *stream)
{
    rec_pics("motion", n, p, k, stream);
    rec_regions(k, r);
    rec(" spec 0x%llx %ux%u l=%u d=%u planes=%u crop=%u fit=%u sampler=%u units=%u per_picture=%u\n", PTR(s->data), s->width, s->height, s->layout, s->dtype,
        s->planes, s->crop, s->fit, s->sampler, s->units, s->per_picture);
    return mock_fail ? -1 : 0;
}
static int m_region_stats(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_stats_spec *s, void *stream)
{
    rec_pics("stats", n, p, k, stream);
    rec_regions(k, r);
    rec(" spec 0x%llx source=%u bins=%u crop=%u\n", PTR(s->data), s->source, s->bins, s->crop);
    return mock_fail ? -1 : 0;
}

int eng_attach(JobSink *s)
{
    Mock *m = (Mock *)calloc(1, sizeof(Mock));
    if (!m) return -1;
    m->out_slot = -1;
    s->user = m; s->configure = m_configure; s->submit = m_submit; s->fetch = m_fetch; s->fetch_begin = m_fetch_begin; s->fetch_end = m_fetch_end;
    s->close = m_close; s->errors = m_errors; s->set_motion = m_set_motion;
    s->tensor_regions = m_tensor_regions; s->tensor_remap = m_tensor_remap; s->motion_regions = m_motion_regions; s->region_stats = m_region_stats;
    g_last = m;
    return 0;
}
void eng_convert_host(int f, uint32_t w, uint32_t h, const uint8_t *d, uint32_t *o) { (void)f; (void)w; (void)h; (void)d; (void)o; }
int eng_sink_device(const JobSink *s) { (void)s; return 0; }
int eng_device_cpus(int d, int *c, int m) { (void)d; (void)c; (void)m; return 0; }
long mock_jobs(void) { pthread_mutex_lock(&g_mu); const long n = g_jobs; pthread_mutex_unlock(&g_mu); return n; }
