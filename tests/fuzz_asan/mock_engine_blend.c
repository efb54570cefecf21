/* A recording device stand-in for the host path of the background model (api.c: h264bsdmiBlendCurrentPictures,
 * h264bsdmiOutputKeptPictures), for tests/fuzz_asan/background.c: h264bsdInit() binds to it like to the HIP engine, frame jobs are
 * swallowed, and the sink entries write all they are given into one text, which the harness takes after the call.  No pixels, no GPU.
 * TEST INFRASTRUCTURE; the product links engine.hip instead. */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
#include "engine.h"
#include "framejob.h"

typedef struct Mock { uint32_t n_slots; } Mock;

static int m_configure(void *u, uint32_t wmb, uint32_t hmb, uint32_t n_slots) { (void)wmb; (void)hmb; ((Mock *)u)->n_slots = n_slots; return 0; }
static int m_submit(void *u, const uint8_t *blob, uint32_t bytes)
{
    const FjHeader *h = (const FjHeader *)blob;
    return bytes < sizeof(FjHeader) || h->cur_slot >= ((const Mock *)u)->n_slots ? -1 : 0;
}
static void m_close(void *u) { free(u); }
static uint32_t m_errors(void *u) { (void)u; return 0; }

static char g_rec[1 << 13];
static size_t g_rec_len;
static void *const *g_call_user;
static uint32_t g_call_n;
#define PTR(p) ((unsigned long long)(uintptr_t)(p))
int mock_fail;                  /* the entries return -1 (after recording) */
int mock_no_blend;              /* eng_attach leaves JobSink.blend_pictures and kept_pictures_out unset: a sink from before they existed */
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

static int inst_of(const SinkTensorPic *p)
{
    for (uint32_t j = 0; j < g_call_n; j++) if (g_call_user[j] == p->sink->user) return (int)j;
    return -1;
}
static int m_tensor_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                            const h264bsdmi_resize_spec *z, void *stream)
{
    (void)n; (void)p; (void)k; (void)r; (void)s; (void)chroma; (void)z; (void)stream;
    rec("regions: not expected\n");
    return -1;
}
static int m_keep_pictures(uint32_t n, const SinkTensorPic *p, void *stream)
{
    rec("keep m=%u stream=0x%llx\n", n, PTR(stream));
    for (uint32_t i = 0; i < n; i++) rec(" pic %d slot=%u\n", inst_of(&p[i]), p[i].slot);
    return mock_fail ? -1 : 0;
}
static int m_blend_pictures(uint32_t n, const SinkTensorPic *p, const uint32_t *fresh, const h264bsdmi_blend_spec *s, uint32_t n_moving, void *stream)
{
    rec("blend m=%u n_moving=%u stream=0x%llx\n", n, n_moving, PTR(stream));
    for (uint32_t i = 0; i < n; i++)
        rec(" pic %d index=%u slot=%u win=%u,%u,%u,%u mr=%u,%u fresh=%u\n", inst_of(&p[i]), p[i].index, p[i].slot, p[i].x0, p[i].y0, p[i].w, p[i].h,
            p[i].matrix, p[i].range, fresh[i]);
    rec(" spec shift=%u hold=%u moving_shift=%u moving=0x%llx\n", s->shift, s->hold, s->moving_shift, PTR(s->moving));
    return mock_fail ? -1 : 0;
}
static int m_kept_pictures_out(uint32_t n, const SinkTensorPic *p, void *const *picture, void *const *fraction, void *stream)
{
    rec("kept_out m=%u stream=0x%llx\n", n, PTR(stream));
    for (uint32_t i = 0; i < n; i++) rec(" inst %d picture=0x%llx fraction=0x%llx\n", inst_of(&p[i]), PTR(picture[i]), PTR(fraction[i]));
    return mock_fail ? -1 : 0;
}

int eng_attach(JobSink *s)
{
    Mock *m = (Mock *)calloc(1, sizeof(Mock));
    if (!m) return -1;
    s->user = m; s->configure = m_configure; s->submit = m_submit; s->close = m_close; s->errors = m_errors;
    s->tensor_regions = m_tensor_regions; s->keep_pictures = m_keep_pictures;
    if (!mock_no_blend) { s->blend_pictures = m_blend_pictures; s->kept_pictures_out = m_kept_pictures_out; }
    g_last = m;
    return 0;
}
void eng_convert_host(int f, uint32_t w, uint32_t h, const uint8_t *d, uint32_t *o) { (void)f; (void)w; (void)h; (void)d; (void)o; }
int eng_sink_device(const JobSink *s) { (void)s; return 0; }
int eng_device_cpus(int d, int *c, int m) { (void)d; (void)c; (void)m; return 0; }
