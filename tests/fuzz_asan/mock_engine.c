/* The recording device stand-in of the host side's tests: h264bsdInit() binds to it like to the HIP engine, frame jobs are swallowed, and
 * a "picture" is eight bytes — the running picture number of the job that was decoded into the frame buffer — so that a harness of the
 * THREADED paths (batch_tsan.c: parser pool, batch calls, two-step pulls) can tell which picture a pull handed out.  No pixels, no GPU.
 * Every optional sink entry that works on current or kept pictures writes all it was given into one text, which the driver programs
 * beside this file take after the call; mock_engine.h says how they steer it.  stub_engine.c is the stand-in that knows no optional entry.
 * TEST INFRASTRUCTURE; the product links engine.hip instead. */
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264bsd_mi355x.h"
#include "engine.h"
#include "framejob.h"
#include "mock_engine.h"

typedef struct Mock { uint64_t *mirror[FJ_MAX_SLOTS + 1]; uint32_t wmb, hmb, n_slots, configured; int out_slot; long submitted; } Mock;
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;     /* stands for the engine's lock */
static long g_jobs;

static int m_configure(void *u, uint32_t wmb, uint32_t hmb, uint32_t n_slots)
{
    Mock *m = (Mock *)u;
    pthread_mutex_lock(&g_mu);
    for (uint32_t i = 0; i <= FJ_MAX_SLOTS; i++) { free(m->mirror[i]); m->mirror[i] = NULL; }
    m->wmb = wmb; m->hmb = hmb; m->n_slots = n_slots; m->configured++;
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

/* ---- the recorded entries.  A sink is named by its instance's place in the call (mock_call). ---- */
static char g_rec[1 << 16];
static size_t g_rec_len;
static void *const *g_call_user;
static uint32_t g_call_n;
static void *g_last;
#define PTR(p) ((unsigned long long)(uintptr_t)(p))
unsigned mock_fail, mock_without;
void mock_call(uint32_t n, void *const *users) { g_call_n = n; g_call_user = users; g_rec_len = 0; g_rec[0] = 0; }
const char *mock_record(void) { return g_rec; }
void *mock_last_attached(void) { return g_last; }
uint32_t mock_configured(const void *user) { return ((const Mock *)user)->configured; }
long mock_jobs(void) { pthread_mutex_lock(&g_mu); const long n = g_jobs; pthread_mutex_unlock(&g_mu); return n; }

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
static int done(unsigned entry) { return mock_fail & entry ? -1 : 0; }
static int inst_of(const SinkTensorPic *p)
{
    for (uint32_t j = 0; j < g_call_n; j++) if (g_call_user[j] == p->sink->user) return (int)j;
    return -1;
}
/* the head line and the pictures; full: with index and box, as the tensor pulls and their pins read them */
static void rec_pics(const char *who, uint32_t n, const SinkTensorPic *p, uint32_t k, void *stream, int full)
{
    rec("%s m=%u k=%u stream=0x%llx\n", who, n, k, PTR(stream));
    for (uint32_t i = 0; i < n; i++) {
        rec(" pic %d slot=%u", inst_of(&p[i]), p[i].slot);
        if (full) rec(" index=%u", p[i].index);
        rec(" win=%u,%u,%u,%u mr=%u,%u", p[i].x0, p[i].y0, p[i].w, p[i].h, p[i].matrix, p[i].range);
        if (full) rec(" box=%u,%u,%u,%u", p[i].box[0], p[i].box[1], p[i].box[2], p[i].box[3]);
        rec("\n");
    }
}
static void rec_regions(uint32_t k, const SinkRegion *r, int full)
{
    for (uint32_t i = 0; i < k; i++) {
        rec(" reg %u index=%u %d,%d,%u,%u", r[i].pic, r[i].index, r[i].x, r[i].y, r[i].w, r[i].h);
        if (full) rec(" box=%u,%u,%u,%u", r[i].box[0], r[i].box[1], r[i].box[2], r[i].box[3]);
        rec("\n");
    }
}
static void rec_tensor_spec(const h264bsdmi_tensor_spec *s, uint32_t chroma)
{
    rec(" spec 0x%llx %ux%u l=%u d=%u ch=%u crop=%u resize=%u mean=%.9g,%.9g,%.9g std=%.9g,%.9g,%.9g chroma=%u\n", PTR(s->data), s->width, s->height, s->layout,
        s->dtype, s->channels, s->crop, s->resize, s->mean[0], s->mean[1], s->mean[2], s->std[0], s->std[1], s->std[2], chroma);
}
static void rec_cells_spec(const h264bsdmi_cells_spec *s)
{
    rec(" spec 0x%llx grid=%ux%u cell=%u source=%u crop=%u mode=%u planes=%u thr=%u,%u,%u keep_after=%u\n", PTR(s->data), s->rows, s->cols, s->cell,
        s->source, s->crop, s->mode, s->planes, s->threshold[0], s->threshold[1], s->threshold[2], s->keep_after);
}

static int m_tensor_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                            const h264bsdmi_resize_spec *z, void *stream)
{
    rec_pics("regions", n, p, k, stream, 1);
    rec_regions(k, r, 1);
    rec_tensor_spec(s, chroma);
    if (z) rec(" resize %u %u pad=%.9g,%.9g,%.9g\n", z->filter, z->fit, z->pad[0], z->pad[1], z->pad[2]);
    else rec(" resize null\n");
    return done(MOCK_TENSOR_REGIONS);
}
static int m_motion_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_motion_spec *s, void *stream)
{
    rec_pics("motion", n, p, k, stream, 1);
    rec_regions(k, r, 1);
    rec(" spec 0x%llx %ux%u l=%u d=%u planes=%u crop=%u fit=%u sampler=%u units=%u per_picture=%u\n", PTR(s->data), s->width, s->height, s->layout, s->dtype,
        s->planes, s->crop, s->fit, s->sampler, s->units, s->per_picture);
    return done(MOCK_MOTION_REGIONS);
}
static int m_tensor_remap(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRemap *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                          const h264bsdmi_remap_spec *z, void *stream)
{
    rec_pics("remap", n, p, k, stream, 1);
    for (uint32_t i = 0; i < k; i++) rec(" map %u index=%u 0x%llx\n", r[i].pic, r[i].index, PTR(r[i].map));
    rec_tensor_spec(s, chroma);
    if (z) rec(" remap %u %u pad=%.9g,%.9g,%.9g\n", z->filter, z->border, z->pad[0], z->pad[1], z->pad[2]);
    else rec(" remap null\n");
    return done(MOCK_TENSOR_REMAP);
}
static int m_region_stats(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_stats_spec *s, void *stream)
{
    rec_pics("stats", n, p, k, stream, 1);
    rec_regions(k, r, 1);
    rec(" spec 0x%llx source=%u bins=%u crop=%u\n", PTR(s->data), s->source, s->bins, s->crop);
    return done(MOCK_REGION_STATS);
}
static int m_keep_pictures(uint32_t n, const SinkTensorPic *p, void *stream)
{
    rec_pics("keep", n, p, 0, stream, 0);
    return done(MOCK_KEEP_PICTURES);
}
static int m_region_change(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_change_spec *s, void *stream)
{
    rec_pics("change", n, p, k, stream, 0);
    rec_regions(k, r, 0);
    rec(" spec 0x%llx source=%u bins=%u crop=%u thr=%u,%u,%u keep_after=%u\n", PTR(s->data), s->source, s->bins, s->crop, s->threshold[0],
        s->threshold[1], s->threshold[2], s->keep_after);
    return done(MOCK_REGION_CHANGE);
}
static int m_region_shift(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_shift_spec *s, void *stream)
{
    rec_pics("shift", n, p, k, stream, 0);
    rec_regions(k, r, 0);
    rec(" spec 0x%llx radius=%u surface=%u crop=%u keep_after=%u\n", PTR(s->data), s->radius, s->surface, s->crop, s->keep_after);
    return done(MOCK_REGION_SHIFT);
}
static int m_cell_maps(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_cells_spec *s, void *stream)
{
    rec_pics("cells", n, p, k, stream, 0);
    rec_regions(k, r, 0);
    rec_cells_spec(s);
    return done(MOCK_CELL_MAPS);
}
static int m_cell_boxes(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_cells_spec *s,
                        const h264bsdmi_boxes_spec *b, void *stream)
{
    rec_pics("boxes", n, p, k, stream, 0);
    rec_regions(k, r, 0);
    rec_cells_spec(s);
    rec(" boxes 0x%llx max=%u plane=%u channel=%u sense=%u level=%u conn=%u min_cells=%u\n", PTR(b->data), b->max_boxes, b->plane, b->channel, b->sense,
        b->level, b->connectivity, b->min_cells);
    return done(MOCK_CELL_BOXES);
}
static int m_blend_pictures(uint32_t n, const SinkTensorPic *p, const uint32_t *fresh, const h264bsdmi_blend_spec *s, uint32_t n_moving, void *stream)
{
    rec("blend m=%u n_moving=%u stream=0x%llx\n", n, n_moving, PTR(stream));
    for (uint32_t i = 0; i < n; i++)
        rec(" pic %d index=%u slot=%u win=%u,%u,%u,%u mr=%u,%u fresh=%u\n", inst_of(&p[i]), p[i].index, p[i].slot, p[i].x0, p[i].y0, p[i].w, p[i].h,
            p[i].matrix, p[i].range, fresh[i]);
    rec(" spec shift=%u hold=%u moving_shift=%u moving=0x%llx\n", s->shift, s->hold, s->moving_shift, PTR(s->moving));
    return done(MOCK_BLEND_PICTURES);
}
static int m_kept_pictures_out(uint32_t n, const SinkTensorPic *p, void *const *picture, void *const *fraction, void *stream)
{
    rec("kept_out m=%u stream=0x%llx\n", n, PTR(stream));
    for (uint32_t i = 0; i < n; i++) rec(" inst %d picture=0x%llx fraction=0x%llx\n", inst_of(&p[i]), PTR(picture[i]), PTR(fraction[i]));
    return done(MOCK_KEPT_PICTURES_OUT);
}
static int m_corner_points(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_corners_spec *s, void *stream)
{
    rec_pics("corners", n, p, k, stream, 0);
    rec_regions(k, r, 0);
    rec(" spec 0x%llx score=%u block=%u nms=%u max_points=%u crop=%u zero=%u min_score=%llu\n", PTR(s->data), s->score, s->block, s->nms,
        s->max_points, s->crop, s->zero, s->min_score);
    return done(MOCK_CORNER_POINTS);
}

int eng_attach(JobSink *s)
{
    Mock *m = (Mock *)calloc(1, sizeof(Mock));
    if (!m) return -1;
    m->out_slot = -1;
    s->user = m; s->configure = m_configure; s->submit = m_submit; s->fetch = m_fetch; s->fetch_begin = m_fetch_begin; s->fetch_end = m_fetch_end;
    s->close = m_close; s->errors = m_errors; s->set_motion = m_set_motion;
    /* what the host paths under test do without: no staging memory, no converted or device pictures, no whole-picture tensors */
    s->acquire = NULL; s->fetch_converted = NULL; s->fetch_device = NULL; s->tensor_out = NULL;
    s->tensor_regions = mock_without & MOCK_TENSOR_REGIONS ? NULL : m_tensor_regions;
    s->motion_regions = mock_without & MOCK_MOTION_REGIONS ? NULL : m_motion_regions;
    s->tensor_remap = mock_without & MOCK_TENSOR_REMAP ? NULL : m_tensor_remap;
    s->region_stats = mock_without & MOCK_REGION_STATS ? NULL : m_region_stats;
    s->keep_pictures = mock_without & MOCK_KEEP_PICTURES ? NULL : m_keep_pictures;
    s->region_change = mock_without & MOCK_REGION_CHANGE ? NULL : m_region_change;
    s->region_shift = mock_without & MOCK_REGION_SHIFT ? NULL : m_region_shift;
    s->cell_maps = mock_without & MOCK_CELL_MAPS ? NULL : m_cell_maps;
    s->cell_boxes = mock_without & MOCK_CELL_BOXES ? NULL : m_cell_boxes;
    s->blend_pictures = mock_without & MOCK_BLEND_PICTURES ? NULL : m_blend_pictures;
    s->kept_pictures_out = mock_without & MOCK_KEPT_PICTURES_OUT ? NULL : m_kept_pictures_out;
    s->corner_points = mock_without & MOCK_CORNER_POINTS ? NULL : m_corner_points;
    g_last = m;
    return 0;
}
void eng_convert_host(int f, uint32_t w, uint32_t h, const uint8_t *d, uint32_t *o) { (void)f; (void)w; (void)h; (void)d; (void)o; }
int eng_sink_device(const JobSink *s) { (void)s; return 0; }
int eng_device_cpus(int d, int *c, int m) { (void)d; (void)c; (void)m; return 0; }
