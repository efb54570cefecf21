/* A recording device stand-in for the ONE host path of the pulls that may compare against kept pictures (api.c: kept_pull, behind
 * h264bsdmiOutputRegionChange, h264bsdmiOutputRegionShift, h264bsdmiOutputCellMaps and h264bsdmiOutputCellBoxes), for
 * tests/fuzz_asan/kept_pulls.c: h264bsdInit() binds to it like to the HIP engine, frame jobs are swallowed, and every sink entry writes
 * its name and how many pictures and regions it was given into one text, which the harness takes after the call.  What each entry is
 * handed in full is the business of the stand-ins of the four features.  No pixels, no GPU.  TEST INFRASTRUCTURE; the product links
 * engine.hip instead. */
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

static char g_rec[1024];
int mock_fail;                  /* bit 0: the four entries, bit 1: keep_pictures return -1 (after recording) */
void mock_call(void) { g_rec[0] = 0; }
const char *mock_record(void) { return g_rec; }
static int rec(const char *who, uint32_t n, uint32_t k, int fails)
{
    const size_t at = strlen(g_rec);
    snprintf(g_rec + at, sizeof(g_rec) - at, "%s m=%u k=%u\n", who, n, k);
    return fails ? -1 : 0;
}

static int m_tensor_regions(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_tensor_spec *s, uint32_t chroma,
                            const h264bsdmi_resize_spec *z, void *stream)
{
    (void)p; (void)r; (void)s; (void)chroma; (void)z; (void)stream;
    return rec("regions: not expected", n, k, 1);
}
static int m_keep_pictures(uint32_t n, const SinkTensorPic *p, void *stream) { (void)p; (void)stream; return rec("keep", n, 0, mock_fail & 2); }
static int m_region_change(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_change_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    return rec("change", n, k, mock_fail & 1);
}
static int m_region_shift(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_shift_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    return rec("shift", n, k, mock_fail & 1);
}
static int m_cell_maps(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_cells_spec *s, void *stream)
{
    (void)p; (void)r; (void)s; (void)stream;
    return rec("cells", n, k, mock_fail & 1);
}
static int m_cell_boxes(uint32_t n, const SinkTensorPic *p, uint32_t k, const SinkRegion *r, const h264bsdmi_cells_spec *s,
                        const h264bsdmi_boxes_spec *b, void *stream)
{
    (void)p; (void)r; (void)s; (void)b; (void)stream;
    return rec("boxes", n, k, mock_fail & 1);
}

int eng_attach(JobSink *s)
{
    Mock *m = (Mock *)calloc(1, sizeof(Mock));
    if (!m) return -1;
    s->user = m; s->configure = m_configure; s->submit = m_submit; s->close = m_close; s->errors = m_errors;
    s->tensor_regions = m_tensor_regions; s->keep_pictures = m_keep_pictures; s->region_change = m_region_change;
    s->region_shift = m_region_shift; s->cell_maps = m_cell_maps; s->cell_boxes = m_cell_boxes;
    return 0;
}
void eng_convert_host(int f, uint32_t w, uint32_t h, const uint8_t *d, uint32_t *o) { (void)f; (void)w; (void)h; (void)d; (void)o; }
int eng_sink_device(const JobSink *s) { (void)s; return 0; }
int eng_device_cpus(int d, int *c, int m) { (void)d; (void)c; (void)m; return 0; }
