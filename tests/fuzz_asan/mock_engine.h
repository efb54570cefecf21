/* How a test program steers the recording device stand-in (mock_engine.c) and reads what it recorded.  TEST INFRASTRUCTURE. */
#ifndef MOCK_ENGINE_H
#define MOCK_ENGINE_H
#include <stdint.h>

/* the optional JobSink entries the stand-in records, one bit each, in the order of the struct's members (hostdec.h) */
enum {
    MOCK_TENSOR_REGIONS = 1 << 0,
    MOCK_MOTION_REGIONS = 1 << 1,
    MOCK_TENSOR_REMAP = 1 << 2,
    MOCK_REGION_STATS = 1 << 3,
    MOCK_KEEP_PICTURES = 1 << 4,
    MOCK_REGION_CHANGE = 1 << 5,
    MOCK_REGION_SHIFT = 1 << 6,
    MOCK_CELL_MAPS = 1 << 7,
    MOCK_CELL_BOXES = 1 << 8,
    MOCK_BLEND_PICTURES = 1 << 9,
    MOCK_KEPT_PICTURES_OUT = 1 << 10,
    MOCK_CORNER_POINTS = 1 << 11,
};
extern unsigned mock_fail;          /* these entries return -1 (after recording) */
extern unsigned mock_without;       /* eng_attach leaves these entries NULL in the sink of the instance it attaches: a sink that lacks them */

/* the instances of the call about to be made, so that a sink is named by its place among them; empties the record */
void mock_call(uint32_t n, void *const *users);
const char *mock_record(void);                      /* all the entries were given since mock_call, as text */
void *mock_last_attached(void);                     /* JobSink.user of the instance attached last */
uint32_t mock_configured(const void *user);         /* how often that instance's sink was configured */
long mock_jobs(void);                               /* frame jobs submitted so far, all instances */
#endif
