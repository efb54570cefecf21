/*
 * engine.h — C interface between the host side (api.c, hostdec) and the HIP engine (engine.hip).
 */
#ifndef H264BSD_AMD_ENGINE_H
#define H264BSD_AMD_ENGINE_H

#include <stdint.h>
#include "hostdec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bind a decoder instance to the device engine: fills *sink.  -1 when no HIP device is usable. */
int  eng_attach(JobSink *sink);
/* Stateless colour conversion of a host I420 frame through the GPU (fmt 0 RGBA, 1 BGRA, 2 YCbCrA). */
void eng_convert_host(int fmt, uint32_t width, uint32_t height, const uint8_t *data, uint32_t *out);
/* The HIP device a bound decoder instance lives on (-1: none), and the CPUs of that device's NUMA node (returns how
 * many were written to cpus[]; 0 when the topology cannot be read). */
int  eng_sink_device(const JobSink *sink);
int  eng_device_cpus(int device, int *cpus, int max);
/* The entries of the engine that came after the last member of JobSink, per sink: what eng_attach would have set in the sink had they
 * been members, NULL for a sink that is not this engine's or has none of them.  A function of the engine beside the sink, to which
 * api.c refers WEAKLY: a device stand-in that was written before it (tests/fuzz_asan) links unchanged, the address is NULL there and
 * api.c refuses the calls that need an entry — refused, not broken — and no stand-in has to grow with the table.  An entry that is
 * NULL in the table is refused likewise.
 *   cell_shift  h264bsdmiOutputCellShift: per cell of a grid over n_regions boxes of the n pictures (distinct instances of one device,
 *               as for JobSink.region_shift) where it lies in the picture against its instance's kept picture — region_shift's search,
 *               one per cell — slice `index` of spec->data each, with one launch.  Every picture's instance has a kept picture of its
 *               coded size; spec->keep_after is not looked at (the caller follows up with keep_pictures).  Called through the table
 *               of any of the n sinks.  0 = ok; <0 = error, nothing enqueued
 *   point_matches  h264bsdmiOutputPointMatches: per region the binary descriptors of the points of spec->kept_points (on the kept
 *               picture of the region's instance) and of spec->current_points (on its current picture), record `index` of each, and
 *               their Hamming matching, into record `index` of spec->data, with two launches on one stream.  The pictures, the kept
 *               pictures, keep_after and the return value as for cell_shift
 *   point_model  h264bsdmiOutputPointModel: per record r < n_records the consensus fit of record r of spec->matches, spec->kept_points
 *               and spec->current_points into record r of spec->data, with one launch.  The first entry without pictures: `sink`, the
 *               sink of the call's first instance, only names the engine and its device; nothing of any instance is read, waited for
 *               or marked.  0 = ok; <0 = error, nothing enqueued
 *   warp_kept   h264bsdmiWarpKeptPictures: the kept picture of every pics[i].sink (distinct instances of one device; each holds one of
 *               its coded size) resampled through maps[i] inside the window pics[i] names, with one launch, and, under
 *               H264BSDMI_WARP_CURRENT, filled from the current picture in pics[i].slot where the source was outside (under REPLICATE
 *               the slot is not looked at: no frame buffer is read).  spec->maps is the caller's list and is not looked at; spec->count:
 *               n_count words, zeroed on the stream ahead of the launch, picture i counts into word pics[i].index.  Called through the
 *               table of any of the n sinks.  0 = ok; <0 = error, nothing enqueued
 *   blend_spread  h264bsdmiBlendCurrentPicturesSpread: JobSink.blend_pictures with the spread beside the kept picture: the n pictures
 *               (distinct instances of one device) blended into their kept pictures under the moving test d > max(hold, V), and V, a
 *               third frame per instance that the engine allocates at the first call, stepped as `spread` says, with one launch.
 *               flags[i]: ENG_SPREAD_FRESH — api.c knows no kept picture of the coded size: the model starts; ENG_SPREAD_UNSET — it
 *               knows no valid spread: V reads as spread->lowest.  spec->moving, n_moving and the return value as for blend_pictures
 *   kept_spread_out  h264bsdmiOutputKeptSpread: the spread of every pics[i].sink (distinct instances of one device; each holds a
 *               kept picture of its coded size and a valid spread) as the planar I420 coded frame into spread[i], with one launch.
 *               0 = ok; <0 = error, nothing enqueued
 * The cell maps' H264BSDMI_CELLS_SPREAD travels through JobSink.cell_maps / cell_boxes; api.c lets it through only where the table
 * carries blend_spread: an engine without the entry has no spread to read. */
#define ENG_SPREAD_FRESH 1u
#define ENG_SPREAD_UNSET 2u
struct h264bsdmi_warp_map;
struct h264bsdmi_warp_spec;
struct h264bsdmi_spread_spec;
typedef struct EngSinkEntries {
    int (*cell_shift)(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                      const struct h264bsdmi_cell_shift_spec *spec, void *stream);
    int (*point_matches)(uint32_t n, const SinkTensorPic *pics, uint32_t n_regions, const SinkRegion *regions,
                         const struct h264bsdmi_matches_spec *spec, void *stream);
    int (*point_model)(const JobSink *sink, uint32_t n_records, const struct h264bsdmi_model_spec *spec, void *stream);
    int (*warp_kept)(uint32_t n, const SinkTensorPic *pics, const struct h264bsdmi_warp_map *maps, const struct h264bsdmi_warp_spec *spec,
                     uint32_t n_count, void *stream);
    int (*blend_spread)(uint32_t n, const SinkTensorPic *pics, const uint32_t *flags, const struct h264bsdmi_blend_spec *spec,
                        const struct h264bsdmi_spread_spec *spread, uint32_t n_moving, void *stream);
    int (*kept_spread_out)(uint32_t n, const SinkTensorPic *pics, void *const *spread, void *stream);
} EngSinkEntries;
const EngSinkEntries *eng_sink_entries(const JobSink *sink);

#ifdef __cplusplus
}
#endif
#endif
