/* kernels/k_keep.hip.h — the current pictures of many instances copied into their kept-picture buffers
 * (h264bsdmiKeepCurrentPictures, and behind h264bsdmiOutputRegionChange with keep_after): whole coded frames, as macroblock tiles,
 * exactly as they lie.  Included by engine.hip after k_region_stats.hip.h; like its siblings, not part of the kernel sources that key
 * the committed counter tables (srchash.py).
 * grid (chunks, items) x 256: ONE launch for the batch.  A lane moves 16 bytes at a time, a workgroup walks its item in steps of
 * gridDim.x x 4 KB.  bytes is a multiple of 16 (a frame is a whole number of 384-byte tiles) and both addresses are 16-byte aligned. */
#pragma once
namespace h264k {

struct KeepItem { const uint8_t *src; uint8_t *dst; uint32_t bytes; };
constexpr uint32_t KEEP_MAX_CHUNKS = 256;       /* workgroups per item: 256 x 256 lanes x 16 bytes = 1 MB per step */

__global__ __launch_bounds__(256) void k_keep(const KeepItem *__restrict__ items)
{
    const KeepItem it = items[blockIdx.y];
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(it.src);
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(it.dst);
    const uint32_t n = it.bytes >> 4;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) dst[i] = src[i];
}

} // namespace h264k
