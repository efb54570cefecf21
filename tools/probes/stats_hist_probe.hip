// Region statistics probe: k_region_stats (h264bsd_amd/csrc/kernels/k_region_stats.hip.h) over N synthetic 1080p frames in the
// product's macroblock tiles, whole frames, the launch shape the engine chooses (S row bands per region, about 1024 workgroups).
// Two contents: FLAT (every sample 128: all 64 lanes of a wavefront add to ONE histogram bin) and BUSY (seeded random bytes).
// Prints per source and bins the median kernel time, the bytes read per second, and a device-to-device copy of the same bytes as
// the ceiling.  The histogram variants are compile-time switches of the header:
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 [-DSTATS_HIST_COPIES=4] [-DSTATS_CHROMA_MULT=0] -I../../h264bsd_amd/csrc
//        stats_hist_probe.hip -o stats_hist_probe ; run: ./stats_hist_probe [frames = 256]
#include "kernels.hip.h"
#include "kernels/region_common.hip.h"
#include "kernels/k_region_stats.hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include <random>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

constexpr uint32_t WMB = 120, HMB = 68;
constexpr size_t FRAME = (size_t)WMB * HMB * 384;

static const void *kernel_of(int src, bool hist)
{
    using namespace h264k;
    static const void *const fns[3][2] = {
        { reinterpret_cast<const void *>(&k_region_stats<ST_Y, false>), reinterpret_cast<const void *>(&k_region_stats<ST_Y, true>) },
        { reinterpret_cast<const void *>(&k_region_stats<ST_YCBCR, false>), reinterpret_cast<const void *>(&k_region_stats<ST_YCBCR, true>) },
        { reinterpret_cast<const void *>(&k_region_stats<ST_RGB, false>), reinterpret_cast<const void *>(&k_region_stats<ST_RGB, true>) } };
    return fns[src][hist];
}

int main(int argc, char **argv)
{
    const uint32_t N = argc > 1 ? (uint32_t)atoi(argv[1]) : 256u;
    if (!N || N > 1024u) { printf("frames: 1 .. 1024\n"); return 1; }
    uint8_t *frames, *copy, *recs, *scratch;
    h264k::StatsItem *items;
    CK(hipMalloc(&frames, N * FRAME));
    CK(hipMalloc(&copy, N * FRAME));
    CK(hipMalloc(&recs, (size_t)N * h264k::STATS_MAX_RECORD));
    const size_t tickets = h264k::STATS_MAX_PARTIALS * sizeof(uint32_t);
    CK(hipMalloc(&scratch, tickets + (size_t)h264k::STATS_MAX_PARTIALS * h264k::STATS_MAX_RECORD));
    CK(hipMemset(scratch, 0, tickets));
    CK(hipMalloc(&items, N * sizeof(h264k::StatsItem)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const uint32_t S = N >= h264k::STATS_MAX_PARTIALS ? 1u : std::min(h264k::STATS_MAX_PARTIALS / N, HMB);
    printf("frames %u  bands %u  copies %d  chroma_mult %d  bytes read %.1f MB\n", N, S, STATS_HIST_COPIES, STATS_CHROMA_MULT, N * FRAME / 1e6);

    std::vector<uint8_t> host(FRAME * 8);
    for (int content = 0; content < 2; content++) {
        if (content == 0) memset(host.data(), 128, host.size());
        else { std::mt19937 g(1); for (size_t i = 0; i < host.size(); i += 4) { const uint32_t v = g(); memcpy(&host[i], &v, 4); } }
        for (uint32_t i = 0; i < N; i++) CK(hipMemcpy(frames + i * FRAME, host.data() + (i % 8) * FRAME, FRAME, hipMemcpyHostToDevice));
        std::vector<float> ms;
        for (int rep = 0; rep < 12; rep++) {
            CK(hipEventRecord(e0, 0));
            CK(hipMemcpyAsync(copy, frames, N * FRAME, hipMemcpyDeviceToDevice, 0));
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1));
            if (rep >= 2) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        printf("%s  copy (read + write)             %8.3f ms  %7.1f GB/s read\n", content ? "busy" : "flat", ms[ms.size() / 2], N * FRAME / ms[ms.size() / 2] / 1e6);
        for (int src = 0; src < 3; src++) {
            for (uint32_t bins : { 0u, 16u, 256u }) {
                const uint32_t C = src == 0 ? 1u : 3u, stride = h264k::stats_record_bytes(C, bins);
                std::vector<h264k::StatsItem> h(N);
                for (uint32_t i = 0; i < N; i++) h[i] = h264k::StatsItem{ frames + i * FRAME, recs + (size_t)i * stride, WMB, 0u, 0u, 1920u, 1080u };
                CK(hipMemcpy(items, h.data(), N * sizeof(h264k::StatsItem), hipMemcpyHostToDevice));
                uint32_t shift = 8; while (bins && (256u >> shift) != bins) shift--;
                h264k::StatsArgs a{ items, scratch + tickets, reinterpret_cast<uint32_t *>(scratch), bins, bins ? shift : 0u };
                void *args[] = { &a };
                ms.clear();
                for (int rep = 0; rep < 12; rep++) {
                    CK(hipEventRecord(e0, 0));
                    CK(hipLaunchKernel(kernel_of(src, bins != 0), dim3(S, N), dim3(256), args, 0, 0));
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    float t; CK(hipEventElapsedTime(&t, e0, e1));
                    if (rep >= 2) ms.push_back(t);
                }
                std::sort(ms.begin(), ms.end());
                /* the record of frame 0: count, and the luma sum, so that a variant that computes something else shows */
                uint32_t head[4];
                CK(hipMemcpy(head, recs, sizeof(head), hipMemcpyDeviceToHost));
                const double bytes = (double)N * WMB * HMB * (src == 0 ? 256 : 384);      /* STATS_Y leaves the chroma lines alone */
                printf("%s  source %d bins %3u              %8.3f ms  %7.1f GB/s read   count %u sum0 %u\n", content ? "busy" : "flat", src, bins,
                       ms[ms.size() / 2], bytes / ms[ms.size() / 2] / 1e6, head[0], head[2]);
            }
        }
    }
    return 0;
}
