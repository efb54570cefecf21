// tests/lane_arith/lane_shims.h — what kernels/inter_lane_block.hip.h needs to compile for the host: the few device builtins and helpers of
// kernels/common.hip.h that it uses, in plain C++.  Shared by tests/lane_arith/lane_arith_host.cpp and tools/probes/lane_quads_host.cpp; include it,
// then the kernel header as it is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using std::max; using std::min;
#define __device__
#define __forceinline__ inline
typedef short s2 __attribute__((ext_vector_type(2)));
static inline s2 pk(int x) { return (s2){ (short)x, (short)x }; }
static inline s2 pk_clip(s2 lo, s2 hi, s2 v) { return __builtin_elementwise_min(__builtin_elementwise_max(v, lo), hi); }
static inline s2 as_s2(uint32_t x) { s2 r; memcpy(&r, &x, 4); return r; }
static inline uint32_t as_u32(s2 x) { uint32_t r; memcpy(&r, &x, 4); return r; }
static inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 255u;
        const uint32_t b = s < 8 ? (uint32_t)((v >> (8 * s)) & 255u) : s == 12 ? 0u : (abort(), 0u);
        r |= b << (8 * i);
    }
    return r;
}
static inline int clip255(int v) { return min(max(v, 0), 255); }
static inline int clip3(int lo, int hi, int v) { return min(max(v, lo), hi); }
static inline int level_scale(int m, int cls)
{
    const uint32_t c = cls == 0 ? 0x2507356Au : cls == 1 ? 0x2F4941CDu : 0x3B9BD250u;
    return (int)((c >> (5 * m)) & 31u);
}
constexpr int TILE = 384, T_CB = 256;
#define FJ_CODED_CHROMA_DC (1u << 25)
