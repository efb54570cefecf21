/* kernels/k_point_model.hip.h — WHICH motion do the point matches agree on: an exhaustive consensus fit of a translation or a similarity
 * (rotation, uniform scale, translation) to the accepted slots of h264bsdmiOutputPointMatches records (h264bsdmiOutputPointModel).  No
 * picture is read: the inputs are three caller records per region, the output one record.  Included by engine.hip after
 * k_point_matches.hip.h; the wave sum is region_common.hip.h's; like them, not part of the kernel sources that key the committed counter
 * tables (srchash.py).
 *
 * The quantity (include/h264bsd_mi355x.h has it in full), all integers, points as complex numbers, p of the kept record, q of the current:
 *     usable      slot i: ACCEPTED, 0 <= j < K, i < min(kept written, K), j < min(current written, K), all four coordinates in 0 .. 16383
 *     TRANSLATION hypothesis a: t = q_a - p_a; i is an inlier iff |q_i - p_i - t|^2 <= tol^2
 *     SIMILARITY  hypothesis a < b, P = p_b - p_a != 0, Q = q_b - q_a != 0, with max_scale S: 65536 |Q|^2 <= S^2 |P|^2 and the converse;
 *                 i is an inlier iff |(q_i - q_a) P - Q (p_i - p_a)|^2 <= tol^2 |P|^2
 *     best        most inliers, then the smallest a, then the smallest b; found iff there is one with count >= min_inliers
 *     record      u32 usable, hypotheses, inliers, found; i32 a, b; u32 0, 0; i64 sum[12]; K x u32 flags: 128 + 4 K bytes, written whole
 * k_point_model, grid (records) x MODEL_THREADS, one workgroup per record:
 *   1. thread i < K reads slot i; the usable pairs are compacted into LDS in slot order (ballot, prefix of the wave, counts of the waves
 *      before), so an index among the n pairs orders as the slot does.
 *   2. the n (n - 1) / 2 hypotheses are laid out as rows of n: row r holds (r, r + 1 ..) and behind it (n - 2 - r, n - 1 - r ..), so that
 *      every thread of a step has one.  A thread carries its hypothesis in registers — P, Q and the constant C = q_a P - Q p_a — and
 *      walks all n pairs with one broadcast 16-byte LDS read each: the residual q_i P - Q p_i - C is eight 24-bit multiply-adds (every
 *      factor is below 2^14 in magnitude, the sums wrap mod 2^32 and the result, below 2^30 in magnitude, is exact), its squared norm two
 *      64-bit multiply-adds, below 2^61, against tol^2 |P|^2 < 2^45.  The thread's best becomes the key count << 16 | (255 - a) << 8 |
 *      (255 - b), larger is better, 0 is "none" (a hypothesis counts its own points: count >= 1); keys meet in a maximum over the
 *      wavefront and an LDS atomic maximum over the workgroup, the counts of hypotheses in a sum: integers, no order shows.
 *   3. thread i < K tests slot i against the winner straight from the definition (differences, 32-bit products, 64-bit squares), writes
 *      its flags, and the twelve moment sums are 64-bit sums over wavefronts, then over the four of them.
 * The three inputs are caller memory: `written` and j are clamped or checked before they index anything, and a coordinate enters
 * arithmetic only after it was found in 0 .. 16383, so whatever they hold no byte outside the three records of r is read and nothing
 * overflows.  Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md §4.4 quotes them; no scratch,
 * no spills. */
#pragma once
namespace h264k {

constexpr uint32_t MODEL_MAX_K = 256;
#ifndef MODEL_THREADS_N
#define MODEL_THREADS_N 1024                                        /* (a build flag for measurements: docs/EXPERIMENTS.md, "Point model") */
#endif
constexpr uint32_t MODEL_THREADS = MODEL_THREADS_N;                 /* 16 wavefronts: four a SIMD, to cover the LDS reads of the walk */
static_assert(MODEL_THREADS >= 256u && MODEL_THREADS <= 1024u && MODEL_THREADS % 64u == 0u, "whole wavefronts, and a thread per slot");
constexpr uint32_t MODEL_COORD_MAX = 16383;
constexpr uint32_t MODEL_TRANSLATION = 0, MODEL_SIMILARITY = 1;
constexpr uint32_t MODEL_SUMS = 12;
static_assert(MODEL_MAX_K <= 256u && MODEL_MAX_K <= MODEL_THREADS, "a thread owns a slot; an index fits a byte of the key");

__host__ __device__ constexpr uint32_t model_record_bytes(uint32_t max_points) { return 128u + 4u * max_points; }

struct ModelArgs { uint8_t *data; const uint8_t *matches; const uint8_t *kept; const uint8_t *current;
                   uint32_t max_points, model, tolerance, max_scale, min_inliers; };

/* a * b + c for |a|, |b| < 2^23, mod 2^32: v_mad_i32_i24, full rate where a 32-bit multiply is not */
__device__ __forceinline__ uint32_t model_mad24(int a, int b, uint32_t c) { return (uint32_t)__mul24(a, b) + c; }

/* |re|^2 + |im|^2 for |re|, |im| <= 2^30: below 2^61 */
__device__ __forceinline__ unsigned long long model_norm(int re, int im)
{
    return (unsigned long long)((long long)re * re) + (unsigned long long)((long long)im * im);
}

__global__ __launch_bounds__(MODEL_THREADS) void k_point_model(ModelArgs a)
{
    __shared__ int4 s_pair[MODEL_MAX_K];                                    /* (xk, yk, xc, yc) of the usable pairs, in slot order */
    __shared__ uint32_t s_slot[MODEL_MAX_K];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_key, s_hyp;
    __shared__ unsigned long long s_sum[4][MODEL_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, K = a.max_points;
    const uint32_t *mt = reinterpret_cast<const uint32_t *>(a.matches + (size_t)blockIdx.x * matches_record_bytes(K));
    const uint32_t *kp = reinterpret_cast<const uint32_t *>(a.kept + (size_t)blockIdx.x * corner_record_bytes(K));
    const uint32_t *cp = reinterpret_cast<const uint32_t *>(a.current + (size_t)blockIdx.x * corner_record_bytes(K));
    uint32_t *dst = reinterpret_cast<uint32_t *>(a.data + (size_t)blockIdx.x * model_record_bytes(K));
    if (tid == 0u) { s_key = 0u; s_hyp = 0u; }

    /* 1. the pair of slot tid, and the compaction */
    int4 mine = make_int4(0, 0, 0, 0);
    bool usable = false;
    if (tid < K) {
        const uint32_t nk = min(kp[2], K), nc = min(cp[2], K);
        const uint32_t j = mt[8u + 4u * tid], flags = mt[11u + 4u * tid];
        if ((flags & 4u) && j < K && tid < nk && j < nc) {
            mine = make_int4((int)kp[8u + 4u * tid], (int)kp[9u + 4u * tid], (int)cp[8u + 4u * j], (int)cp[9u + 4u * j]);
            usable = (uint32_t)mine.x <= MODEL_COORD_MAX && (uint32_t)mine.y <= MODEL_COORD_MAX &&
                     (uint32_t)mine.z <= MODEL_COORD_MAX && (uint32_t)mine.w <= MODEL_COORD_MAX;
        }
    }
    unsigned long long vote = 0ull;
    if (wave < 4u) {
        vote = __ballot(usable);
        if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(vote);
    }
    __syncthreads();
    const uint32_t n = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (usable) {
        uint32_t at = (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; w++) at += s_wave[w];
        s_pair[at] = mine;
        s_slot[at] = tid;
    }
    __syncthreads();

    /* 2. every hypothesis against every pair */
    uint32_t key = 0u, hyp = 0u;
    if (a.model == MODEL_SIMILARITY) {
        const uint32_t rows = n / 2u;                                       /* ceil((n - 1) / 2) rows of n */
        const unsigned long long S2 = (unsigned long long)a.max_scale * a.max_scale, T2 = (unsigned long long)a.tolerance * a.tolerance;
        for (uint32_t t = tid; t < rows * n; t += MODEL_THREADS) {
            const uint32_t r = t / n, c = t - r * n, first = n - 1u - r;
            uint32_t ia, ib;
            if (c < first) { ia = r; ib = r + 1u + c; }
            else if (2u * r + 2u != n) { ia = n - 2u - r; ib = ia + 1u + (c - first); }
            else continue;                                                  /* the middle row has no partner */
            const int4 A = s_pair[ia], B = s_pair[ib];
            const int Px = B.x - A.x, Py = B.y - A.y, Qx = B.z - A.z, Qy = B.w - A.w;
            if (!(Px | Py) || !(Qx | Qy)) continue;
            const uint32_t PP = (uint32_t)(Px * Px + Py * Py), QQ = (uint32_t)(Qx * Qx + Qy * Qy);         /* < 2^29 */
            if (a.max_scale && (65536ull * QQ > S2 * PP || 65536ull * PP > S2 * QQ)) continue;
            hyp++;
            const unsigned long long bound = T2 * PP;                                                       /* < 2^45 */
            /* re = qx Px - qy Py - px Qx + py Qy - Cre;  im = qx Py + qy Px - py Qx - px Qy - Cim */
            const uint32_t Cre = (uint32_t)(A.z * Px - A.w * Py - A.x * Qx + A.y * Qy), Cim = (uint32_t)(A.z * Py + A.w * Px - A.y * Qx - A.x * Qy);
            uint32_t count = 0u;
#pragma unroll 4
            for (uint32_t i = 0; i < n; i++) {
                const int4 v = s_pair[i];
                const int re = (int)model_mad24(v.z, Px, model_mad24(v.w, -Py, model_mad24(v.x, -Qx, model_mad24(v.y, Qy, 0u - Cre))));
                const int im = (int)model_mad24(v.z, Py, model_mad24(v.w, Px, model_mad24(v.y, -Qx, model_mad24(v.x, -Qy, 0u - Cim))));
                count += model_norm(re, im) <= bound ? 1u : 0u;
            }
            key = max(key, count << 16 | (255u - ia) << 8 | (255u - ib));
        }
    } else {
        const uint32_t T2 = a.tolerance * a.tolerance;
        for (uint32_t ia = tid; ia < n; ia += MODEL_THREADS) {
            const int4 A = s_pair[ia];
            const int tx = A.z - A.x, ty = A.w - A.y;
            hyp++;
            uint32_t count = 0u;
            for (uint32_t i = 0; i < n; i++) {
                const int4 v = s_pair[i];
                const int dx = v.z - v.x - tx, dy = v.w - v.y - ty;                                         /* < 2^15 in magnitude */
                count += (uint32_t)(dx * dx) + (uint32_t)(dy * dy) <= T2 ? 1u : 0u;
            }
            key = max(key, count << 16 | (255u - ia) << 8 | 255u);
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, d));
    hyp = stats_wave_sum(hyp);
    if (lane == 0u) {
        if (key) (void)__hip_atomic_fetch_max(&s_key, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (hyp) region_lds_add(&s_hyp, hyp);
    }
    __syncthreads();

    /* 3. the winner: flags, sums, header */
    key = s_key;
    const uint32_t best = key >> 16, ia = 255u - (key >> 8 & 255u), ib = 255u - (key & 255u);
    const bool found = key != 0u && best >= a.min_inliers;
    bool inlier = false;
    if (found && usable) {
        const int4 A = s_pair[ia];
        if (a.model == MODEL_SIMILARITY) {
            const int4 B = s_pair[ib];
            const int Px = B.x - A.x, Py = B.y - A.y, Qx = B.z - A.z, Qy = B.w - A.w;
            const int dpx = mine.x - A.x, dpy = mine.y - A.y, dqx = mine.z - A.z, dqy = mine.w - A.w;
            const int re = (dqx * Px - dqy * Py) - (Qx * dpx - Qy * dpy), im = (dqx * Py + dqy * Px) - (Qx * dpy + Qy * dpx);
            inlier = model_norm(re, im) <= (unsigned long long)(a.tolerance * a.tolerance) * (uint32_t)(Px * Px + Py * Py);
        } else {
            const int dx = (mine.z - mine.x) - (A.z - A.x), dy = (mine.w - mine.y) - (A.w - A.y);
            inlier = (uint32_t)(dx * dx) + (uint32_t)(dy * dy) <= a.tolerance * a.tolerance;
        }
    }
    if (tid < K) dst[32u + tid] = (usable ? 1u : 0u) | (inlier ? 2u : 0u);
    if (wave < 4u) {
        const uint32_t x = inlier ? (uint32_t)mine.x : 0u, y = inlier ? (uint32_t)mine.y : 0u;
        const uint32_t u = inlier ? (uint32_t)mine.z : 0u, v = inlier ? (uint32_t)mine.w : 0u;
        const uint32_t terms[MODEL_SUMS] = { x, y, u, v, x * x, x * y, y * y, x * u, y * u, x * v, y * v, u * u + v * v };      /* < 2^29 */
#pragma unroll
        for (uint32_t k = 0; k < MODEL_SUMS; k++) {
            const unsigned long long s = stats_wave_sum((unsigned long long)terms[k]);
            if (lane == 0u) s_sum[wave][k] = s;
        }
    }
    __syncthreads();
    if (tid < MODEL_SUMS) {                                                 /* a record is 4-byte aligned only: two stores a sum */
        const unsigned long long s = s_sum[0][tid] + s_sum[1][tid] + s_sum[2][tid] + s_sum[3][tid];
        dst[8u + 2u * tid] = (uint32_t)s;
        dst[9u + 2u * tid] = (uint32_t)(s >> 32);
    }
    if (tid == 0u) {
        dst[0] = n;
        dst[1] = s_hyp;
        dst[2] = found ? best : 0u;
        dst[3] = found ? 1u : 0u;
        dst[4] = found ? s_slot[ia] : 0xFFFFFFFFu;
        dst[5] = found && a.model == MODEL_SIMILARITY ? s_slot[ib] : 0xFFFFFFFFu;
        dst[6] = 0u;
        dst[7] = 0u;
    }
}

} // namespace h264k
