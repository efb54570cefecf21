/* kernels/luma_search.hip.h — what the search and point kernels share: k_region_shift, k_cell_shift, k_corner_points and
 * k_point_describe, which stage luma of kept and current pictures from the macroblock tiles into LDS clamped at the WINDOW, and the two
 * SAD searches among them, which rank displacements by the same rule (their inner loops stay their own: docs/EXPERIMENTS.md).  Included by engine.hip after
 * region_common.hip.h and ahead of k_region_shift.hip.h; like its users, not part of the kernel sources that key the committed counter
 * tables (srchash.py).  Every piece is __forceinline__: what a kernel gets from here is the code it used to carry itself.  The
 * constants of the searches (SHIFT_*, FLOW_*) stay in the kernels' own headers.
 *     LumaWindow, luma_stage                  a window of a frame; rows of its luma into LDS as raster rows of dwords
 *     shift_sad4                              the masked path: four SADs of a template dword of which only some bytes count
 *     shift_field                             one 16-bit field of a packed sum
 *     shift_key, shift_key_dx / _dy / _best   the tie rule of the argmin as ONE 64-bit key, and its decode */
#pragma once
namespace h264k {

/* the window [wx0, wx1) x [wy0, wy1) of a frame of wmb macroblocks per row, in luma samples of the coded frame.  luma_stage takes this,
 * or any item that has these five members (k_region_shift hands it its ShiftItem, which keeps that kernel's code as it was) */
struct LumaWindow { uint32_t wmb, wx0, wy0, wx1, wy1; };

/* rows x cols4 dwords of a frame's luma into LDS as raster rows: byte k of dword j of row i is the sample at
 * (clamp(X0 + 4 j + k, wx0, wx1 - 1), clamp(Y0 + i, wy0, wy1 - 1)).  Every SAMPLE taken is inside the window; the aligned dwords of the
 * fast path may start up to 3 bytes left of wx0 or end up to 3 bytes right of wx1 - 1, but they lie in the 16-byte tile rows of samples of
 * the window, so inside the frame */
template <class Window>
__device__ __forceinline__ void luma_stage(const uint8_t *frame, const Window &w, int X0, int Y0, uint32_t cols4, uint32_t rows,
                                           uint32_t *lds, uint32_t pitch, uint32_t tid)
{
    for (uint32_t i = tid; i < rows * cols4; i += 256u) {
        const uint32_t r = i / cols4, j = i - r * cols4;
        const uint32_t Y = (uint32_t)min(max(Y0 + (int)r, (int)w.wy0), (int)w.wy1 - 1);
        const int X = X0 + 4 * (int)j;
        const uint8_t *row = frame + (size_t)(Y >> 4) * w.wmb * TILE + (Y & 15u) * 16u;
        uint32_t v;
        if (X >= (int)w.wx0 && X + 3 < (int)w.wx1) {
            const uint32_t xa = (uint32_t)X & ~3u, sh = (uint32_t)X & 3u, xb = sh ? xa + 4u : xa;       /* xb <= X + 3: inside as well */
            const uint32_t lo = *reinterpret_cast<const uint32_t *>(row + (size_t)(xa >> 4) * TILE + (xa & 15u));
            const uint32_t hi = *reinterpret_cast<const uint32_t *>(row + (size_t)(xb >> 4) * TILE + (xb & 15u));
            v = __builtin_amdgcn_alignbyte(hi, lo, sh);
        } else {
            v = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x = (uint32_t)min(max(X + k, (int)w.wx0), (int)w.wx1 - 1);
                v |= (uint32_t)row[(size_t)(x >> 4) * TILE + (x & 15u)] << (8 * k);
            }
        }
        lds[r * pitch + j] = v;
    }
}

/* the four SADs of template dword t against the bytes k .. k + 3 of c1:c0, k = 0 .. 3, bytes outside m left out, added to sum[] */
__device__ __forceinline__ void shift_sad4(uint32_t c0, uint32_t c1, uint32_t t, uint32_t m, uint32_t *sum)
{
#pragma unroll
    for (int k = 0; k < 4; k++) sum[k] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(c1, c0, (uint32_t)k) & m, t & m, sum[k]);
}

/* field k of a packed sum: the SAD of the k-th of a quad's four displacements since the sum was last cleared */
__device__ __forceinline__ uint32_t shift_field(unsigned long long acc, uint32_t k) { return (uint32_t)(acc >> (16u * k)) & 0xFFFFu; }

/* The tie rule of the argmin: the smallest SAD, then the smallest dx^2 + dy^2, then the smallest dy, then the smallest dx, as the
 * minimum of ONE 64-bit key per displacement (dxi, dyi) = (dx + R, dy + R), both below 64 and dx^2 + dy^2 <= 512 < 2^20 */
__device__ __forceinline__ unsigned long long shift_key(uint32_t sad, uint32_t dxi, uint32_t dyi, uint32_t R)
{
    const int dx = (int)dxi - (int)R, dy = (int)dyi - (int)R;
    return (unsigned long long)sad << 32 | (unsigned long long)(uint32_t)(dx * dx + dy * dy) << 12 | dyi << 6 | dxi;
}
__device__ __forceinline__ uint32_t shift_key_dx(unsigned long long key, uint32_t R) { return (uint32_t)((int)(key & 63u) - (int)R); }
__device__ __forceinline__ uint32_t shift_key_dy(unsigned long long key, uint32_t R) { return (uint32_t)((int)((key >> 6) & 63u) - (int)R); }
__device__ __forceinline__ uint32_t shift_key_best(unsigned long long key) { return (uint32_t)(key >> 32); }

} // namespace h264k
