/* kernels/k_tensor_out.hip.h — k_tensor_out / k_tensor_resize: the next pictures of many decoder instances into ONE dense
 * caller-owned tensor (h264bsdmiNextOutputTensorBatch[Colour]), one launch per call, grid.y = one item per picture — and the pieces
 * the other tensor headers share, one definition each: the item and the element encoders, the window's chroma (TcWin), the colour of
 * a sample (tc_pixel), the 8-sample segment (tc_chroma_seg, tc_seg) and the 2 x 2 blend (tc_blend).  Included by engine.hip AFTER
 * kernels.hip.h (whose helpers it uses: luma_at, chroma_at, yuv_pixel) and BEFORE k_tensor_aa.hip.h, k_tensor_roi.hip.h and
 * k_tensor_remap.hip.h, in that order; not part of the kernel sources that key the committed counter tables (srchash.py).
 *
 * Colour: per source pixel and output channel c, v = med3(k[c][0] Y + k[c][3] + k[c][1] (Cb - 128) + k[c][2] (Cr - 128), lo[c], hi[c])
 * in fp32 on the 8-bit samples (Cb, Cr upsampled first when bilinear; centred, and luma first, so that no intermediate holds a large
 * offset that the result cancels: f16 outputs near 0 need the absolute precision).  The host folds the range, the matrix of the
 * picture, the clamp to [0, 1] and the output's scale (255 for U8, (. - mean[c]) / std[c] for floats) into the item (engine.hip,
 * colour_item).  U8 writes rint(v), floats v (f16 rounded to nearest even); alpha is 255 / 1.0.  Since the output scale is affine,
 * resizing interpolates v itself.
 * Bilinear chroma (chroma_sample_loc_type 0): luma (x, y) takes chroma at (x / 2, y / 2 - 1/4): rows weighted 3/4 (its own) and 1/4
 * (the one above for even y, below for odd y), columns 1 (even x) or 1/2 + 1/2 (odd x), neighbours clamped to the chroma of the
 * source window; every weight is a multiple of 1/8, so the upsampled sample is exact in fp32.
 *
 * REF, the reference's conversion (src/h264bsd_decoder.c:1163-1370): integer BT.601 limited range, nearest chroma, to 8-bit R, G, B
 * (CH_Y: the luma byte).  The resize path takes those bytes from the item's map, which holds the reference's coefficients / 256 with
 * its rounding term and bounds [0, 255], so that v truncated is exactly the reference's byte; without resize yuv_pixel's integer
 * arithmetic gives the same bytes in fewer instructions (the channel order is the item's bgr).  Float outputs are
 * (b / 255 - mean[c]) / std[c] of the 8-bit value b (a 256-entry table per channel in LDS, no resize); the resize path interpolates
 * the 8-bit values in fp32 with the source coordinates of torch.nn.functional.interpolate(mode="bilinear", align_corners=False,
 * antialias=False). */
#pragma once
namespace h264k {

/* one picture of a call, staged in pinned host memory and read through its device alias (like H2dItem): source frame, destination,
 * window, and the colour map of its output channels */
struct TensorItem { const uint8_t *src; uint8_t *dst; uint32_t wmb, x0, y0, w, h, bgr; float k[3][4]; float lo[3], hi[3]; };  /* bgr: REF only */
struct TensorArgs { const TensorItem *items; uint32_t width, height, chroma; float mean[3], std[3]; };     /* mean / std: REF only */

enum { TO_U8 = 0, TO_F16 = 1, TO_F32 = 2 };
enum { TO_NCHW = 0, TO_NHWC = 1 };
enum { TO_RGB = 0, TO_BGR = 1, TO_RGBA = 2, TO_BGRA = 3, TO_Y = 4 };
enum { TC_NEAREST = 0, TC_BILINEAR = 1 };

template <int DT> struct ToElem { typedef uint32_t T; };
template <> struct ToElem<TO_U8> { typedef uint8_t T; };
template <> struct ToElem<TO_F16> { typedef uint16_t T; };

template <int C> constexpr int tc_nc() { return C == 1 ? 1 : 3; }
constexpr int TO_SEG = 8;       /* output pixels per lane and row in k_tensor_out */

template <int DT> __device__ __forceinline__ typename ToElem<DT>::T to_enc(float f)
{
    if constexpr (DT == TO_F16) return __builtin_bit_cast(uint16_t, (_Float16)f);      /* round to nearest even */
    else return __float_as_uint(f);
}

/* N elements of one output row: whole 16-byte (or 8-byte) stores when the segment is complete and aligned, else one element at a time */
template <typename E, int N> __device__ __forceinline__ void to_store(E *p, const E *v, uint32_t valid, bool vec)
{
    constexpr int bytes = N * (int)sizeof(E);
    if (vec && valid == (uint32_t)N) {
        if constexpr (bytes % 16 == 0) {
#pragma unroll
            for (int i = 0; i < bytes / 16; i++) {
                uint4 q;
                __builtin_memcpy(&q, reinterpret_cast<const char *>(v) + 16 * i, 16);
                reinterpret_cast<uint4 *>(p)[i] = q;
            }
        } else {
#pragma unroll
            for (int i = 0; i < bytes / 8; i++) {
                uint2 q;
                __builtin_memcpy(&q, reinterpret_cast<const char *>(v) + 8 * i, 8);
                reinterpret_cast<uint2 *>(p)[i] = q;
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < N; k++)
        if ((uint32_t)k < valid) p[k] = v[k];
}

__device__ __forceinline__ float tc_value(const TensorItem &it, int c, float y, float cb, float cr)
{
    return __builtin_amdgcn_fmed3f(fmaf(it.k[c][2], cr, fmaf(it.k[c][1], cb, fmaf(it.k[c][0], y, it.k[c][3]))), it.lo[c], it.hi[c]);
}

template <int DT> __device__ __forceinline__ typename ToElem<DT>::T tc_enc(float v)
{
    if constexpr (DT == TO_U8) return (uint8_t)(uint32_t)__builtin_rintf(v);
    else return to_enc<DT>(v);
}
template <int DT> __device__ __forceinline__ typename ToElem<DT>::T tc_alpha()
{
    if constexpr (DT == TO_U8) return 255;
    else return to_enc<DT>(1.0f);
}

/* chroma columns cx .. cx + 7 of row cy of one plane (byte k = column cx + k): word loads, two when cx is a multiple of 4, three
 * otherwise; words beyond the coded chroma width ccw read as 0 */
__device__ __forceinline__ unsigned long long tc_chroma8(const uint8_t *__restrict__ src, int wmb, int plane, uint32_t cx, uint32_t cy, uint32_t ccw)
{
    const uint32_t cxa = cx & ~3u, cs = (cx & 3u) * 8u;
    unsigned long long v = *reinterpret_cast<const uint32_t *>(src + chroma_at(wmb, plane, (int)cxa, (int)cy));
    if (cxa + 4u < ccw) v |= (unsigned long long)*reinterpret_cast<const uint32_t *>(src + chroma_at(wmb, plane, (int)cxa + 4, (int)cy)) << 32;
    if (cs) {
        const unsigned long long w2 = cxa + 8u < ccw ? *reinterpret_cast<const uint32_t *>(src + chroma_at(wmb, plane, (int)cxa + 8, (int)cy)) : 0u;
        v = (v >> cs) | (w2 << (64u - cs));
    }
    return v;
}

/* the chroma of the 8 luma samples sx .. sx + 7 (sx even) of row sy, one plane, minus 128: nearest, or bilinear with the neighbour row
 * nb and the window's last chroma column chi */
__device__ __forceinline__ void tc_chroma_seg(float *out, const uint8_t *__restrict__ src, int wmb, int plane, uint32_t sx, uint32_t sy,
                                              uint32_t ccw, bool bil, uint32_t nb, uint32_t chi)
{
    const uint32_t cx = sx >> 1;
    const unsigned long long row = tc_chroma8(src, wmb, plane, cx, sy >> 1, ccw);
    if (!bil) {
#pragma unroll
        for (int k = 0; k < TO_SEG; k++) out[k] = (float)(uint32_t)((row >> (8 * (k >> 1))) & 255u) - 128.0f;
        return;
    }
    const unsigned long long nbr = tc_chroma8(src, wmb, plane, cx, nb, ccw);
    float v[TO_SEG / 2 + 1];
#pragma unroll
    for (int j = 0; j <= TO_SEG / 2; j++) {
        v[j] = fmaf(0.25f, (float)(uint32_t)((nbr >> (8 * j)) & 255u), 0.75f * (float)(uint32_t)((row >> (8 * j)) & 255u));
        if (j && cx + (uint32_t)j > chi) v[j] = v[j - 1];          /* right edge of the window (only column chi + 1 is read by a valid pixel) */
    }
#pragma unroll
    for (int k = 0; k < TO_SEG; k++) out[k] = ((k & 1) ? 0.5f * (v[k >> 1] + v[(k >> 1) + 1]) : v[k >> 1]) - 128.0f;
}

/* The chroma of a picture's source window, once per kernel: bil (bilinear upsampling; never for REF), the window's last chroma column
 * chi and its first and last chroma rows rlo, rhi (what the neighbours of the bilinear chroma are clamped to), and the coded chroma
 * width ccw */
struct TcWin {
    bool bil;
    uint32_t chi, rlo, rhi, ccw;
    /* the neighbour chroma row of luma row sy: the one above for even sy, below for odd sy, inside the window */
    __device__ __forceinline__ uint32_t nb(uint32_t sy) const
    {
        const uint32_t cy = sy >> 1;
        return (sy & 1u) ? min(cy + 1u, rhi) : max(cy, rlo + 1u) - 1u;
    }
};
template <bool REF> __device__ __forceinline__ TcWin tc_win(const TensorItem &it, uint32_t chroma)
{
    return TcWin{ !REF && chroma == TC_BILINEAR, (it.x0 + it.w) / 2u - 1u, it.y0 / 2u, (it.y0 + it.h) / 2u - 1u, it.wmb * 8u };
}

/* the colour of one sample (y, cb, cr: luma and chroma minus 128) into p[0 .. NC); REF: the 8-bit values */
template <int NC, bool REF> __device__ __forceinline__ void tc_pixel(float *p, const TensorItem &it, float y, float cb, float cr)
{
    if constexpr (NC == 1) p[0] = __builtin_amdgcn_fmed3f(fmaf(it.k[0][0], y, it.k[0][3]), it.lo[0], it.hi[0]);
    else {
#pragma unroll
        for (int c = 0; c < 3; c++) p[c] = tc_value(it, c, y, cb, cr);
    }
    if constexpr (REF) {
#pragma unroll
        for (int c = 0; c < NC; c++) p[c] = __builtin_truncf(p[c]);
    }
}

/* the 8 luma samples yv (byte k = column sx + k, sx even) of row sy with their chroma (word loads, tc_chroma_seg) converted by
 * tc_pixel: put(k, p) receives sample k's p[0 .. NC) */
template <int NC, bool REF, typename Put>
__device__ __forceinline__ void tc_seg(const TensorItem &it, int wmb, const TcWin &w, unsigned long long yv, uint32_t sx, uint32_t sy, Put &&put)
{
    float cb[TO_SEG] = {}, cr[TO_SEG] = {};     /* (NC == 1: not read by tc_pixel, but passed to it) */
    if constexpr (NC == 3) {
        const uint32_t nb = w.nb(sy);
        tc_chroma_seg(cb, it.src, wmb, 0, sx, sy, w.ccw, w.bil, nb, w.chi);
        tc_chroma_seg(cr, it.src, wmb, 1, sx, sy, w.ccw, w.bil, nb, w.chi);
    }
#pragma unroll
    for (int k = 0; k < TO_SEG; k++) {
        float p[NC];
        tc_pixel<NC, REF>(p, it, (float)(uint32_t)((yv >> (8 * k)) & 255u), cb[k], cr[k]);
        put(k, p);
    }
}

/* the 2 x 2 blend of the resampling kernels with the weights lx, ly of the second column and row: a + l (b - a), which keeps equal
 * neighbours exact; REF as the reference path has it: hy (hx v00 + lx v01) + ly (hx v10 + lx v11) with three FMAs in a fixed order */
template <bool REF> __device__ __forceinline__ float tc_blend(float v00, float v01, float v10, float v11, float lx, float ly)
{
    if constexpr (REF) {
#pragma clang fp contract(off)
        const float hx = 1.0f - lx, hy = 1.0f - ly;
        return fmaf(hy, fmaf(hx, v00, lx * v01), ly * fmaf(hx, v10, lx * v11));
    } else {
        const float top = fmaf(lx, v01 - v00, v00), bot = fmaf(lx, v11 - v10, v10);
        return fmaf(ly, bot - top, top);
    }
}

/* No resize: the output is the source window pixel for pixel.  A wavefront covers 64 output columns x 16 rows in two passes of 8 rows; a
 * lane takes 8 horizontally adjacent pixels of one row: ONE 8-byte luma load when the window starts on a multiple of 8 columns (the two
 * rows of a chroma row pair are in the same pass), two otherwise (funnel shift).  Chroma: 2 word loads per plane and row when the window
 * starts on a multiple of 8 columns, 3 otherwise; bilinear loads the neighbour row as well; REF loads 1 word per plane, 2 when not
 * aligned.  Stores: NCHW one 8-pixel piece per plane (f16: 16 bytes; a pass of a wavefront writes 8 rows x 128 bytes per plane), NHWC
 * 8 * C elements; the ragged right edge (window width not a multiple of 8) and unaligned rows go element by element in the same launch.
 * REF floats look the 8-bit value up in the table. */
template <int DT, int LAYOUT, int C, bool REF>
__global__ __launch_bounds__(256) void k_tensor_out(TensorArgs a)
{
    constexpr int NC = tc_nc<C>();
    typedef typename ToElem<DT>::T E;
    __shared__ float lut[NC][256];
    if constexpr (REF && DT != TO_U8) {
#pragma unroll
        for (int c = 0; c < NC; c++) lut[c][threadIdx.x] = ((float)threadIdx.x / 255.0f - a.mean[c]) / a.std[c];
        __syncthreads();
    }
    const TensorItem it = a.items[blockIdx.y];
    const uint32_t W = a.width, H = a.height, cw = it.wmb * 16u;
    const int wmb = (int)it.wmb;
    const TcWin win = tc_win<REF>(it, a.chroma);
    const uint32_t nux = (W + 63u) / 64u, units = nux * ((H + 15u) / 16u);
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t seg = lane & 7u, r = lane >> 3;
    const bool vec = (W % TO_SEG) == 0 && (reinterpret_cast<uintptr_t>(it.dst) & 15u) == 0;
    const size_t plane = (size_t)W * H;
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t u = blockIdx.x * 4u + wave; u < units; u += gridDim.x * 4u) {
        const uint32_t ox = (u % nux) * 64u + seg * TO_SEG;
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const uint32_t oy = (u / nux) * 16u + pass * 8u + r;
            if (ox >= W || oy >= H) continue;
            const uint32_t valid = min((uint32_t)TO_SEG, W - ox);
            const uint32_t sx = it.x0 + ox, sy = it.y0 + oy;
            const uint32_t sxa = sx & ~7u, ls = (sx & 7u) * 8u;
            unsigned long long yv = *reinterpret_cast<const unsigned long long *>(it.src + luma_at(wmb, (int)sxa, (int)sy));
            if (ls) {
                const unsigned long long hi = sxa + 8u < cw ? *reinterpret_cast<const unsigned long long *>(it.src + luma_at(wmb, (int)sxa + 8, (int)sy)) : 0ull;
                yv = (yv >> ls) | (hi << (64u - ls));
            }
            float cb[TO_SEG], cr[TO_SEG];
            unsigned long long cbw = 0, crw = 0;        /* REF: chroma columns sx / 2 .. sx / 2 + 3 */
            if constexpr (NC == 3 && REF) {
                const uint32_t cx = sx >> 1, cy = sy >> 1, cxa = cx & ~3u, cs = (cx & 3u) * 8u;
                cbw = *reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 0, (int)cxa, (int)cy));
                crw = *reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 1, (int)cxa, (int)cy));
                if (cs) {
                    if (cxa + 4u < (cw >> 1)) {
                        cbw |= (unsigned long long)*reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 0, (int)cxa + 4, (int)cy)) << 32;
                        crw |= (unsigned long long)*reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 1, (int)cxa + 4, (int)cy)) << 32;
                    }
                    cbw >>= cs; crw >>= cs;
                }
            } else if constexpr (NC == 3) {
                const uint32_t nb = win.nb(sy);
                tc_chroma_seg(cb, it.src, wmb, 0, sx, sy, cw >> 1, win.bil, nb, win.chi);
                tc_chroma_seg(cr, it.src, wmb, 1, sx, sy, cw >> 1, win.bil, nb, win.chi);
            }
            E v[TO_SEG * C];
#pragma unroll
            for (int k = 0; k < TO_SEG; k++) {
                const uint32_t Yv = (uint32_t)(yv >> (8 * k)) & 255u;
                const float y = (float)Yv;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    E e;
                    if (c == 3) e = tc_alpha<DT>();
                    else if constexpr (REF) {
                        uint32_t b = Yv;
                        if constexpr (NC == 3) {
                            const uint32_t rgb = yuv_pixel(0, (int)Yv, (int)((cbw >> (8 * (k >> 1))) & 255u), (int)((crw >> (8 * (k >> 1))) & 255u));
                            b = c == 1 ? (rgb >> 8) & 255u : (c == 0) == !it.bgr ? rgb & 255u : (rgb >> 16) & 255u;
                        }
                        if constexpr (DT == TO_U8) e = (E)b;
                        else e = to_enc<DT>(lut[c][b]);
                    } else if constexpr (NC == 1) {
                        e = tc_enc<DT>(__builtin_amdgcn_fmed3f(fmaf(it.k[0][0], y, it.k[0][3]), it.lo[0], it.hi[0]));
                    } else {
                        e = tc_enc<DT>(tc_value(it, c, y, cb[k], cr[k]));
                    }
                    v[LAYOUT == TO_NCHW ? c * TO_SEG + k : k * C + c] = e;
                }
            }
            if constexpr (LAYOUT == TO_NCHW) {
#pragma unroll
                for (int c = 0; c < C; c++) to_store<E, TO_SEG>(dst + c * plane + (size_t)oy * W + ox, v + c * TO_SEG, valid, vec);
            } else {
                to_store<E, TO_SEG * C>(dst + ((size_t)oy * W + ox) * C, v, valid * C, vec);
            }
        }
    }
}

constexpr int TCR_COLS = 64, TCR_ROWS = 8;      /* output tile of one workgroup and step in k_tensor_resize */

/* torch's bilinear source coordinate (align_corners=False): max((o + 0.5) * scale - 0.5, 0), its integer part i and the weight l of
 * i + 1.  Rounded after every operation (the test model rounds the same way); REF with one FMA, as the reference path has always had. */
template <bool REF> __device__ __forceinline__ void tcr_coord(uint32_t o, float scale, int &i, float &l)
{
#pragma clang fp contract(off)
    const float f = fmaxf(REF ? fmaf((float)o + 0.5f, scale, -0.5f) : ((float)o + 0.5f) * scale - 0.5f, 0.0f);
    i = (int)f;
    l = f - (float)i;
}

/* the colour of source pixel (x, y) of the window (absolute coordinates), into p[0 .. NC); REF: the 8-bit values */
template <int NC, bool REF>
__device__ __forceinline__ void tcr_convert(float *p, const TensorItem &it, int wmb, const TcWin &w, uint32_t x, uint32_t y)
{
    const uint8_t *__restrict__ src = it.src;
    const float Y = (float)src[luma_at(wmb, (int)x, (int)y)];
    float cc[2] = { 0.0f, 0.0f };
    if constexpr (NC == 3) {
        const uint32_t c0 = x >> 1, r0 = y >> 1;
        if (!w.bil) {
#pragma unroll
            for (int q = 0; q < 2; q++) cc[q] = (float)src[chroma_at(wmb, q, (int)c0, (int)r0)];
        } else {
            const uint32_t c1 = min(c0 + (x & 1u), w.chi), r1 = w.nb(y);
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const float a0 = (float)src[chroma_at(wmb, q, (int)c0, (int)r0)], a1 = (float)src[chroma_at(wmb, q, (int)c1, (int)r0)];
                const float b0 = (float)src[chroma_at(wmb, q, (int)c0, (int)r1)], b1 = (float)src[chroma_at(wmb, q, (int)c1, (int)r1)];
                cc[q] = fmaf(0.25f, 0.5f * (b0 + b1), 0.75f * (0.5f * (a0 + a1)));
            }
        }
    }
    tc_pixel<NC, REF>(p, it, Y, cc[0] - 128.0f, cc[1] - 128.0f);
}

/* Resize.  A workgroup takes an output tile of 64 columns x 8 rows at a time.  Phase 1: the tile's 8 x 2 source rows (y0, y1 of each
 * output row) times its 64 x 2 source columns (x0, x1 of each output column) are converted, one source pixel per slot and lane, 8 per
 * lane, into LDS; the loads of the 2048 slots are independent of each other.  Phase 2: each lane interpolates 2 output pixels from LDS
 * (tc_blend; U8 rounds exact halves to even, as the model does, REF halves up) and stores them.  Slots
 * are not shared between neighbouring output rows or columns: when upscaling, a source pixel may be converted once per slot that
 * names it. */
template <int DT, int LAYOUT, int C, bool REF>
__global__ __launch_bounds__(256) void k_tensor_resize(TensorArgs a)
{
    constexpr int NC = tc_nc<C>();
    typedef typename ToElem<DT>::T E;
    __shared__ float lds[2 * TCR_ROWS][2 * TCR_COLS][NC];
    const TensorItem it = a.items[blockIdx.y];
    const uint32_t W = a.width, H = a.height;
    const int wmb = (int)it.wmb;
    const TcWin win = tc_win<REF>(it, a.chroma);
    const float scale_x = (float)it.w / (float)W, scale_y = (float)it.h / (float)H;
    const uint32_t nux = (W + TCR_COLS - 1u) / TCR_COLS, units = nux * ((H + TCR_ROWS - 1u) / TCR_ROWS);
    const size_t plane = (size_t)W * H;
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t tx = (u % nux) * TCR_COLS, ty = (u / nux) * TCR_ROWS;
#pragma unroll
        for (int i = 0; i < 2 * TCR_ROWS * 2 * TCR_COLS / 256; i++) {
            const uint32_t s = threadIdx.x + 256u * i, ra = s / (2 * TCR_COLS), cb = s % (2 * TCR_COLS);
            const uint32_t ox = tx + cb / 2u, oy = ty + ra / 2u;
            if (ox >= W || oy >= H) continue;
            int xi, yi;
            float lx, ly;
            tcr_coord<REF>(ox, scale_x, xi, lx);
            tcr_coord<REF>(oy, scale_y, yi, ly);
            const uint32_t x = (cb & 1u) ? (uint32_t)min(xi + 1, (int)it.w - 1) : (uint32_t)xi;
            const uint32_t y = (ra & 1u) ? (uint32_t)min(yi + 1, (int)it.h - 1) : (uint32_t)yi;
            tcr_convert<NC, REF>(lds[ra][cb], it, wmb, win, it.x0 + x, it.y0 + y);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TCR_ROWS * TCR_COLS / 256; i++) {
            const uint32_t o = threadIdx.x + 256u * i, r = o / TCR_COLS, j = o % TCR_COLS;
            const uint32_t ox = tx + j, oy = ty + r;
            if (ox >= W || oy >= H) continue;
            int xi, yi;
            float lx, ly;
            tcr_coord<REF>(ox, scale_x, xi, lx);
            tcr_coord<REF>(oy, scale_y, yi, ly);
            const size_t pix = (size_t)oy * W + ox;
#pragma unroll
            for (int c = 0; c < C; c++) {
                E e;
                if (c == 3) e = tc_alpha<DT>();
                else {
                    const float v = tc_blend<REF>(lds[2 * r][2 * j][c], lds[2 * r][2 * j + 1][c], lds[2 * r + 1][2 * j][c],
                                                  lds[2 * r + 1][2 * j + 1][c], lx, ly);
                    if constexpr (!REF) e = tc_enc<DT>(v);
                    else if constexpr (DT == TO_U8) e = (E)min(255, (int)(v + 0.5f));     /* (not the shared tail's fmed3 form) */
                    else e = to_enc<DT>((v / 255.0f - a.mean[c]) / a.std[c]);
                }
                if constexpr (LAYOUT == TO_NCHW) dst[c * plane + pix] = e;
                else dst[pix * C + c] = e;
            }
        }
        __syncthreads();
    }
}

} // namespace h264k
