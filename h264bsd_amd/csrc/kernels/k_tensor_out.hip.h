/* kernels/k_tensor_out.hip.h — k_tensor_out / k_tensor_resize: the next pictures of many decoder instances into ONE dense
 * caller-owned tensor (h264bsdmiNextOutputTensorBatch), one launch per call, grid.y = one item per picture.
 * Included by engine.hip AFTER kernels.hip.h (whose helpers it uses: luma_at, chroma_at, yuv_pixel); not part of the kernel
 * sources that key the committed counter tables (srchash.py).
 *
 * Colour is the reference's (src/h264bsd_decoder.c:1163-1370, yuv_pixel): integer BT.601 limited range, nearest chroma, per
 * SOURCE pixel, to 8-bit R, G, B; CH_Y is the luma byte itself.  Float outputs are (v / 255 - mean[c]) / std[c] in fp32 (c = the
 * output channel), fp16 rounded to nearest even; the resize path is bilinear on the 8-bit values in fp32, with the source
 * coordinates of torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False). */
#pragma once
namespace h264k {

/* one picture of a call, staged in pinned host memory and read through its device alias (like H2dItem) */
struct TensorItem { const uint8_t *src; uint8_t *dst; uint32_t wmb, x0, y0, w, h, pad; };
struct TensorArgs { const TensorItem *items; uint32_t width, height; float mean[3], std[3]; };

enum { TO_U8 = 0, TO_F16 = 1, TO_F32 = 2 };
enum { TO_NCHW = 0, TO_NHWC = 1 };
enum { TO_RGB = 0, TO_BGR = 1, TO_RGBA = 2, TO_BGRA = 3, TO_Y = 4 };

template <int DT> struct ToElem { typedef uint32_t T; };
template <> struct ToElem<TO_U8> { typedef uint8_t T; };
template <> struct ToElem<TO_F16> { typedef uint16_t T; };

constexpr int to_channels(int ch) { return ch == TO_Y ? 1 : ch >= TO_RGBA ? 4 : 3; }

/* byte of output channel c (0..2) of a yuv_pixel(0, ...) word (R in bits 0-7, G 8-15, B 16-23) */
template <int CH> __device__ __forceinline__ uint32_t to_pick(uint32_t rgba, int c)
{
    const int k = (CH == TO_BGR || CH == TO_BGRA) ? 2 - c : c;
    return (rgba >> (8 * k)) & 255u;
}

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

constexpr int TO_SEG = 8;       /* output pixels per lane and row in k_tensor_out */

/* No resize: the output is the source window pixel for pixel.  A wavefront covers 64 output columns x 16 rows in two passes of
 * 8 rows; a lane takes 8 horizontally adjacent pixels of one row: ONE 8-byte luma load and one 4-byte load per chroma plane when the
 * window starts on a multiple of 8 columns (the two rows of a chroma row pair are in the same pass, so every byte of a tile is
 * fetched by one instruction), two of each otherwise (even offsets: funnel shift).  Values come from a 256-entry table per channel
 * in LDS, so the normalisation costs a lookup and is exactly the fp32 formula.  Stores: NCHW one 8-pixel piece per plane (f16: 16
 * bytes; a pass of a wavefront writes 8 rows x 128 bytes per plane), NHWC 8 * C elements; the ragged right edge (window width not a
 * multiple of 8) and unaligned rows go element by element in the same launch. */
template <int DT, int LAYOUT, int CH>
__global__ __launch_bounds__(256) void k_tensor_out(TensorArgs a)
{
    constexpr int C = to_channels(CH), NC = CH == TO_Y ? 1 : 3;
    typedef typename ToElem<DT>::T E;
    __shared__ float lut[NC][256];
    if constexpr (DT != TO_U8) {
#pragma unroll
        for (int c = 0; c < NC; c++) lut[c][threadIdx.x] = ((float)threadIdx.x / 255.0f - a.mean[c]) / a.std[c];
        __syncthreads();
    }
    const TensorItem it = a.items[blockIdx.y];
    const uint32_t W = a.width, H = a.height, cw = it.wmb * 16u;
    const int wmb = (int)it.wmb;
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
            unsigned long long cb = 0, cr = 0;
            if constexpr (CH != TO_Y) {
                const uint32_t cx = sx >> 1, cy = sy >> 1, cxa = cx & ~3u, cs = (cx & 3u) * 8u;
                cb = *reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 0, (int)cxa, (int)cy));
                cr = *reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 1, (int)cxa, (int)cy));
                if (cs) {
                    if (cxa + 4u < (cw >> 1)) {
                        cb |= (unsigned long long)*reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 0, (int)cxa + 4, (int)cy)) << 32;
                        cr |= (unsigned long long)*reinterpret_cast<const uint32_t *>(it.src + chroma_at(wmb, 1, (int)cxa + 4, (int)cy)) << 32;
                    }
                    cb >>= cs; cr >>= cs;
                }
            }
            E v[TO_SEG * C];
#pragma unroll
            for (int k = 0; k < TO_SEG; k++) {
                const uint32_t Yv = (uint32_t)(yv >> (8 * k)) & 255u;
                uint32_t rgba = 0;
                if constexpr (CH != TO_Y)
                    rgba = yuv_pixel(0, (int)Yv, (int)((cb >> (8 * (k >> 1))) & 255u), (int)((cr >> (8 * (k >> 1))) & 255u));
#pragma unroll
                for (int c = 0; c < C; c++) {
                    E e;
                    if (c == 3) {
                        if constexpr (DT == TO_U8) e = 255; else e = to_enc<DT>(1.0f);
                    } else {
                        const uint32_t b = CH == TO_Y ? Yv : to_pick<CH>(rgba, c);
                        if constexpr (DT == TO_U8) e = (E)b; else e = to_enc<DT>(lut[c][b]);
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

/* source pixel (x, y) of a frame in tiles, as the 8-bit values of the output channels (luma for CH_Y, else a yuv_pixel word) */
template <int CH> __device__ __forceinline__ uint32_t to_src_pixel(const uint8_t *__restrict__ src, int wmb, int x, int y)
{
    const uint32_t Yv = src[luma_at(wmb, x, y)];
    if constexpr (CH == TO_Y) return Yv;
    else return yuv_pixel(0, (int)Yv, src[chroma_at(wmb, 0, x >> 1, y >> 1)], src[chroma_at(wmb, 1, x >> 1, y >> 1)]);
}

/* Resize: one output pixel per lane; four source pixels, each converted, interpolated per channel in fp32 like
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False): scale = src / dst, source coordinate
 * max((o + 0.5) * scale - 0.5, 0), the right / lower neighbour clamped to the window.  Latency-bound at the sizes networks take
 * (1080p -> 224x224: 50 k output pixels per picture); kept plain. */
template <int DT, int LAYOUT, int CH>
__global__ __launch_bounds__(256) void k_tensor_resize(TensorArgs a)
{
    constexpr int C = to_channels(CH), NC = CH == TO_Y ? 1 : 3;
    typedef typename ToElem<DT>::T E;
    const TensorItem it = a.items[blockIdx.y];
    const uint32_t W = a.width, H = a.height, n = W * H;
    const int wmb = (int)it.wmb;
    const float scale_x = (float)it.w / (float)W, scale_y = (float)it.h / (float)H;
    const size_t plane = (size_t)n;
    E *dst = reinterpret_cast<E *>(it.dst);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t ox = i % W, oy = i / W;
        const float fx = fmaxf(((float)ox + 0.5f) * scale_x - 0.5f, 0.0f), fy = fmaxf(((float)oy + 0.5f) * scale_y - 0.5f, 0.0f);
        const int x0 = (int)fx, y0 = (int)fy;
        const int x1 = min(x0 + 1, (int)it.w - 1), y1 = min(y0 + 1, (int)it.h - 1);
        const float lx = fx - (float)x0, ly = fy - (float)y0, hx = 1.0f - lx, hy = 1.0f - ly;
        const int bx = (int)it.x0, by = (int)it.y0;
        const uint32_t p00 = to_src_pixel<CH>(it.src, wmb, bx + x0, by + y0), p01 = to_src_pixel<CH>(it.src, wmb, bx + x1, by + y0);
        const uint32_t p10 = to_src_pixel<CH>(it.src, wmb, bx + x0, by + y1), p11 = to_src_pixel<CH>(it.src, wmb, bx + x1, by + y1);
#pragma unroll
        for (int c = 0; c < C; c++) {
            E e;
            if (c == 3) {
                if constexpr (DT == TO_U8) e = 255; else e = to_enc<DT>(1.0f);
            } else {
                const float v00 = (float)(CH == TO_Y ? p00 : to_pick<CH>(p00, c)), v01 = (float)(CH == TO_Y ? p01 : to_pick<CH>(p01, c));
                const float v10 = (float)(CH == TO_Y ? p10 : to_pick<CH>(p10, c)), v11 = (float)(CH == TO_Y ? p11 : to_pick<CH>(p11, c));
                const float v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
                if constexpr (DT == TO_U8) e = (E)min(255, (int)(v + 0.5f));
                else e = to_enc<DT>((v / 255.0f - a.mean[c < NC ? c : 0]) / a.std[c < NC ? c : 0]);
            }
            if constexpr (LAYOUT == TO_NCHW) dst[c * plane + i] = e;
            else dst[(size_t)i * C + c] = e;
        }
    }
}

} // namespace h264k
