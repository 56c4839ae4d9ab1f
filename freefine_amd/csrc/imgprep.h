// Device image preparation of the feature metrics (FID-DINO, Kernel Distance, Background / Subject Consistency): from the decoded uint8 image to the operand rows
// of the patch-embedding GEMM.
//
//   resize_h_kernel / resize_v_kernel   PIL's Image.resize(BILINEAR) on 8-bit images restated: two separable passes in int32 with 22-bit fixed-point
//                                       coefficients (PIL libImaging/Resample.c: ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc,
//                                       PRECISION_BITS = 32 - 8 - 2).  The coefficient tables are built on the host (ops.pil_bilinear_coeffs); the kernels only
//                                       multiply, add, shift and clamp, so the result does not depend on the compiler's floating point.
//   resize_win_h_kernel / _v_kernel     the same passes for any PIL filter's tables, 1 or 3 channels, a destination crop window and a keep mask (below)
//   patch_rows_kernel                   ToTensor + Normalize as a [3][256] lookup (evaluated on the host by torch) and the im2col of a ViT patch embedding
//                                       (Conv2d(kernel = stride = patch)): one row per patch, columns (channel, ky, kx), zero padding up to ldo.
//   patch_rows_pair_kernel              the same rows as the split-bf16 PAIR operand of an FFN_BF16X3 GEMM (hi = bf16(v), lo = bf16(v - hi); layout: common.h
//                                       pair_pos): what patch_rows_kernel<float> + split_pair8_kernel write, bit for bit, without the fp32 rows in between.
//
// Traffic is small (a 512 x 512 image is 768 KB in, 147 KB out), so the kernels are plain: byte loads that are contiguous across a workgroup's threads
// (bytes along an image row are contiguous over (x, c)), no vector loads (an image row starts at any byte address).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/freefine_hip.h"
#include "common.h"

// largest side of a source or destination image: one source row (3 * IMGPREP_MAX_SIDE bytes) is staged in LDS by the horizontal pass
#define IMGPREP_MAX_SIDE FFN_IMGPREP_MAX_SIDE
#define IMGPREP_THREADS 256

__device__ __forceinline__ uint8_t imgprep_clip8(int acc) {
    acc >>= 22;
    return (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// Horizontal pass: src [B][H][W][3] -> dst [B][H][ow][3].  One workgroup per source row (grid = (H, B)): the row is staged in LDS, then one thread per
// output byte (xx, c).  bounds [ow][2] = (xmin, n), coef [ow][ksize].  (xmin, n) are clamped into the row: a bad table cannot make the kernel read outside it.
__global__ __launch_bounds__(IMGPREP_THREADS) void resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int ow,
                                                                   const int* __restrict__ bounds, const int* __restrict__ coef, int ksize) {
    __shared__ uint8_t row[3 * IMGPREP_MAX_SIDE];
    const long r = (long)blockIdx.y * gridDim.x + blockIdx.x;              // row index over (b, y)
    const uint8_t* s = src + r * W * 3;
    for (int i = threadIdx.x; i < W * 3; i += IMGPREP_THREADS) row[i] = s[i];
    __syncthreads();
    uint8_t* d = dst + r * ow * 3;
    for (int o = threadIdx.x; o < ow * 3; o += IMGPREP_THREADS) {
        const int xx = o / 3, c = o - 3 * xx;
        int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
        xmin = xmin < 0 ? 0 : (xmin > W - 1 ? W - 1 : xmin);
        n = n > ksize ? ksize : n;
        n = n > W - xmin ? W - xmin : n;
        const int* k = coef + (long)xx * ksize;
        int acc = 1 << 21;
        for (int x = 0; x < n; ++x) acc += (int)row[(xmin + x) * 3 + c] * k[x];
        d[o] = imgprep_clip8(acc);
    }
}

// Vertical pass: src [B][H][ow][3] -> dst [B][oh][ow][3].  One workgroup per output row and 256 consecutive bytes of it (grid = (ceil(3 ow / 256), oh, B)):
// the row's coefficients are the same for the whole workgroup, every source row is read with contiguous bytes.
__global__ __launch_bounds__(IMGPREP_THREADS) void resize_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int oh, int row_bytes,
                                                                   const int* __restrict__ bounds, const int* __restrict__ coef, int ksize) {
    const int o = blockIdx.x * IMGPREP_THREADS + threadIdx.x;
    if (o >= row_bytes) return;
    const int yy = blockIdx.y;
    int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    ymin = ymin < 0 ? 0 : (ymin > H - 1 ? H - 1 : ymin);
    n = n > ksize ? ksize : n;
    n = n > H - ymin ? H - ymin : n;
    const int* k = coef + (long)yy * ksize;
    const uint8_t* s = src + ((long)blockIdx.z * H + ymin) * row_bytes + o;
    int acc = 1 << 21;
    for (int y = 0; y < n; ++y) acc += (int)s[(long)y * row_bytes] * k[y];
    dst[((long)blockIdx.z * oh + yy) * row_bytes + o] = imgprep_clip8(acc);
}

// ---- the general PIL resize (ffn_resize_pil_u8): any filter's tables (signed coefficients, any width up to FFN_IMGPREP_MAX_TAPS), C = 1 or 3 channels, a
// destination crop window (y0, x0, ch, cw) inside oh x ow, and an optional keep mask applied while the source row is staged in LDS -- the masked image of the
// consistency metrics (Background / Subject Consistency) never exists in memory.  Same arithmetic as the two bilinear kernels above; the sum is kept in
// uint32 (two's complement: the same bits as PIL's int) so that a bad table wraps instead of overflowing a signed int.

// keep rule of one pixel: SUM_LT128 = (uint8)(m1 + m2) < 128 (the reference's uint8 wrap: 200 + 100 = 44 keeps, 128 + 128 = 0 keeps), GT128 = m1 > 128
__device__ __forceinline__ bool imgprep_keep(int rule, const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2, long i) {
    if (rule == FFN_KEEP_SUM_LT128) return (uint8_t)((unsigned)m1[i] + (m2 ? (unsigned)m2[i] : 0u)) < 128;
    if (rule == FFN_KEEP_GT128) return m1[i] > 128;
    return true;
}

// Horizontal pass: src [B][H][W][C] -> dst [B][H][cw][C], only the window's columns x0 .. x0 + cw - 1 of the ow the tables describe.  One workgroup per source
// row (grid = (H, B)); the row is staged in LDS with dropped pixels as 0 in all channels (m1 / m2 [B][H][W], rule FFN_KEEP_*), then one thread per output byte.
template <int C>
__global__ __launch_bounds__(IMGPREP_THREADS) void resize_win_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ m1,
                                                                       const uint8_t* __restrict__ m2, int rule, int W, int x0, int cw,
                                                                       const int* __restrict__ bounds, const int* __restrict__ coef, int ksize) {
    __shared__ uint8_t row[3 * IMGPREP_MAX_SIDE];
    const long r = (long)blockIdx.y * gridDim.x + blockIdx.x;              // row index over (b, y)
    const uint8_t* s = src + r * W * C;
    for (int i = threadIdx.x; i < W * C; i += IMGPREP_THREADS) row[i] = imgprep_keep(rule, m1, m2, r * W + i / C) ? s[i] : (uint8_t)0;
    __syncthreads();
    uint8_t* d = dst + r * cw * C;
    for (int o = threadIdx.x; o < cw * C; o += IMGPREP_THREADS) {
        const int j = o / C, c = o - C * j, xx = x0 + j;
        int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
        xmin = xmin < 0 ? 0 : (xmin > W - 1 ? W - 1 : xmin);
        n = n > ksize ? ksize : n;
        n = n > W - xmin ? W - xmin : n;
        const int* k = coef + (long)xx * ksize;
        unsigned acc = 1u << 21;
        for (int x = 0; x < n; ++x) acc += (unsigned)row[(xmin + x) * C + c] * (unsigned)k[x];
        d[o] = imgprep_clip8((int)acc);
    }
}

// Vertical pass: src [B][H][cw][C] -> dst [B][ch][cw][C], only the window's rows y0 .. y0 + ch - 1.  grid = (ceil(row_bytes / 256), ch, B), row_bytes = cw C.
__global__ __launch_bounds__(IMGPREP_THREADS) void resize_win_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int y0, int ch, int row_bytes,
                                                                       const int* __restrict__ bounds, const int* __restrict__ coef, int ksize) {
    const int o = blockIdx.x * IMGPREP_THREADS + threadIdx.x;
    if (o >= row_bytes) return;
    const int yy = y0 + blockIdx.y;
    int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    ymin = ymin < 0 ? 0 : (ymin > H - 1 ? H - 1 : ymin);
    n = n > ksize ? ksize : n;
    n = n > H - ymin ? H - ymin : n;
    const int* k = coef + (long)yy * ksize;
    const uint8_t* s = src + ((long)blockIdx.z * H + ymin) * row_bytes + o;
    unsigned acc = 1u << 21;
    for (int y = 0; y < n; ++y) acc += (unsigned)s[(long)y * row_bytes] * (unsigned)k[y];
    dst[((long)blockIdx.z * ch + blockIdx.y) * row_bytes + o] = imgprep_clip8((int)acc);
}

// Patch rows: src [B][H][W][3] uint8 -> out [B * (H / ps) * (W / ps)][ldo] of T; column j = (c, ky, kx) holds lut[c][src[b][py ps + ky][px ps + kx][c]],
// columns 3 ps ps .. ldo - 1 are zero.  One thread per output element (grid-stride): the writes of a workgroup are contiguous.
template <typename T>
__global__ __launch_bounds__(IMGPREP_THREADS) void patch_rows_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut, T* __restrict__ out, long total,
                                                                     int H, int W, int ps, int ldo) {
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += IMGPREP_THREADS) tab[i] = lut[i];
    __syncthreads();
    const int pw = W / ps, ph = H / ps, pp = ps * ps;
    for (long i = (long)blockIdx.x * IMGPREP_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * IMGPREP_THREADS) {
        const long m = i / ldo;
        const int j = (int)(i - m * ldo);
        float v = 0.f;
        if (j < 3 * pp) {
            const int c = j / pp, rem = j - c * pp, ky = rem / ps, kx = rem - ky * ps;
            const long b = m / ((long)ph * pw);
            const int p = (int)(m - b * ph * pw), py = p / pw, px = p - py * pw;
            v = tab[c * 256 + src[((b * H + (long)py * ps + ky) * W + (long)px * ps + kx) * 3 + c]];
        }
        DT<T>::st(out + i, v);
    }
}

// Patch rows in pair form: src [B][H][W][3] uint8 -> out bf16 [B * (H / ps) * (W / ps)][2K], the pair form of rows of K fp32 columns (K % 32 == 0: 128-byte
// blocks [hi(32) | lo(32)]; else the planes [hi(K) | lo(K)]); columns 3 ps ps .. K - 1 are zero in both halves.  The table has 768 entries, so its split is
// done once per workgroup: tab[c][byte] = hi | lo << 16 with hi = bf16(v) (RNE), lo = bf16(v - hi) -- the arithmetic of split_pair8_kernel -- and an element
// costs one byte load and one LDS lookup.  One thread per 8 consecutive columns of a row (K % 8 == 0: a run of 8 never crosses a 32-column block), so both
// halves leave as 16-byte stores; the (c, ky, kx) of the run's first column is divided out once and stepped from there.
__global__ __launch_bounds__(IMGPREP_THREADS) void patch_rows_pair_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut, bf16* __restrict__ out, long total,
                                                                          int H, int W, int ps, int K) {
    __shared__ uint32_t tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += IMGPREP_THREADS) {
        const float v = lut[i];
        const uint32_t hi = f32_to_bf16(v);
        tab[i] = hi | ((uint32_t)f32_to_bf16(v - bf16_to_f32((uint16_t)hi)) << 16);
    }
    __syncthreads();
    const int pw = W / ps, ph = H / ps, pp = ps * ps, kq = K >> 3, lo_off = pair_lo(K);
    for (long i = (long)blockIdx.x * IMGPREP_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * IMGPREP_THREADS) {
        const long m = i / kq;
        const int j0 = (int)(i - m * kq) << 3;
        const long b = m / ((long)ph * pw);
        const int p = (int)(m - b * ph * pw), py = p / pw, px = p - py * pw;
        int c = j0 / pp, rem = j0 - c * pp, ky = rem / ps, kx = rem - ky * ps;
        uint32_t e[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            e[w] = 0u;
            if (j0 + w < 3 * pp) e[w] = tab[c * 256 + src[((b * H + (long)py * ps + ky) * W + (long)px * ps + kx) * 3 + c]];
            if (++kx == ps) {
                kx = 0;
                if (++ky == ps) { ky = 0; ++c; }
            }
        }
        u32x4 hi, lo;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            hi[w] = (e[2 * w] & 0xffffu) | (e[2 * w + 1] << 16);
            lo[w] = (e[2 * w] >> 16) | (e[2 * w + 1] & 0xffff0000u);
        }
        bf16* q = out + m * 2 * K + pair_pos(j0, K);
        *reinterpret_cast<u32x4*>(q) = hi;
        *reinterpret_cast<u32x4*>(q + lo_off) = lo;
    }
}
