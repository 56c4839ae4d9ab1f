// Click-to-mask (freefine_amd/sam.py: EfficientSAM): the three kernels around the network that an interactive caller feels, none of them a GEMM.
//
//   sam_patch_rows_kernel        EfficientSam.preprocess after ToTensor, straight into the patch GEMM's operand rows: v = byte / 255 in fp32, ATen's
//                                upsample_bilinear2d (align_corners = False, no antialiasing) to side x side where the image has another size, then
//                                (v - mean) / std; row = patch, columns (channel, ky, kx) as encoder.im2col.  No fp32 image exists in memory.
//   sam_patch_rows_pair_kernel   the same values as the split-bf16 PAIR operand (hi = bf16(v), lo = bf16(v - hi); layout: common.h pair_pos), 8 columns per thread.
//   hyper_masks_kernel           logits[n][m][pixel] = <hyper[n][m][:], up[n][pixel][:]>: the mask decoder's hyper_in @ upscaled.view(b, c, h w) on NHWC rows.
//   upsample_bicubic_kernel      ATen's upsample_bicubic2d (align_corners = False, A = -0.75) of the logits to the image size, and the thresholded uint8 mask
//                                from the very value that is stored.
//
// Included after caseprep.h: floating-point contraction is OFF here too.  The no-resize rows are (byte / 255 - mean) / std bit for bit as torch evaluates
// them, and the interpolations round every product and every sum as ATen's scalar code does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/freefine_hip.h"
#include "common.h"

#pragma clang fp contract(off)

#define SAM_THREADS 256

struct sam_norm { float mean[3], std[3]; };      // by value in the kernel arguments

// ATen area_pixel_compute_source_index (align_corners = False, not cubic) + guard_index_and_lambda: i0, i1 = i0 + (i0 < in - 1), weight of i1
__device__ __forceinline__ void sam_bilinear_tap(float scale, int dst, int in, int* i0, int* i1, float* w1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    int i = (int)s;
    i = i > in - 1 ? in - 1 : i;
    float l = s - (float)i;
    l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
    *i0 = i;
    *i1 = i + (i < in - 1 ? 1 : 0);
    *w1 = l;
}

// the normalised value of destination pixel (y, x), channel c of image `img` [H][W][3]; sh, sw = in / out in fp32 (unused when the sizes agree)
__device__ __forceinline__ float sam_pixel(const uint8_t* __restrict__ img, int H, int W, int side, float sh, float sw, int y, int x, int c, const sam_norm& nm) {
    float v;
    if (H == side && W == side) {
        v = (float)img[((long)y * W + x) * 3 + c] / 255.f;
    } else {
        int y0, y1, x0, x1;
        float h1, w1;
        sam_bilinear_tap(sh, y, H, &y0, &y1, &h1);
        sam_bilinear_tap(sw, x, W, &x0, &x1, &w1);
        const float h0 = 1.f - h1, w0 = 1.f - w1;
        const float v00 = (float)img[((long)y0 * W + x0) * 3 + c] / 255.f, v01 = (float)img[((long)y0 * W + x1) * 3 + c] / 255.f;
        const float v10 = (float)img[((long)y1 * W + x0) * 3 + c] / 255.f, v11 = (float)img[((long)y1 * W + x1) * 3 + c] / 255.f;
        v = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11);
    }
    return (v - nm.mean[c]) / nm.std[c];
}

// src [B][H][W][3] uint8 -> out [B (side / ps)^2][ldo] of T, columns 3 ps ps .. ldo - 1 zero.  One thread per output element (grid-stride): the writes of a
// workgroup are contiguous, the byte reads of one patch row (kx) are neighbours.
template <typename T>
__global__ __launch_bounds__(SAM_THREADS) void sam_patch_rows_kernel(const uint8_t* __restrict__ src, T* __restrict__ out, long total, int H, int W, int side, int ps,
                                                                    int ldo, sam_norm nm) {
    const int pw = side / ps, pp = ps * ps;
    const float sh = (float)H / (float)side, sw = (float)W / (float)side;
    for (long i = (long)blockIdx.x * SAM_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SAM_THREADS) {
        const long m = i / ldo;
        const int j = (int)(i - m * ldo);
        float v = 0.f;
        if (j < 3 * pp) {
            const int c = j / pp, rem = j - c * pp, ky = rem / ps, kx = rem - ky * ps;
            const long b = m / ((long)pw * pw);
            const int p = (int)(m - b * pw * pw), py = p / pw, px = p - py * pw;
            v = sam_pixel(src + b * H * W * 3, H, W, side, sh, sw, py * ps + ky, px * ps + kx, c, nm);
        }
        DT<T>::st(out + i, v);
    }
}

// The pair form: out bf16 [B (side / ps)^2][2K]; one thread per 8 consecutive columns of a row (K % 8 == 0: a run of 8 never crosses a 32-column block),
// both halves leave as 16-byte stores.  hi / lo: the arithmetic of split_pair8_kernel.
__global__ __launch_bounds__(SAM_THREADS) void sam_patch_rows_pair_kernel(const uint8_t* __restrict__ src, bf16* __restrict__ out, long total, int H, int W, int side,
                                                                         int ps, int K, sam_norm nm) {
    const int pw = side / ps, pp = ps * ps, kq = K >> 3, lo_off = pair_lo(K);
    const float sh = (float)H / (float)side, sw = (float)W / (float)side;
    for (long i = (long)blockIdx.x * SAM_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SAM_THREADS) {
        const long m = i / kq;
        const int j0 = (int)(i - m * kq) << 3;
        const long b = m / ((long)pw * pw);
        const int p = (int)(m - b * pw * pw), py = p / pw, px = p - py * pw;
        int c = j0 / pp, rem = j0 - c * pp, ky = rem / ps, kx = rem - ky * ps;
        uint32_t h[8], l[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            h[w] = l[w] = 0u;
            if (j0 + w < 3 * pp) {
                const float v = sam_pixel(src + b * H * W * 3, H, W, side, sh, sw, py * ps + ky, px * ps + kx, c, nm);
                h[w] = f32_to_bf16(v);
                l[w] = f32_to_bf16(v - bf16_to_f32((uint16_t)h[w]));
            }
            if (++kx == ps) {
                kx = 0;
                if (++ky == ps) { ky = 0; ++c; }
            }
        }
        u32x4 hi, lo;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            hi[w] = h[2 * w] | (h[2 * w + 1] << 16);
            lo[w] = l[2 * w] | (l[2 * w + 1] << 16);
        }
        bf16* q = out + m * 2 * K + pair_pos(j0, K);
        *reinterpret_cast<u32x4*>(q) = hi;
        *reinterpret_cast<u32x4*>(q + lo_off) = lo;
    }
}

// up [N][hw][C] fp32 (C % 4 == 0, C <= 64), hyper [N][M][C] (M <= 8) -> out [N][M][hw].  grid = (ceil(hw / 256), N); the M vectors of the sample are staged in
// LDS, one thread per pixel reads its C channels as 16-byte loads and keeps the M sums (in ascending channel order) in registers; the stores of a mask are
// contiguous across the workgroup.
__global__ __launch_bounds__(SAM_THREADS) void hyper_masks_kernel(const float* __restrict__ up, const float* __restrict__ hyper, float* __restrict__ out, int hw, int C,
                                                                 int M) {
    __shared__ float hv[8 * 64];
    const long n = blockIdx.y;
    for (int i = threadIdx.x; i < M * C; i += SAM_THREADS) hv[i] = hyper[n * M * C + i];
    __syncthreads();
    const int px = blockIdx.x * SAM_THREADS + threadIdx.x;
    if (px >= hw) return;
    const float4* row = reinterpret_cast<const float4*>(up + (n * hw + px) * C);
    float acc[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.f;
    for (int c4 = 0; c4 < C / 4; ++c4) {
        const float4 u = row[c4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (m < M) {
                const float* h = hv + m * C + 4 * c4;
                acc[m] = acc[m] + u.x * h[0];
                acc[m] = acc[m] + u.y * h[1];
                acc[m] = acc[m] + u.z * h[2];
                acc[m] = acc[m] + u.w * h[3];
            }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (m < M) out[(n * M + m) * hw + px] = acc[m];
}

// ATen cubic_convolution1 / cubic_convolution2 and get_cubic_upsample_coefficients
__device__ __forceinline__ void sam_cubic_coeffs(float t, float* k) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x3 = 2.f - t, x2 = 1.f - t;
    k[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    k[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    k[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    k[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// src [N][h][w] fp32 -> dst [N][H][W] fp32 and (mask != null) mask [N][H][W] = 255 (dst >= 0).  grid = (ceil(W / 256), H, N), one thread per output pixel.
// Source coordinate scale (dst + 0.5) - 0.5 with scale = in / out in fp32, NOT clamped; the four tap indices per axis are clamped to the border; rows first
// (each the sum of its four column taps), then the four rows, as ATen's upsample_bicubic2d sums.
__global__ __launch_bounds__(SAM_THREADS) void upsample_bicubic_kernel(const float* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ mask, int h, int w,
                                                                      int H, int W) {
    const int x = blockIdx.x * SAM_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float* s = src + (long)blockIdx.z * h * w;
    const float ry = ((float)h / (float)H) * ((float)y + 0.5f) - 0.5f, rx = ((float)w / (float)W) * ((float)x + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    float ky[4], kx[4];
    sam_cubic_coeffs(ry - fy, ky);
    sam_cubic_coeffs(rx - fx, kx);
    const int iy = (int)fy, ix = (int)fx;
    int cx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = ix - 1 + j;
        cx[j] = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
    }
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = iy - 1 + i;
        r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
        const float* row = s + (long)r * w;
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) t = t + row[cx[j]] * kx[j];
        v = v + t * ky[i];
    }
    const long o = ((long)blockIdx.z * H + y) * W + x;
    dst[o] = v;
    if (mask) mask[o] = v >= 0.f ? 255 : 0;
}
