// Click-to-mask (freefine_amd/sam.py: EfficientSAM): the three kernels around the network that an interactive caller feels, none of them a GEMM.
//
//   sam_patch_rows_kernel        EfficientSam.preprocess after ToTensor, straight into the patch GEMM's operand rows: v = byte / 255 in fp32, ATen's
//                                upsample_bilinear2d (align_corners = False, no antialiasing) to side x side where the image has another size, then
//                                (v - mean) / std; row = patch, columns (channel, ky, kx) as encoder.im2col.  No fp32 image exists in memory.
//   sam_patch_rows_pair_kernel   the same values as the split-bf16 PAIR operand (hi = bf16(v), lo = bf16(v - hi); layout: common.h pair_pos), 8 columns per thread.
//   hyper_masks_kernel           logits[n][m][pixel] = <hyper[n][m][:], up[n][pixel][:]>: the mask decoder's hyper_in @ upscaled.view(b, c, h w) on NHWC rows.
//   upsample_bicubic_kernel      ATen's upsample_bicubic2d (align_corners = False, A = -0.75) of the logits to the image size, and the thresholded uint8 mask
//                                from the very value that is stored.
// and the two of automatic mask generation (HipEfficientSam.generate), whose cost is what happens to 3 x points^2 candidate maps at image size:
//   upsample_bicubic_stats_kernel  the same bicubic values counted, not stored: per map the pixels >= 0, > +offset, > -offset and the box of the first
//   box_nms_kernel                 the pairwise IoU > thresh bit matrix of score-ordered boxes, one 64 x 64 tile of pairs per workgroup
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

// The value of destination pixel (y, x) of a map s [h][w] resampled to H x W: ATen's upsample_bicubic2d.  Source coordinate scale (dst + 0.5) - 0.5 with
// scale = in / out in fp32, NOT clamped; the four tap indices per axis are clamped to the border; rows first (each the sum of its four column taps), then
// the four rows, as ATen sums.  The ONE place this value is computed: upsample_bicubic_kernel stores it, upsample_bicubic_stats_kernel counts it, and the
// two cannot differ in a rounding.
__device__ __forceinline__ float sam_bicubic_value(const float* __restrict__ s, int h, int w, int H, int W, int y, int x) {
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
    return v;
}

// src [N][h][w] fp32 -> dst [N][H][W] fp32 and (mask != null) mask [N][H][W] = 255 (dst >= 0).  grid = (ceil(W / 256), H, N), one thread per output pixel.
__global__ __launch_bounds__(SAM_THREADS) void upsample_bicubic_kernel(const float* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ mask, int h, int w,
                                                                      int H, int W) {
    const int x = blockIdx.x * SAM_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float v = sam_bicubic_value(src + (long)blockIdx.z * h * w, h, w, H, W, y, x);
    const long o = ((long)blockIdx.z * H + y) * W + x;
    dst[o] = v;
    if (mask) mask[o] = v >= 0.f ? 255 : 0;
}

// ---- automatic mask generation (freefine_amd/sam.py generate): what the point-grid pass wants from 3 x points^2 candidate maps at image size --------------
#define SAM_STATS_ROW_BLOCKS 16      // workgroups per map: each strides over its rows and ends in at most 7 global atomics
#define SAM_WAVE 64

// stats int32 [N][8] = area, n_hi, n_lo, x_min, y_min, x_max, y_max, 0.  The three launches of one call: neutral elements, accumulation, empty maps -> 0 0 0 0.
__global__ __launch_bounds__(SAM_THREADS) void bicubic_stats_init_kernel(int* __restrict__ stats, int N) {
    const int n = blockIdx.x * SAM_THREADS + threadIdx.x;
    if (n >= N) return;
    int* st = stats + 8 * (long)n;
    st[0] = st[1] = st[2] = 0;
    st[3] = st[4] = 0x7fffffff;
    st[5] = st[6] = -1;
    st[7] = 0;
}

__global__ __launch_bounds__(SAM_THREADS) void bicubic_stats_finish_kernel(int* __restrict__ stats, int N) {
    const int n = blockIdx.x * SAM_THREADS + threadIdx.x;
    if (n >= N) return;
    int* st = stats + 8 * (long)n;
    if (st[0] == 0) st[3] = st[4] = st[5] = st[6] = 0;
}

// src [N][h][w] fp32 -> per map the counts of v >= 0, v > +offset, v > -offset and the extents of v >= 0 over the H x W values v that
// upsample_bicubic_kernel would store; no fp32 image is written.  mask (may be null) [N][H][W] = 255 (v >= 0).  grid = (row blocks, N): a workgroup takes rows
// blockIdx.x, + gridDim.x, .. in runs of 256 columns.  Everything accumulated is an integer, so the result does not depend on the order of execution: the counts
// are wave ballots and population counts (uniform over the wave), the extents per-lane integer min / max folded across the wave by shuffles at the end; the four
// waves meet in LDS and the workgroup issues 3 atomic adds and, where it saw a pixel of the mask, 4 atomic min / max.
__global__ __launch_bounds__(SAM_THREADS) void upsample_bicubic_stats_kernel(const float* __restrict__ src, int* __restrict__ stats, uint8_t* __restrict__ mask, int h, int w,
                                                                            int H, int W, float offset) {
    __shared__ int part[SAM_THREADS / SAM_WAVE][7];
    const long n = blockIdx.y;
    const float* s = src + n * h * w;
    const float lo_t = -offset;
    int area = 0, n_hi = 0, n_lo = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        for (int xb = 0; xb < W; xb += SAM_THREADS) {           // uniform bounds: every lane reaches the ballots
            const int x = xb + threadIdx.x;
            bool on = false, hi = false, lo = false;
            if (x < W) {
                const float v = sam_bicubic_value(s, h, w, H, W, y, x);
                on = v >= 0.f;
                hi = v > offset;
                lo = v > lo_t;
                if (mask) mask[(n * H + y) * W + x] = on ? 255 : 0;
                if (on) {
                    x0 = x < x0 ? x : x0;
                    x1 = x > x1 ? x : x1;
                    y0 = y < y0 ? y : y0;
                    y1 = y > y1 ? y : y1;
                }
            }
            area += __popcll(__ballot(on));
            n_hi += __popcll(__ballot(hi));
            n_lo += __popcll(__ballot(lo));
        }
    }
#pragma unroll
    for (int d = SAM_WAVE / 2; d >= 1; d >>= 1) {
        const int a = __shfl_xor(x0, d, SAM_WAVE), b = __shfl_xor(y0, d, SAM_WAVE), c = __shfl_xor(x1, d, SAM_WAVE), e = __shfl_xor(y1, d, SAM_WAVE);
        x0 = a < x0 ? a : x0;
        y0 = b < y0 ? b : y0;
        x1 = c > x1 ? c : x1;
        y1 = e > y1 ? e : y1;
    }
    const int wave = threadIdx.x / SAM_WAVE;
    if (threadIdx.x % SAM_WAVE == 0) {
        int* p = part[wave];
        p[0] = area, p[1] = n_hi, p[2] = n_lo, p[3] = x0, p[4] = y0, p[5] = x1, p[6] = y1;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < SAM_THREADS / SAM_WAVE; ++k) {
        const int* p = part[k];
        area += p[0], n_hi += p[1], n_lo += p[2];
        x0 = p[3] < x0 ? p[3] : x0;
        y0 = p[4] < y0 ? p[4] : y0;
        x1 = p[5] > x1 ? p[5] : x1;
        y1 = p[6] > y1 ? p[6] : y1;
    }
    int* st = stats + 8 * n;
    if (area) atomicAdd(st + 0, area);
    if (n_hi) atomicAdd(st + 1, n_hi);
    if (n_lo) atomicAdd(st + 2, n_lo);
    if (area) {
        atomicMin(st + 3, x0);
        atomicMin(st + 4, y0);
        atomicMax(st + 5, x1);
        atomicMax(st + 6, y1);
    }
}

// boxes fp32 [M][4] XYXY, best first -> suppress uint64 [M][ceil(M / 64)]: bit j of row i = (j > i and iou(i, j) > thresh), torchvision's box arithmetic in fp32
// (no "+ 1"; contraction is off, every operation rounds on its own): area = (x2 - x1)(y2 - y1), inter = max(min(x2) - max(x1), 0) max(min(y2) - max(y1), 0),
// iou = inter / (area_i + area_j - inter).  0 / 0 is NaN and NaN > thresh is false: two zero-area boxes do not suppress each other.  grid = (column blocks,
// row blocks), one wave per 64 x 64 tile of pairs: lane = row, the tile's 64 column boxes in LDS.  Tiles below the diagonal are written as zeros: the whole
// matrix is defined by this launch.
__global__ __launch_bounds__(SAM_WAVE) void box_nms_kernel(const float* __restrict__ boxes, unsigned long long* __restrict__ suppress, int M, float thresh) {
    __shared__ float4 col[SAM_WAVE];
    const int nb = gridDim.x, cb = blockIdx.x, rb = blockIdx.y;
    const int i = rb * SAM_WAVE + threadIdx.x, jl = cb * SAM_WAVE + threadIdx.x;
    if (cb >= rb && jl < M) col[threadIdx.x] = make_float4(boxes[4 * (long)jl], boxes[4 * (long)jl + 1], boxes[4 * (long)jl + 2], boxes[4 * (long)jl + 3]);
    __syncthreads();
    if (i >= M) return;
    unsigned long long bits = 0ull;
    if (cb >= rb) {
        const float x1 = boxes[4 * (long)i], y1 = boxes[4 * (long)i + 1], x2 = boxes[4 * (long)i + 2], y2 = boxes[4 * (long)i + 3];
        const float ai = (x2 - x1) * (y2 - y1);
        const int cols = M - cb * SAM_WAVE < SAM_WAVE ? M - cb * SAM_WAVE : SAM_WAVE;
        for (int k = 0; k < cols; ++k) {
            if (cb * SAM_WAVE + k <= i) continue;
            const float4 b = col[k];
            const float aj = (b.z - b.x) * (b.w - b.y);
            const float iw = fmaxf(fminf(x2, b.z) - fmaxf(x1, b.x), 0.f), ih = fmaxf(fminf(y2, b.w) - fmaxf(y1, b.y), 0.f);
            const float inter = iw * ih;
            const float iou = inter / ((ai + aj) - inter);
            if (iou > thresh) bits |= 1ull << k;
        }
    }
    suppress[(long)i * nb + cb] = bits;
}
