// Device case preparation of the GeoBench harness (freefine_amd/geobench.py, device_prep=True): the four cv2 restatements of src/utils/vis_utils.py on uint8
// images, byte for byte what the numpy functions give (they are the reference; neither is pinned against OpenCV on the interpolating paths).
//
//   lanczos8_kernel        _resize_lanczos4: 8 x 8 taps per output pixel from two host-built tables (index int32 clamped to the border, weight fp64 normalised:
//                          the idx / wgt arrays of _lanczos4_matrix), vertical sum first, then horizontal, taps in ascending order, rint, clamp.  The vertical
//                          sums are recomputed per output pixel (64 multiply-adds per channel) instead of going through an fp64 scratch image.
//   gather_kernel          _resize_nearest: a gather through two host-built index tables; optionally the m[m > 0] = 1 of read_and_resize_mask.
//   dilate_h / _v_kernel   dilate_mask: a separable k x k maximum, window x - k/2 .. x + k - k/2 - 1, outside the image reads as 0.
//   mask_bbox_kernel       first / last set row and column of a mask (what _affine_for_edit takes from np.where): block reduction, then 4 integer atomics.
//   coarse_edit_kernel     re_edit_2d / re_edit_3d fused: inverse affine in fp64, nearest mask tap, bilinear image taps on the 1/32 grid, the three selects.
//                          The warped image and the warped mask are never stored.
//
// Floating-point contraction is OFF for this header: the numpy code rounds every product and every sum, and a fused multiply-add in the coordinate
// (a00 x + a01 y) + a02 moves coordinates across 1/32 cells (another bilinear weight) or across .5 (another mask tap); in the Lanczos sums it changes the
// last bits a restatement of the tap loop in numpy would have to reproduce.  Coordinates must be fp64: fp32 cannot hold x * 32 + 0.5 exactly at these sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/freefine_hip.h"

#pragma clang fp contract(off)

#define CASEPREP_THREADS 256

__device__ __forceinline__ uint8_t caseprep_rint8(double v) {
    v = rint(v);                                    // round half to even, like np.rint
    return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

// src [B][H][W][C] -> dst [B][oh][ow][C].  grid = (ceil(ow / 256), oh, B), one thread per output pixel.  iy [oh][8], wy [oh][8], ix [ow][8], wx [ow][8]; indices
// are clamped into the image again here: a bad table cannot make the kernel read outside it.
template <int C>
__global__ __launch_bounds__(CASEPREP_THREADS) void lanczos8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int oh, int ow,
                                                                    const int* __restrict__ iy, const double* __restrict__ wy, const int* __restrict__ ix,
                                                                    const double* __restrict__ wx) {
    const int x = blockIdx.x * CASEPREP_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const uint8_t* s = src + (long)blockIdx.z * H * W * C;
    long row[8];
    double ky[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int r = iy[y * 8 + i];
        r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        row[i] = (long)r * W * C;
        ky[i] = wy[y * 8 + i];
    }
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (int j = 0; j < 8; ++j) {
        int col = ix[x * 8 + j];
        col = col < 0 ? 0 : (col > W - 1 ? W - 1 : col);
        const double kx = wx[x * 8 + j];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < 8; ++i) v = v + ky[i] * (double)s[row[i] + (long)col * C + c];
            acc[c] = acc[c] + kx * v;
        }
    }
    uint8_t* d = dst + (((long)blockIdx.z * oh + y) * ow + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = caseprep_rint8(acc[c]);
}

// src [B][H][W][C] -> dst [B][oh][ow][C], dst[y][x] = src[iy[y]][ix[x]]; binarise: every nonzero byte becomes 1.  One thread per output byte.
__global__ __launch_bounds__(CASEPREP_THREADS) void gather_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int C, int oh, int ow,
                                                                  const int* __restrict__ iy, const int* __restrict__ ix, int binarise) {
    const int o = blockIdx.x * CASEPREP_THREADS + threadIdx.x, y = blockIdx.y;
    if (o >= ow * C) return;
    const int x = o / C, c = o - x * C;
    int r = iy[y], col = ix[x];
    r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
    col = col < 0 ? 0 : (col > W - 1 ? W - 1 : col);
    uint8_t v = src[(((long)blockIdx.z * H + r) * W + col) * C + c];
    if (binarise && v) v = 1;
    dst[((long)blockIdx.z * oh + y) * (long)ow * C + o] = v;
}

// Horizontal maximum: src [B][H][W][C] -> dst, window x - k/2 .. x + k - k/2 - 1 cut to the row (pixels outside are 0, and bytes are >= 0).
__global__ __launch_bounds__(CASEPREP_THREADS) void dilate_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int C, int k) {
    const int o = blockIdx.x * CASEPREP_THREADS + threadIdx.x;
    if (o >= W * C) return;
    const long base = ((long)blockIdx.z * gridDim.y + blockIdx.y) * (long)W * C;
    const int x = o / C, c = o - x * C;
    int lo = x - k / 2, hi = x + k - k / 2 - 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > W - 1 ? W - 1 : hi;
    unsigned m = 0;
    for (int i = lo; i <= hi; ++i) {
        const unsigned v = src[base + (long)i * C + c];
        m = v > m ? v : m;
    }
    dst[base + o] = (uint8_t)m;
}

// Vertical maximum over rows y - k/2 .. y + k - k/2 - 1; row_bytes = W C.  grid = (ceil(row_bytes / 256), H, B).
__global__ __launch_bounds__(CASEPREP_THREADS) void dilate_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int row_bytes, int k) {
    const int o = blockIdx.x * CASEPREP_THREADS + threadIdx.x, y = blockIdx.y;
    if (o >= row_bytes) return;
    const long base = (long)blockIdx.z * H * row_bytes + o;
    int lo = y - k / 2, hi = y + k - k / 2 - 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > H - 1 ? H - 1 : hi;
    unsigned m = 0;
    for (int i = lo; i <= hi; ++i) {
        const unsigned v = src[base + (long)i * row_bytes];
        m = v > m ? v : m;
    }
    dst[base + (long)y * row_bytes] = (uint8_t)m;
}

// mask [B][H][W][mc], channel 0 read, any nonzero byte is set.  box [B][4] int32 = (-top, bottom, -left, right) as running maxima, preset by the launch to a large
// negative value (bytes 0x80): an empty mask leaves bottom < 0.  grid = (min(H, 64), B): a block strides over rows, reduces in LDS, thread 0 issues 4 atomics.
__global__ __launch_bounds__(CASEPREP_THREADS) void mask_bbox_kernel(const uint8_t* __restrict__ mask, int* __restrict__ box, int H, int W, int mc) {
    __shared__ int red[4][CASEPREP_THREADS];
    const uint8_t* m = mask + (long)blockIdx.y * H * W * mc;
    const int none = (int)0x80808080;
    int v0 = none, v1 = none, v2 = none, v3 = none;
    for (int y = blockIdx.x; y < H; y += gridDim.x)
        for (int x = threadIdx.x; x < W; x += CASEPREP_THREADS)
            if (m[((long)y * W + x) * mc]) {
                v0 = -y > v0 ? -y : v0;
                v1 = y > v1 ? y : v1;
                v2 = -x > v2 ? -x : v2;
                v3 = x > v3 ? x : v3;
            }
    red[0][threadIdx.x] = v0; red[1][threadIdx.x] = v1; red[2][threadIdx.x] = v2; red[3][threadIdx.x] = v3;
    __syncthreads();
    for (int st = CASEPREP_THREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int q = 0; q < 4; ++q) {
                const int a = red[q][threadIdx.x], b = red[q][threadIdx.x + st];
                red[q][threadIdx.x] = a > b ? a : b;
            }
        __syncthreads();
    }
    if (threadIdx.x < 4 && red[threadIdx.x][0] != none) atomicMax(box + blockIdx.y * 4 + threadIdx.x, red[threadIdx.x][0]);
}

__device__ __forceinline__ double caseprep_tap(const uint8_t* __restrict__ img, int H, int W, int yy, int xx, int c) {
    return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (double)img[((long)yy * W + xx) * 3 + c] : 0.0;
}

// One thread per destination pixel, grid = (ceil(W / 256), H, B).  d.inv [B][6]: rows 0 and 1 of the inverse affine.
__global__ __launch_bounds__(CASEPREP_THREADS) void coarse_edit_kernel(ffn_coarse_edit_desc d) {
    const int x = blockIdx.x * CASEPREP_THREADS + threadIdx.x, y = blockIdx.y, H = d.H, W = d.W;
    if (x >= W) return;
    const long b = blockIdx.z, px = (b * H + y) * W + x;
    const double* a = d.inv + b * 6;
    const uint8_t* img = d.src_img + b * H * W * 3;
    const uint8_t* msk = d.src_mask + b * H * W * d.mask_c;
    const double xd = (double)x, yd = (double)y;
    const double sx = (a[0] * xd + a[1] * yd) + a[2];
    const double sy = (a[3] * xd + a[4] * yd) + a[5];
    // target mask: the nearest tap (round half up) of the source mask, 0 outside
    const double mxd = floor(sx + 0.5), myd = floor(sy + 0.5);
    bool t = false;
    if (mxd >= 0.0 && mxd < (double)W && myd >= 0.0 && myd < (double)H) t = msk[((long)(int)myd * W + (int)mxd) * d.mask_c] != 0;
    d.tmask[px] = t ? 255 : 0;
    uint8_t o[3];
    if (t) {
        const double qx = floor(sx * 32.0 + 0.5) / 32.0, qy = floor(sy * 32.0 + 0.5) / 32.0;
        const double x0d = floor(qx), y0d = floor(qy);
        const double fx = qx - x0d, fy = qy - y0d;
        // a corner beyond [-2, side] has all of its taps outside the image, like the clamped one
        const int x0 = (int)(x0d < -2.0 ? -2.0 : (x0d > (double)W ? (double)W : x0d)), y0 = (int)(y0d < -2.0 ? -2.0 : (y0d > (double)H ? (double)H : y0d));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t00 = caseprep_tap(img, H, W, y0, x0, c), t01 = caseprep_tap(img, H, W, y0, x0 + 1, c);
            const double t10 = caseprep_tap(img, H, W, y0 + 1, x0, c), t11 = caseprep_tap(img, H, W, y0 + 1, x0 + 1, c);
            o[c] = caseprep_rint8((t00 * (1.0 - fx) + t01 * fx) * (1.0 - fy) + (t10 * (1.0 - fx) + t11 * fx) * fy);
        }
    }
    const uint8_t* himg = (d.hole_img ? d.hole_img : d.src_img) + px * 3;
    const uint8_t* bg = d.bg + px * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        bool holed;
        if (d.hole_mask) holed = d.hole_mask[px * d.hole_mask_c + (d.hole_mask_c == 3 ? c : 0)] != 0;
        else holed = msk[((long)y * W + x) * d.mask_c] != 0;
        d.final_img[px * 3 + c] = t ? o[c] : bg[c];
        d.trans_hole[px * 3 + c] = t ? o[c] : (holed ? (uint8_t)0 : himg[c]);
    }
}
