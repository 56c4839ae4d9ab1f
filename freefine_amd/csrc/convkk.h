// The kernels of the Inception-v3 feature extractor behind FID (freefine_amd/inception.py): a general KH x KW convolution, window pooling, the global mean
// and the image preparation.  All fp32, all NHWC "column views": a pixel's channels are contiguous, consecutive pixels are `ld` floats apart, so a layer
// reads or writes a slice of a wider (concatenated) tensor in place.
//
//   convkk_kernel<BM, BN, WM, WN>   implicit GEMM out[m][n] = sum_k A[m][k] W[n][k] (+ bias[n], ReLU) on the exact-fp32 16x16x4 MFMA.  m = (b, oy, ox),
//                                   k = (ky, kx, ci); A is never stored: a 16-byte chunk of K is 4 input channels of ONE tap (Cin % 4 == 0), read from the image
//                                   or zero where the tap falls outside it, the row is past M or k is past K.  256 threads = 4 waves, each WM x WN of the
//                                   BM x BN tile; K in steps of 32 through LDS (one buffer, the next step's global loads in flight during the MFMAs).
//                                   LDS rows are 8 chunks (128 bytes); chunk c of row r sits in slot c ^ ((r >> 1) & 7), so the 16 lanes of a ds_read_b128
//                                   phase (16 rows, one chunk column) and of a ds_write_b128 phase (2 rows, 8 chunks) touch 16 different 16-byte bank groups.
//                                   Operand convention of common.h: lane group g = lane >> 4 supplies chunk g of a 64-byte K slab and MFMA e of 4 consumes
//                                   element e of every chunk -- the same permutation of k for both operands.  W is the MFMA's A operand and the image its B
//                                   operand, so a lane ends with 4 consecutive n of one m: one 16-byte store per 16x16 tile.  No split-K, no atomics: the
//                                   summation order is fixed and two runs are bit-identical.
//   pool2d_kernel<OP>               k x k window maximum, or the mean over the window's IN-IMAGE taps (avg_pool2d(count_include_pad=False)), taps in (ky, kx)
//                                   order; one thread per output pixel and 4 channels.
//   mean_hw_kernel                  AdaptiveAvgPool2d(1): one thread per image and 4 channels sums the HW pixels in ascending order.
//   fid_prep_kernel                 uint8 image -> lut (ToTensor + Normalize) -> ATen's bilinear upsample (align_corners = False) -> 2 v - 1, as 4-channel
//                                   NHWC pixels with a zero fourth channel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/freefine_hip.h"
#include "common.h"

#define CONVKK_THREADS 256
#define CONVKK_BK 32                          // floats of K per step
#define CONVKK_CPR (CONVKK_BK / 4)            // 16-byte chunks per LDS row

struct convkk_args {
    const float* x;
    const float* w;
    const float* bias;
    float* out;
    int M, N, K, Kpad;
    int Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad_h, pad_w, ldx, ldo, relu;
};

__device__ __forceinline__ int convkk_slot(int row, int chunk) { return row * CONVKK_CPR + (chunk ^ ((row >> 1) & (CONVKK_CPR - 1))); }

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(CONVKK_THREADS) void convkk_kernel(convkk_args a) {
    static_assert((BM / WM) * (BN / WN) == CONVKK_THREADS / 64, "four waves cover the tile");
    static_assert(BM % 32 == 0 && BN % 32 == 0 && WM % 16 == 0 && WN % 16 == 0, "tile shapes");
    constexpr int PA = BM / 32, PB = BN / 32;      // loader passes: 32 rows x 8 chunks per pass
    constexpr int TM = WM / 16, TN = WN / 16;      // 16x16 tiles per wave
    constexpr int NWN = BN / WN;
    __shared__ f32x4 sA[BM * CONVKK_CPR];
    __shared__ f32x4 sB[BN * CONVKK_CPR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int lc = tid & 7, lr = tid >> 3;         // the loader's chunk and row within a pass

    // the image coordinates of this thread's PA rows: fixed over the K loop
    long img[PA];
    int iy0[PA], ix0[PA];
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int m = m0 + p * 32 + lr;
        if (m < a.M) {
            const int hw = a.Hout * a.Wout;
            const int b = m / hw, r = m - b * hw;
            const int oy = r / a.Wout, ox = r - oy * a.Wout;
            img[p] = (long)b * a.Hin * a.Win;
            iy0[p] = oy * a.stride - a.pad_h;
            ix0[p] = ox * a.stride - a.pad_w;
        } else {
            img[p] = 0;
            iy0[p] = -(1 << 20);                   // every tap falls outside: the row loads zeros
            ix0[p] = 0;
        }
    }

    f32x4 ra[PA], rb[PB];
    auto load = [&](int kt) {
        const int k = kt * CONVKK_BK + lc * 4;
        const bool kin = k < a.K;
        const int tap = k / a.Cin, ci = k - tap * a.Cin;
        const int ky = tap / a.KW, kx = tap - ky * a.KW;
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int iy = iy0[p] + ky, ix = ix0[p] + kx;
            const bool in = kin && (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
            ra[p] = in ? *reinterpret_cast<const f32x4*>(a.x + (img[p] + (long)iy * a.Win + ix) * a.ldx + ci) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const int n = n0 + p * 32 + lr;
            rb[p] = (kin && n < a.N) ? *reinterpret_cast<const f32x4*>(a.w + (long)n * a.Kpad + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (a.K + CONVKK_BK - 1) / CONVKK_BK;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int p = 0; p < PA; ++p) sA[convkk_slot(p * 32 + lr, lc)] = ra[p];
#pragma unroll
        for (int p = 0; p < PB; ++p) sB[convkk_slot(p * 32 + lr, lc)] = rb[p];
        __syncthreads();
        if (kt + 1 < nk) load(kt + 1);
#pragma unroll
        for (int s = 0; s < CONVKK_BK / 16; ++s) {
            const int c = 4 * s + (lane >> 4);
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = sA[convkk_slot(wm * WM + i * 16 + (lane & 15), c)];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = sB[convkk_slot(wn * WN + j * 16 + (lane & 15), c)];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j][e], fa[i][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // acc[i][j]: column (lane & 15) = m, rows 4 (lane >> 4) + reg = n
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm * WM + i * 16 + (lane & 15);
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WN + j * 16 + 4 * (lane >> 4);
            if (n >= a.N) continue;                // N % 4 == 0: the four columns are inside together
            f32x4 v = acc[i][j];
            if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + n);
            if (a.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
            }
            *reinterpret_cast<f32x4*>(a.out + (long)m * a.ldo + n) = v;
        }
    }
}

// ---- window pooling ----------------------------------------------------------------------------------------------------------------------------------
template <int OP>      // FFN_POOL_MAX / FFN_POOL_AVG_VALID
__global__ __launch_bounds__(CONVKK_THREADS) void pool2d_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int Hin, int Win, int Hout, int Wout,
                                                                int C4, int ldx, int ldy, int k, int stride, int pad) {
    for (long t = (long)blockIdx.x * CONVKK_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * CONVKK_THREADS) {
        const int c = (int)(t % C4) * 4;
        long p = t / C4;
        const int ox = (int)(p % Wout);
        p /= Wout;
        const int oy = (int)(p % Hout);
        const long b = p / Hout;
        f32x4 v = OP == FFN_POOL_MAX ? f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY} : f32x4{0.f, 0.f, 0.f, 0.f};
        int count = 0;
        for (int ky = 0; ky < k; ++ky) {
            const int iy = oy * stride - pad + ky;
            if ((unsigned)iy >= (unsigned)Hin) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int ix = ox * stride - pad + kx;
                if ((unsigned)ix >= (unsigned)Win) continue;
                const f32x4 u = *reinterpret_cast<const f32x4*>(x + ((b * Hin + iy) * Win + ix) * ldx + c);
                if (OP == FFN_POOL_MAX) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (u[e] > v[e] || u[e] != u[e]) ? u[e] : v[e];      // a NaN wins, as in ATen
                } else {
                    v += u;
                }
                ++count;
            }
        }
        if (OP != FFN_POOL_MAX) {
            const float n = (float)count;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] / n;
        }
        *reinterpret_cast<f32x4*>(y + ((b * Hout + oy) * Wout + ox) * ldy + c) = v;
    }
}

// ---- the global mean: y [B][C] = mean over HW of x [B][HW] (pixel stride ldx), pixels summed in ascending order ---------------------------------------
__global__ __launch_bounds__(CONVKK_THREADS) void mean_hw_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int HW, int C4, int ldx) {
    const long t = (long)blockIdx.x * CONVKK_THREADS + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C4) * 4;
    const long b = t / C4;
    const float* p = x + b * HW * ldx + c;
    f32x4 s{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < HW; ++i) s += *reinterpret_cast<const f32x4*>(p + (long)i * ldx);
    const float n = (float)HW;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = s[e] / n;
    *reinterpret_cast<f32x4*>(y + b * C4 * 4 + c) = s;
}

// ---- image preparation: src uint8 [B][S][S][3] -> out fp32 [B][T][T][4] ------------------------------------------------------------------------------
// ATen's upsample_bilinear2d, align_corners = False: scale = S / T in fp32, source = max(0, scale (dst + 0.5) - 0.5), i0 = min(int(source), S - 1),
// i1 = i0 + (i0 < S - 1), weight of i1 = source - i0; blended as h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) on v = lut[c][byte]; then 2 v - 1.
__global__ __launch_bounds__(CONVKK_THREADS) void fid_prep_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut, float* __restrict__ out, long total,
                                                                 int S, int T) {
    const long t = (long)blockIdx.x * CONVKK_THREADS + threadIdx.x;
    if (t >= total) return;
    const int ox = (int)(t % T);
    const long q = t / T;
    const int oy = (int)(q % T);
    const long b = q / T;
    const float scale = (float)S / (float)T;
    float sy = scale * ((float)oy + 0.5f) - 0.5f, sx = scale * ((float)ox + 0.5f) - 0.5f;
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
    int y0 = (int)sy, x0 = (int)sx;
    y0 = y0 > S - 1 ? S - 1 : y0;
    x0 = x0 > S - 1 ? S - 1 : x0;
    const int y1 = y0 + (y0 < S - 1), x1 = x0 + (x0 < S - 1);
    const float h1 = sy - (float)y0, w1 = sx - (float)x0, h0 = 1.f - h1, w0 = 1.f - w1;
    const uint8_t* im = src + b * S * S * 3;
    const uint8_t *p00 = im + ((long)y0 * S + x0) * 3, *p01 = im + ((long)y0 * S + x1) * 3, *p10 = im + ((long)y1 * S + x0) * 3, *p11 = im + ((long)y1 * S + x1) * 3;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* l = lut + c * 256;
        const float r = h0 * (w0 * l[p00[c]] + w1 * l[p01[c]]) + h1 * (w0 * l[p10[c]] + w1 * l[p11[c]]);
        v[c] = 2.f * r - 1.f;
    }
    *reinterpret_cast<f32x4*>(out + t * 4) = v;
}
