// DIFT correspondence search of the Mean Distance metric (reference: evaluation/metrics/MD/mean_distance.py:139-165) without the upsampled feature maps.
//
// The reference upsamples both [1, C, h, w] feature maps bilinearly to [1, C, H, W] (1.3 GB each at SD-2.1 / 512^2) and takes, per keypoint, the argmax of a
// cosine map over all H x W pixels.  Bilinear interpolation is linear: the full-resolution vector at a pixel is f = wa a + wb b + wc c + wd d of the four
// low-resolution vectors of its cell (a = (y0, x0), b = (y0, x1), c = (y1, x0), d = (y1, x1), x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1) as ATen clamps), so
//     <q, f>  = wa D[a] + wb D[b] + wc D[c] + wd D[d]                 D[j] = <q, F[j]>                          (K x hw dot products)
//     |f|^2   = sum_ij wi wj <F[i], F[j]>                              from five low-resolution maps indexed at the cell's corners:
//               N[j] = <j, j>, R[j] = <j, j+x>, Dn[j] = <j, j+y>, DR[j] = <j, j+x+y>, DL[j] = <j+x, j+y>   (neighbours clamped)
// which is exact in real arithmetic.  What remains per keypoint is a scan of H x W pixels at ~40 FMAs each over tables that stay in cache.
//
// Kernels (plain fp32 vector arithmetic, wave reductions by shuffles in a fixed order: every result is deterministic whatever the launch geometry):
//   dift_mean_kernel<T>   one wave per low-resolution position of the edited image: the ensemble mean of its E rows, in fp32        -> Tm [hw][C]
//   dift_query_kernel<T>  one wave per keypoint: the 4-tap bilinear sample of the source image's ensemble mean at the keypoint     -> q [K][C], |q| [K]
//   dift_gram_kernel      one wave per position: N, R, Dn, DR, DL                                                                     -> 5 x [hw]
//   dift_dots_kernel      one wave per position: D[k][j] for the keypoints of this launch                                             -> D [K][hw]
//   dift_match_kernel     one workgroup per keypoint: cosine at every pixel, (value, lowest flat index) maximum                       -> (row, col) [K], cos [K]
// Source coordinates and weights follow ATen's upsample_bilinear2d (align_corners = False, size given) in fp32, every operation rounded on its own:
// src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = float(n_src) / n_dst.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

#define DIFT_KP_PER_LAUNCH 32
#define DIFT_MATCH_THREADS 1024

struct dift_kps {
    int rc[DIFT_KP_PER_LAUNCH][2];   // (row, col) at full resolution, validated on the host
};

__device__ __forceinline__ float dift_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ATen's area_pixel_compute_source_index + guard_index_and_lambda in fp32 (no contraction: the reference rounds the product before the subtraction)
__device__ __forceinline__ void dift_src_index(int dst, int n_src, float scale, int& i0, int& i1, float& lam) {
    float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, n_src - 1);
    i1 = min(i0 + 1, n_src - 1);
    lam = fminf(fmaxf(__fsub_rn(s, (float)i0), 0.f), 1.f);
}

// one 16-byte chunk of a row (4 floats / 8 bf16) starting at element c, as floats.  The last chunk of a bf16 row with C % 8 == 4 is an 8-byte load whose upper
// four values read as zero; returns whether the chunk was a whole one.
template <typename T>
__device__ __forceinline__ bool dift_load(const T* row, int c, int C, float* v) {
    if constexpr (sizeof(T) == 2) {
        if (c + 8 > C) {
            const u32x2 half = *reinterpret_cast<const u32x2*>(row + c);
            DT<T>::unpack(u32x4{half[0], half[1], 0u, 0u}, v);
            return false;
        }
    }
    DT<T>::unpack(*reinterpret_cast<const u32x4*>(row + c), v);
    return true;
}

template <typename T>
__global__ __launch_bounds__(256) void dift_mean_kernel(const T* __restrict__ x, long es, int ld, int E, int C, int hw, float* __restrict__ Tm) {
    constexpr int EPC = DT<T>::EPC;
    const int j = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (j >= hw) return;
    const float fe = (float)E;
    for (int c = lane * EPC; c < C; c += 64 * EPC) {
        float acc[EPC], v[EPC];
        bool whole = true;
#pragma unroll
        for (int i = 0; i < EPC; ++i) acc[i] = 0.f;
        for (int e = 0; e < E; ++e) {
            whole = dift_load(x + e * es + (long)j * ld, c, C, v);
#pragma unroll
            for (int i = 0; i < EPC; ++i) acc[i] += v[i];
        }
#pragma unroll
        for (int i = 0; i < EPC; ++i) acc[i] = acc[i] / fe;
        float* o = Tm + (long)j * C + c;
        store4(o, acc);
        if (EPC == 8 && whole) store4(o + 4, acc + EPC - 4);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dift_query_kernel(const T* __restrict__ x, long es, int ld, int E, int C, int h, int w, float sy, float sx,
                                                         dift_kps kp, int n, float* __restrict__ q, float* __restrict__ qn) {
    constexpr int EPC = DT<T>::EPC;
    const int k = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (k >= n) return;
    int y0, y1, x0, x1;
    float ly, lx;
    dift_src_index(kp.rc[k][0], h, sy, y0, y1, ly);
    dift_src_index(kp.rc[k][1], w, sx, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx, fe = (float)E;
    const long pos[4] = {(long)(y0 * w + x0) * ld, (long)(y0 * w + x1) * ld, (long)(y1 * w + x0) * ld, (long)(y1 * w + x1) * ld};
    float qq = 0.f;
    for (int c = lane * EPC; c < C; c += 64 * EPC) {
        float m[4][EPC], v[EPC], r[EPC];
        bool whole = true;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < EPC; ++i) m[t][i] = 0.f;
            for (int e = 0; e < E; ++e) {
                whole = dift_load(x + e * es + pos[t], c, C, v);
#pragma unroll
                for (int i = 0; i < EPC; ++i) m[t][i] += v[i];
            }
        }
#pragma unroll
        for (int i = 0; i < EPC; ++i) {
            const float top = hx * (m[0][i] / fe) + lx * (m[1][i] / fe), bot = hx * (m[2][i] / fe) + lx * (m[3][i] / fe);
            r[i] = hy * top + ly * bot;
            qq += r[i] * r[i];                         // (elements past a short last chunk are zero)
        }
        float* o = q + (long)k * C + c;
        store4(o, r);
        if (EPC == 8 && whole) store4(o + 4, r + EPC - 4);
    }
    qq = dift_wave_sum(qq);
    if (lane == 0) qn[k] = sqrtf(qq);
}

__global__ __launch_bounds__(256) void dift_gram_kernel(const float* __restrict__ Tm, int C, int h, int w, float* __restrict__ N, float* __restrict__ R,
                                                        float* __restrict__ Dn, float* __restrict__ DR, float* __restrict__ DL) {
    const int j = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (j >= h * w) return;
    const int y = j / w, x = j - y * w, xr = min(x + 1, w - 1), yd = min(y + 1, h - 1);
    const float* pa = Tm + (long)j * C;
    const float* pb = Tm + (long)(y * w + xr) * C;
    const float* pc = Tm + (long)(yd * w + x) * C;
    const float* pd = Tm + (long)(yd * w + xr) * C;
    float sn = 0.f, sr = 0.f, sd = 0.f, sdr = 0.f, sdl = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(pa + c), b = *reinterpret_cast<const f32x4*>(pb + c);
        const f32x4 cc = *reinterpret_cast<const f32x4*>(pc + c), d = *reinterpret_cast<const f32x4*>(pd + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sn += a[i] * a[i];
            sr += a[i] * b[i];
            sd += a[i] * cc[i];
            sdr += a[i] * d[i];
            sdl += b[i] * cc[i];
        }
    }
    sn = dift_wave_sum(sn);
    sr = dift_wave_sum(sr);
    sd = dift_wave_sum(sd);
    sdr = dift_wave_sum(sdr);
    sdl = dift_wave_sum(sdl);
    if (lane == 0) {
        N[j] = sn;
        R[j] = sr;
        Dn[j] = sd;
        DR[j] = sdr;
        DL[j] = sdl;
    }
}

// D[k][j] = <q[k], Tm[j]> for the n keypoints of this launch (q, D already offset to the first of them)
__global__ __launch_bounds__(256) void dift_dots_kernel(const float* __restrict__ Tm, const float* __restrict__ q, int C, int hw, int n, float* __restrict__ D) {
    const int j = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (j >= hw) return;
    const float* pt = Tm + (long)j * C;
    for (int k = 0; k < n; ++k) {
        const float* pq = q + (long)k * C;
        float s = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(pt + c), b = *reinterpret_cast<const f32x4*>(pq + c);
            s += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
        }
        s = dift_wave_sum(s);
        if (lane == 0) D[(long)k * hw + j] = s;
    }
}

// numpy's argmax rule on (value, flat index): the larger value wins, equal values -> the lower index; NaN never enters (only `>` comparisons admit a value)
__device__ __forceinline__ void dift_better(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

// grid = keypoints of this launch, one workgroup each (D, qn, out_* already offset to the first of them)
__global__ __launch_bounds__(DIFT_MATCH_THREADS) void dift_match_kernel(const float* __restrict__ N, const float* __restrict__ R, const float* __restrict__ Dn,
                                                                        const float* __restrict__ DR, const float* __restrict__ DL, const float* __restrict__ D,
                                                                        const float* __restrict__ qn, int h, int w, int H, int W, float sy, float sx,
                                                                        int* __restrict__ out_rc, float* __restrict__ out_cos) {
    __shared__ float s_v[DIFT_MATCH_THREADS / 64];
    __shared__ int s_i[DIFT_MATCH_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* Dk = D + (long)k * h * w;
    const float qnk = fmaxf(qn[k], 1e-8f);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    const int npix = H * W;
    for (int p = tid; p < npix; p += DIFT_MATCH_THREADS) {
        const int r = p / W, c = p - r * W;
        int y0, y1, x0, x1;
        float ly, lx;
        dift_src_index(r, h, sy, y0, y1, ly);
        dift_src_index(c, w, sx, x0, x1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float wa = hy * hx, wb = hy * lx, wc = ly * hx, wd = ly * lx;
        const int ia = y0 * w + x0, ib = y0 * w + x1, ic = y1 * w + x0, id = y1 * w + x1;
        const float sq = wa * wa * N[ia] + wb * wb * N[ib] + wc * wc * N[ic] + wd * wd * N[id];
        const float cr = wa * wb * R[ia] + wc * wd * R[ic] + wa * wc * Dn[ia] + wb * wd * Dn[ib] + wa * wd * DR[ia] + wb * wc * DL[ia];
        const float n2 = sq + 2.f * cr;
        const float dot = wa * Dk[ia] + wb * Dk[ib] + wc * Dk[ic] + wd * Dk[id];
        const float cs = dot / (qnk * fmaxf(sqrtf(fmaxf(n2, 0.f)), 1e-8f));
        if (cs > best) {                               // p grows: the first of equal values stays
            best = cs;
            bi = p;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dift_better(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    if (lane == 0) {
        s_v[wave] = best;
        s_i[wave] = bi;
    }
    __syncthreads();
    if (wave == 0) {
        best = lane < DIFT_MATCH_THREADS / 64 ? s_v[lane] : -INFINITY;
        bi = lane < DIFT_MATCH_THREADS / 64 ? s_i[lane] : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dift_better(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) {
            const bool none = bi == 0x7fffffff;        // every cosine was NaN (non-finite features): position (0, 0), cosine NaN
            const int p = none ? 0 : bi;
            out_rc[2 * k] = p / W;
            out_rc[2 * k + 1] = p - (p / W) * W;
            out_cos[k] = none ? __int_as_float(0x7fc00000) : best;
        }
    }
}
