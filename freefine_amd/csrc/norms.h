// GroupNorm / LayerNorm / row-softmax for [B, HW, C] (channel-contiguous) activations, gfx950.
// HBM-bound kernels: 16-byte vector accesses, fp32 statistics (final group reduction in fp64).
//
// GroupNorm(32 groups) is split into (1) per-channel partial statistics (mean, M2) over pixel chunks, (2) a tiny finalize
// that turns them into per-(batch, channel) scale/shift, (3) an elementwise apply with optional SiLU.
// Replaces torch.nn.GroupNorm + SiLU inside diffusers ResnetBlock2D / Transformer2DModel / conv_norm_out
// (reached from /root/reference/src/utils/attention.py:105-214).
#pragma once
#include "common.h"
#include "layernorm_row.h"      // store_pair4, layernorm_row

// ---- (1) partial statistics: grid (nchunk, B), 256 threads ------------------------------------------------------
// partial[b][chunk][c][2] = (mean, M2) of channel c over the chunk's pixels, M2 = sum (x - mean)^2.  (sum, sum of squares) in fp32 loses the variance to
// the cancellation in E[x^2] - mean^2 once |mean| is a few times the standard deviation (tests/test_norms_gpu.py: 3.3e-5 of the output at mean = 16 std,
// 1.9e-3 at 256 std), so every thread sums x - pivot and (x - pivot)^2 (pivot = its first pixel: within a few std of its mean) and the pieces are merged
// as (count, mean, M2) in fp64.  The number of pixels of a piece follows from its index, so it is not stored.
__device__ __forceinline__ int gn_row_count(int p0, int p1, int row, int ppi) {      // pixels p0 + row, p0 + row + ppi, ... below p1
    return p0 + row < p1 ? (p1 - p0 - row + ppi - 1) / ppi : 0;
}
template <typename T>
__global__ __launch_bounds__(256) void gn_partial_kernel(const T* __restrict__ x, float* __restrict__ partial, int HW,
                                                         int C, int pix_per_chunk) {
    constexpr int EPC = DT<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ls = reinterpret_cast<float*>(smem);  // [ppi][C][2] per-thread-row (mean, M2) (round 2: no LDS atomics -- 16 contended atomic
                                                 // adds per thread made this HBM-bound kernel run at 2.7 TB/s)
    const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
    const int cch = C / EPC;                 // 16-byte chunks per pixel
    const int tid = threadIdx.x;
    const int p0 = chunk * pix_per_chunk;
    const int p1 = min(HW, p0 + pix_per_chunk);
    float* dst = partial + ((long)b * nchunk + chunk) * 2 * C;
    for (int cbase = 0; cbase < cch; cbase += 256) {
        const int cols = min(cch - cbase, 256);  // chunk columns handled concurrently in this sweep
        const int ppi = max(1, 256 / cols);       // pixel rows of threads
        const int cc = cbase + tid % cols, pp = tid / cols;
        const bool active = pp < ppi;
        if (active) {
            float s[EPC], ss[EPC], pv[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) s[e] = ss[e] = pv[e] = 0.f;
            // eight pixels in flight per thread: a single dependent load per iteration made this kernel latency bound
            const T* src = x + ((long)b * HW) * C + cc * EPC;
            int px = p0 + pp;
            const int cnt = gn_row_count(p0, p1, pp, ppi), first = px;      // the pivot is the thread's first pixel, taken from the first batch of loads (a load of its own would add a round trip to memory)
            for (; px + 7 * ppi < p1; px += 8 * ppi) {
                u32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const u32x4*>(src + (long)(px + u * ppi) * C);
                // all eight loads before any arithmetic.  Without this barrier the compiler issues three (bf16) of the loads up front and the other five one at a
                // time, each behind an s_waitcnt vmcnt(0), between the sums.  tools/bench_kernels.py --only norm, B = 4, GroupNorm + SiLU without -> with it:
                // bf16 64x64 C=960 38.6 -> 29.9 us, 32x32 C=1920 47.1 -> 28.8 us; fp32 45.0 -> 42.1 and 45.0 -> 38.5 us
                __builtin_amdgcn_sched_barrier(0);
                if (px == first) DT<T>::unpack(v[0], pv);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float f[EPC];
                    DT<T>::unpack(v[u], f);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const float d = f[e] - pv[e];
                        s[e] += d;
                        ss[e] += d * d;
                    }
                }
            }
            for (; px < p1; px += ppi) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(src + (long)px * C);
                float f[EPC];
                DT<T>::unpack(v, f);
                if (px == first) DT<T>::unpack(v, pv);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float d = f[e] - pv[e];
                    s[e] += d;
                    ss[e] += d * d;
                }
            }
            const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float m = s[e] * inv;                                                // mean of x - pivot
                ls[(pp * cols + (cc - cbase)) * 2 * EPC + 2 * e] = pv[e] + m;
                ls[(pp * cols + (cc - cbase)) * 2 * EPC + 2 * e + 1] = fmaxf(ss[e] - s[e] * m, 0.f);
            }
        }
        __syncthreads();
        // fixed-order merge of the pixel rows of threads (deterministic): mean = sum n_r mean_r / n, M2 = sum (M2_r + n_r mean_r^2) - n mean^2 -- in fp64, where
        // the cancellation costs 2 log2(|mean| / std) of 53 bits
        const int n = max(p1 - p0, 0);
        for (int i = tid; i < cols * EPC; i += 256) {
            double sm = 0.0, sq = 0.0;
            for (int r = 0; r < ppi; ++r) {
                const double nr = (double)gn_row_count(p0, p1, r, ppi), mr = (double)ls[(r * cols * EPC + i) * 2];
                sm += nr * mr;
                sq += (double)ls[(r * cols * EPC + i) * 2 + 1] + nr * mr * mr;
            }
            const double mean = n > 0 ? sm / (double)n : 0.0;
            const double m2 = fmax(sq - sm * mean, 0.0);
            dst[(cbase * EPC + i) * 2] = (float)mean;      // [c][2] with c = (cbase + column) * EPC + e: same interleaving as ls
            dst[(cbase * EPC + i) * 2 + 1] = (float)m2;
        }
        __syncthreads();
    }
}

// ---- (2) finalize: grid (G, B), 64 threads: scale[b][c] = rstd*gamma[c], shift[b][c] = beta[c]-mean*rstd*gamma[c]
__global__ __launch_bounds__(64) void gn_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ scale,
                                                         float* __restrict__ shift, int HW, int C, int G, int nchunk,
                                                         int pix_per_chunk, float eps) {
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int cg = C / G;
    const double n = (double)HW * cg;
    double s = 0.0, sq = 0.0;
    for (int i = lane; i < nchunk * cg; i += 64) {
        const int ch = i / cg, c = g * cg + (i - ch * cg);
        const double ni = (double)max(min(HW, (ch + 1) * pix_per_chunk) - ch * pix_per_chunk, 0);      // pixels of chunk ch
        const float* src = partial + (((long)b * nchunk + ch) * C + c) * 2;
        const double mi = (double)src[0];
        s += ni * mi;
        sq += (double)src[1] + ni * mi * mi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        sq += __shfl_xor(sq, off);
    }
    const double mean = s / n;
    const double m2 = fmax(sq - s * mean, 0.0);      // M2 of the slice; fp64: the cancellation costs 2 log2(|mean| / std) of 53 bits
    const float rstd = (float)(1.0 / sqrt(m2 / n + (double)eps));
    for (int i = lane; i < cg; i += 64) {
        const int c = g * cg + i;
        const float sc = rstd * gamma[c];
        scale[(long)b * C + c] = sc;
        shift[(long)b * C + c] = (float)((double)beta[c] - mean * (double)sc);      // one rounding: mean * sc is what x * sc cancels against in the apply pass
    }
}

// ---- (3) apply: y = act(x*scale[b][c] + shift[b][c]) ------------------------------------------------------
template <typename T, bool SILU, bool PAIR = false>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       long nchunks_total, int HW, int C) {
    constexpr int EPC = DT<T>::EPC;
    const int cch = C / EPC;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nchunks_total; i += (long)gridDim.x * 256) {
        const long pix = i / cch;
        const int cc = (int)(i - pix * cch);
        const int b = (int)(pix / HW);
        const u32x4 v = *reinterpret_cast<const u32x4*>(x + i * EPC);
        float f[EPC];
        DT<T>::unpack(v, f);
        const float* sc = scale + (long)b * C + cc * EPC;
        const float* sh = shift + (long)b * C + cc * EPC;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            float t = f[e] * sc[e] + sh[e];
            if (SILU) t = silu_for<T>(t);          // bf16 activations: the fast form (common.h); fp32 (parity / split-bf16 modes): exact
            f[e] = t;
        }
        if constexpr (PAIR) store_pair4(reinterpret_cast<bf16*>(y), pix, C, cc * EPC, f);
        else *reinterpret_cast<u32x4*>(y + i * EPC) = DT<T>::pack(f);
    }
}

// ---- (3p) apply with PAIR output, 8 channels per thread (round 6): two 16-byte loads, two 16-byte stores (hi / lo).  The 4-channel form above
// stores 8 bytes per lane (measured on gfx950: 8-byte accesses run at 0.54-0.70 of the 16-byte rate) and, for T = float, evaluates SiLU with libm's
// expf + an IEEE division (~30 instructions per value: the kernel was VALU-bound, 25 % slower per byte than the statistics pass).  The pair form
// carries 16-17 significant bits, so SiLU is x * rcp(1 + exp2(-x log2 e)) here (v_exp_f32 / v_rcp_f32: ~1 ulp each, 2e-7 relative).
// C % 8 == 0 (a thread's 8 channels never straddle a 32-column block of the blocked layout).
// RAW (round 6, ffn_groupnorm_pair_raw): the same pass also writes the pair form of x ITSELF to yraw -- the operand of the ResBlock's 1x1 shortcut GEMM, which
// otherwise costs a ffn_split_pair pass (a second read of x) beside this one.
template <bool SILU, bool RAW = false>
__global__ __launch_bounds__(256) void gn_apply_pair8_kernel(const float* __restrict__ x, bf16* __restrict__ y, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, long n8_total, int HW, int C, bf16* __restrict__ yraw = nullptr) {
    const int cch = C / 8;
    const int lo_off = pair_lo(C);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8_total; i += (long)gridDim.x * 256) {
        const long pix = i / cch;
        const int c = (int)(i - pix * cch) * 8;
        const int b = (int)(pix / HW);
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + pix * C + c), v1 = *reinterpret_cast<const f32x4*>(x + pix * C + c + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(scale + (long)b * C + c), s1 = *reinterpret_cast<const f32x4*>(scale + (long)b * C + c + 4);
        const f32x4 h0 = *reinterpret_cast<const f32x4*>(shift + (long)b * C + c), h1 = *reinterpret_cast<const f32x4*>(shift + (long)b * C + c + 4);
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[e] = v0[e] * s0[e] + h0[e];
            f[4 + e] = v1[e] * s1[e] + h1[e];
        }
        if (SILU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = silu_fast(f[e]);
        }
        u32x4 hi, lo;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            hi[w] = pack_bf16x2(f[2 * w], f[2 * w + 1]);
            lo[w] = pack_bf16x2(f[2 * w] - __uint_as_float(hi[w] << 16), f[2 * w + 1] - __uint_as_float(hi[w] & 0xffff0000u));
        }
        bf16* q = y + pix * 2 * C + pair_pos(c, C);
        *reinterpret_cast<u32x4*>(q) = hi;
        *reinterpret_cast<u32x4*>(q + lo_off) = lo;
        if (RAW) {
            const float r[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                hi[w] = pack_bf16x2(r[2 * w], r[2 * w + 1]);
                lo[w] = pack_bf16x2(r[2 * w] - __uint_as_float(hi[w] << 16), r[2 * w + 1] - __uint_as_float(hi[w] & 0xffff0000u));
            }
            bf16* qr = yraw + pix * 2 * C + pair_pos(c, C);
            *reinterpret_cast<u32x4*>(qr) = hi;
            *reinterpret_cast<u32x4*>(qr + lo_off) = lo;
        }
    }
}

// ---- (3b) apply with fp8 output (FFN_FP8 convolutions): y8[pixel][Cp] = e4m3(act(x * scale + shift) * qs), channels C .. Cp-1 = 0.
// Cp (a multiple of 128) is the padded channel count the fp8 ping-pong conv needs; qs is the power-of-two activation scale.
template <bool SILU>
__global__ __launch_bounds__(256) void gn_apply_f8_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ y, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, long nchunks_total, int HW, int C, int Cp, float qs) {
    // one thread = 16 channels of one pixel: two 16-byte loads, ONE 16-byte store (8-byte stores ran this pass at 2.5 TB/s of real traffic)
    const int cch = Cp / 16;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nchunks_total; i += (long)gridDim.x * 256) {
        const long pix = i / cch;
        const int c0 = (int)(i - pix * cch) * 16;
        u32x4 o = u32x4{0u, 0u, 0u, 0u};
        if (c0 < C) {                                        // C % 16 == 0 is checked by the launcher
            const int b = (int)(pix / HW);
            const u32x4 v0 = *reinterpret_cast<const u32x4*>(x + pix * C + c0);
            const u32x4 v1 = *reinterpret_cast<const u32x4*>(x + pix * C + c0 + 8);
            float f[16];
            DT<bf16>::unpack(v0, f);
            DT<bf16>::unpack(v1, f + 8);
            const float* sc = scale + (long)b * C + c0;
            const float* sh = shift + (long)b * C + c0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float t = f[e] * sc[e] + sh[e];
                if (SILU) t = silu_fast(t);
                f[e] = t * qs;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) o[w] = pack_fp8x4(f[4 * w], f[4 * w + 1], f[4 * w + 2], f[4 * w + 3]);
        }
        *reinterpret_cast<u32x4*>(y + pix * Cp + c0) = o;
    }
}

// ---- fused GroupNorm for slices that one workgroup can own: grid (G, B), 1024 threads ----------------------------------
// pass 1: sum / sumsq of x - pivot over the (batch, group) slice [HW][cg] (element pairs, 4 or 8 bytes per load; the slice is L2 resident),
// block reduction (fp32 per thread, fp64 across threads), pass 2: y = act((x - mean) * rstd * gamma + beta).
template <typename T, bool SILU, bool PAIR = false>
__global__ __launch_bounds__(1024) void gn_fused_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int HW, int C, int G, float eps) {
    __shared__ double red[2][16];
    __shared__ float stat[3];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = C / G, hp = cg / 2;                      // channel pairs per pixel in this group
    const long base = (long)b * HW * C + (long)g * cg;
    const int npair = HW * hp;
    // sums of x - pivot (pivot = the thread's first element), moved to the slice's first element P in fp64: E[x^2] - mean^2 of the raw values loses
    // 2 log2(|mean| / std) bits of fp32 sums to cancellation (1.2e-5 of the output at mean = 16 std on a 50 x 2 slice)
    const float P = DT<T>::ld(x + base);
    float s = 0.f, ss = 0.f, pv = 0.f;
    int cnt = 0;
    for (int i = tid; i < npair; i += 1024) {
        const int px = i / hp, c2 = i - px * hp;
        const T* src = x + base + (long)px * C + 2 * c2;
        const float a = DT<T>::ld(src), c = DT<T>::ld(src + 1);
        if (i == tid) pv = a;
        const float da = a - pv, dc = c - pv;
        s += da + dc;
        ss += da * da + dc * dc;
        cnt += 2;
    }
    const double dl = (double)pv - (double)P;
    double ds = (double)s + cnt * dl, dss = (double)ss + 2.0 * dl * (double)s + cnt * dl * dl;      // sums of x - P and (x - P)^2 (cnt = 0: both 0)
    for (int off = 32; off > 0; off >>= 1) {
        ds += __shfl_xor(ds, off);
        dss += __shfl_xor(dss, off);
    }
    if (lane == 0) {
        red[0][wave] = ds;
        red[1][wave] = dss;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0, tt = 0;
        for (int w = 0; w < 16; ++w) {
            t += red[0][w];
            tt += red[1][w];
        }
        const double n = (double)HW * cg, rel = t / n, mean = (double)P + rel;
        double var = tt / n - rel * rel;
        if (var < 0) var = 0;
        stat[0] = (float)mean;
        stat[1] = (float)(1.0 / sqrt(var + (double)eps));
        stat[2] = (float)(mean - (double)stat[0]);           // the mean as hi + lo: rounded to one float it is off by up to 2^-24 |mean|, |mean| / std times the fp32 ulp of the result
    }
    __syncthreads();
    const float mean = stat[0], rstd = stat[1], mean_lo = stat[2];
    for (int i = tid; i < npair; i += 1024) {
        const int px = i / hp, c2 = i - px * hp;
        const int c = g * cg + 2 * c2;
        const long off = base + (long)px * C + 2 * c2;
        const float sc0 = rstd * gamma[c], sc1 = rstd * gamma[c + 1];
        float a = ((DT<T>::ld(x + off) - mean) - mean_lo) * sc0 + beta[c];           // the mean first: x * sc0 and mean * sc0 would each be rounded at |mean| / std times the result
        float d = ((DT<T>::ld(x + off + 1) - mean) - mean_lo) * sc1 + beta[c + 1];
        if (SILU) {
            a = silu_for<T>(a);
            d = silu_for<T>(d);
        }
        if constexpr (PAIR) {
            bf16* yp = reinterpret_cast<bf16*>(y);
            const long prow = ((long)b * HW + px) * 2 * C;
            const uint32_t hi = pack_bf16x2(a, d);
            *reinterpret_cast<uint32_t*>(yp + prow + pair_pos(c, C)) = hi;
            *reinterpret_cast<uint32_t*>(yp + prow + pair_pos(c, C) + pair_lo(C)) = pack_bf16x2(a - __uint_as_float(hi << 16), d - __uint_as_float(hi & 0xffff0000u));
        } else {
            DT<T>::st(y + off, a);
            DT<T>::st(y + off + 1, d);
        }
    }
}

// ---- LayerNorm over C per row; one wave per row, two-pass in registers --------------------------------------
template <typename T, int MAXCH, bool PAIR = false>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int M, int C, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= M) return;
    layernorm_row<T, MAXCH, PAIR>(x, (long)row, y, (long)row, gamma, beta, C, eps, lane);
}

// ---- row softmax (VAE mid-block single-head attention path: scores materialised once, 2 calls per image) ----
// in: fp32 or T scores [M][N] (already scaled), out: T probabilities.  One 256-thread block per row.
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const T* __restrict__ x, T* __restrict__ y, int N, float scale) {
    __shared__ float red[8];
    const long row = blockIdx.x;
    const T* xr = x + row * N;
    T* yr = y + row * N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = -1e30f;
    for (int i = tid; i < N; i += 256) m = fmaxf(m, DT<T>::ld(xr + i) * scale);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f;
    for (int i = tid; i < N; i += 256) s += expf(DT<T>::ld(xr + i) * scale - m);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) red[4 + wave] = s;
    __syncthreads();
    s = red[4] + red[5] + red[6] + red[7];
    const float inv = 1.0f / s;
    for (int i = tid; i < N; i += 256) DT<T>::st(yr + i, expf(DT<T>::ld(xr + i) * scale - m) * inv);
}
