// The row routine of every LayerNorm entry, in a header of its own so that translation units beside capi.hip can use it (norms.h defines kernels that are no
// templates: it can be part of one unit only).  ffn_layernorm / ffn_layernorm_pair (norms.h layernorm_kernel) and ffn_pool_layernorm (attn_causal.hip) all
// call layernorm_row: the same loads, sums and affine step, so the same bits.
#pragma once
#include "common.h"

// PAIR output (split-bf16 mode, T = float): the normalised row is written in the bf16 pair form an FFN_BF16X3 GEMM reads as its A operand
// (hi = bf16(v), lo = bf16(v - hi); blocked layout: common.h pair_pos) instead of fp32 -- same bytes, and the separate ffn_split_pair pass disappears.
__device__ __forceinline__ void store_pair4(bf16* yp, long row, int C, int c, const float* f) {
    u32x2 hi, lo;
    hi[0] = pack_bf16x2(f[0], f[1]);
    hi[1] = pack_bf16x2(f[2], f[3]);
    lo[0] = pack_bf16x2(f[0] - __uint_as_float(hi[0] << 16), f[1] - __uint_as_float(hi[0] & 0xffff0000u));
    lo[1] = pack_bf16x2(f[2] - __uint_as_float(hi[1] << 16), f[3] - __uint_as_float(hi[1] & 0xffff0000u));
    bf16* q = yp + row * 2 * C + pair_pos(c, C);
    *reinterpret_cast<u32x2*>(q) = hi;
    *reinterpret_cast<u32x2*>(q + pair_lo(C)) = lo;
}

// layernorm_row: one wave normalises row `row` of x [.][C] and writes it as row `orow` of y.  The routine of every LayerNorm entry (ffn_layernorm,
// ffn_layernorm_pair, and ffn_pool_layernorm in attn_causal.hip, whose row is gathered): the same loads, sums and affine step, so the same bits.
// TO (ffn_embed_tokens_ln: T = float, TO = bf16): the output's element type where it differs from the input's; the four values of a chunk go out as one 8-byte store.
template <typename T, int MAXCH, bool PAIR = false, typename TO = T>  // MAXCH = max 16-byte chunks per lane
__device__ __forceinline__ void layernorm_row(const T* x, long row, TO* y, long orow, const float* gamma, const float* beta, int C, float eps, int lane) {
    constexpr int EPC = DT<T>::EPC;
    const int cch = C / EPC;
    float f[MAXCH][EPC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int cc = lane + 64 * i;
        if (cc < cch) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(x + row * C + cc * EPC);
            DT<T>::unpack(v, f[i]);
#pragma unroll
            for (int e = 0; e < EPC; ++e) s += f[i][e];
        }
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int cc = lane + 64 * i;
        if (cc < cch) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
#pragma clang fp contract(off)      // d * d rounded, then added: where the compiler fuses the two depends on how the routine is inlined, and the fused sum has other bits
                const float d = f[i][e] - mean;
                ss += d * d;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    const float rstd = 1.0f / sqrtf(ss / (float)C + eps);
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int cc = lane + 64 * i;
        if (cc < cch) {
            float o[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const int c = cc * EPC + e;
                o[e] = (f[i][e] - mean) * rstd * gamma[c] + beta[c];
            }
            if constexpr (PAIR) store_pair4(reinterpret_cast<bf16*>(y), orow, C, cc * EPC, o);
            else if constexpr (sizeof(TO) == sizeof(T)) *reinterpret_cast<u32x4*>(y + orow * C + cc * EPC) = DT<T>::pack(o);
            else store4(y + orow * C + cc * EPC, o);
        }
    }
}
