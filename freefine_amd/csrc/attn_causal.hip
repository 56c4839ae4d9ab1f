// The text tower's unit of libfreefine_hip.so: the kernels only the CLIP text tower needs (attention_causal.h: attn_causal_kernel in its three
// arithmetic modes, embed_tokens_kernel), and the two small kernels behind the CLIP towers' projections (pool_layernorm_kernel, cosine_rows_kernel).
// Default code generation.  It exports the entries of its own kernels (ffn_embed_tokens, ffn_pool_layernorm, ffn_cosine_rows); attn_causal_kernel is
// planned and launched by ffn_attn (capi_attn.hip), which reaches it through fcausal_kernel (attn_units.h).
#include <limits.h>

#include "capi_common.h"
#include "attention_causal.h"
#include "layernorm_row.h"
#include "attn_units.h"

attn_kernel_t fcausal_kernel(int dtype) {
    return dtype == FFN_BF16 ? attn_causal_kernel<bf16, false> : (dtype == FFN_BF16X3 ? attn_causal_kernel<float, true> : attn_causal_kernel<float, false>);
}

// ---- token + position embedding of the text tower ------------------------------------------------------------------------
extern "C" int ffn_embed_tokens(void* stream, int dtype, const int* ids, const float* table, const float* pos, void* out, long M, int S, int C, int V) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16 || dtype == FFN_BF16X3, "embed_tokens: bad dtype %d", dtype);
    REQUIRE(ids && table && pos && out && aligned16(table) && aligned16(pos) && aligned16(out), "embed_tokens: null / unaligned pointer");
    REQUIRE(M > 0 && S > 0 && V > 0 && C > 0 && C % 4 == 0 && M < (1l << 31), "embed_tokens: bad shape M=%ld S=%d C=%d V=%d (C %% 4 == 0)", M, S, C, V);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n4 = M * (C / 4);
    if (dtype == FFN_BF16) LAUNCH(embed_tokens_kernel<bf16>, dim3(grid_for(n4)), dim3(256), 0, s, ids, table, pos, (bf16*)out, n4, S, C, V);
    else LAUNCH(embed_tokens_kernel<float>, dim3(grid_for(n4)), dim3(256), 0, s, ids, table, pos, (float*)out, n4, S, C, V);
    return check_launch("embed_tokens");
}

// ---- ffn_pool_layernorm: LayerNorm of ONE row per sequence -- row 0 (ids == nullptr: the image tower's class token) or the row at the first position holding
// the sequence's largest token id (open_clip's text pooling: the end-of-text token has the largest id).  One workgroup = one wave per sequence; the
// argmax is a wave reduction over S <= 128 ids (two per lane; the entry allows 96); the norm is layernorm_row.h layernorm_row, the routine of ffn_layernorm.
template <typename T, int MAXCH, bool PAIR>
__global__ __launch_bounds__(64) void pool_layernorm_kernel(const T* __restrict__ x, const int* __restrict__ ids, T* __restrict__ y,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int S, int C, float eps) {
    const int n = blockIdx.x, lane = threadIdx.x;
    int pos = 0;
    if (ids) {
        const int* row = ids + (long)n * S;
        int best = INT_MIN, at = INT_MAX;                  // (largest id, its first position) of this lane's positions, then of the wave
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = lane + 64 * i;
            if (q < S) {
                const int v = row[q];
                if (v > best) { best = v; at = q; }        // q ascends: an equal id later does not replace the first
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const int ob = __shfl_xor(best, off), oa = __shfl_xor(at, off);
            if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
        }
        pos = __builtin_amdgcn_readfirstlane(at);           // S >= 1: lane 0 holds position 0, so at < S
    }
    layernorm_row<T, MAXCH, PAIR>(x, (long)n * S + pos, y, (long)n, gamma, beta, C, eps, lane);
}

// dtype FFN_F32 / FFN_BF16; pair (fp32 input only): the pair rows of ffn_layernorm_pair.  MAXCH as ffn_layernorm chooses it.
extern "C" int ffn_pool_layernorm(void* stream, int dtype, const void* x, const int* ids, void* y, const float* gamma, const float* beta, int N, int S, int C,
                                  float eps, int pair) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "pool_layernorm: bad dtype %d", dtype);
    REQUIRE(pair == 0 || (pair == 1 && dtype == FFN_F32), "pool_layernorm: pair output takes fp32 input (dtype %d, pair %d)", dtype, pair);
    REQUIRE(x && y && gamma && beta, "pool_layernorm: null pointer");
    REQUIRE(aligned16(x) && aligned16(y) && (reinterpret_cast<uintptr_t>(ids) & 3) == 0, "pool_layernorm: x, y must be 16-byte aligned, ids 4-byte aligned");
    const int epc = dtype == FFN_F32 ? 4 : 8;
    REQUIRE(N > 0 && S > 0 && C > 0 && C % epc == 0 && C / epc <= 64 * 6, "pool_layernorm: bad shape N=%d S=%d C=%d (C %% %d == 0, C <= %d)", N, S, C, epc,
            64 * 6 * epc);
    REQUIRE(!ids || S <= 96, "pool_layernorm: S=%d ids per sequence (at most 96)", S);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cch = C / epc;
#define POOL_LN(T, MAXCH, PAIR) LAUNCH((pool_layernorm_kernel<T, MAXCH, PAIR>), dim3((unsigned)N), dim3(64), 0, s, (const T*)x, ids, (T*)y, gamma, beta, S, C, eps)
    if (dtype == FFN_BF16) {
        if (cch <= 128) POOL_LN(bf16, 2, false);
        else POOL_LN(bf16, 6, false);
    } else if (pair) {
        if (cch <= 128) POOL_LN(float, 2, true);
        else POOL_LN(float, 6, true);
    } else {
        if (cch <= 128) POOL_LN(float, 2, false);
        else POOL_LN(float, 6, false);
    }
#undef POOL_LN
    return check_launch("pool_layernorm");
}

// ---- ffn_cosine_rows: out[i] = <a_i, b_j> / (max(|a_i|, 1e-12) max(|b_j|, 1e-12)), j = i or 0 (one b row for all): the cosine of F.normalize'd rows.
// One wave per row, four rows per workgroup.  A lane sums the products of its 16-byte chunks (lane, lane + 64, ...) in order, then the three sums go
// through a fixed xor tree: no atomics, the same bits every run.
__global__ __launch_bounds__(256) void cosine_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int B, int P,
                                                          int b_rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* ar = a + (long)row * P;
    const float* br = b + (b_rows == 1 ? 0l : (long)row * P);
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int c = lane * 4; c < P; c += 256) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(ar + c), v = *reinterpret_cast<const f32x4*>(br + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ab += u[e] * v[e];
            aa += u[e] * u[e];
            bb += v[e] * v[e];
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        ab += __shfl_xor(ab, off);
        aa += __shfl_xor(aa, off);
        bb += __shfl_xor(bb, off);
    }
    if (lane == 0) out[row] = ab / (fmaxf(sqrtf(aa), 1e-12f) * fmaxf(sqrtf(bb), 1e-12f));
}

extern "C" int ffn_cosine_rows(void* stream, const float* a, const float* b, float* out, int B, int P, int b_rows) {
    REQUIRE(a && b && out, "cosine_rows: null pointer");
    REQUIRE(aligned16(a) && aligned16(b) && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "cosine_rows: a, b must be 16-byte aligned, out 4-byte aligned");
    REQUIRE(B > 0 && P > 0 && P % 4 == 0, "cosine_rows: bad shape B=%d P=%d (P %% 4 == 0)", B, P);
    REQUIRE(b_rows == 1 || b_rows == B, "cosine_rows: b has %d rows (1 or B=%d)", b_rows, B);
    LAUNCH(cosine_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, b, out, B, P, b_rows);
    return check_launch("cosine_rows");
}
