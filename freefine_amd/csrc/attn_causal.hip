// The text tower's unit of libfreefine_hip.so: the kernels only the CLIP text tower needs (attention_causal.h: attn_causal_kernel in its three
// arithmetic modes, embed_tokens_kernel), and the two small kernels behind the CLIP towers' projections (pool_layernorm_kernel, cosine_rows_kernel).
// Default code generation.  It exports the entries of its own kernels (ffn_embed_tokens, ffn_pool_layernorm, ffn_cosine_rows); attn_causal_kernel is
// planned and launched by ffn_attn (capi_attn.hip), which reaches it through fcausal_kernel (attn_units.h).  The two small kernels of the ImageReward score's
// BERT live here too, beside the lookup and the row norm they build on (ffn_embed_tokens_ln, ffn_affine_chain).
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

// ---- ffn_embed_tokens_ln: y[m] = LayerNorm(table[ids[m]] + pos[m % S]) -- BERT's embedding (BLIP's text encoder), whose LayerNorm sits behind the lookup.
// One wave per row, four rows per workgroup.  A lane forms the fp32 sums of its own 16-byte chunks (lane, lane + 64, ...: layernorm_row's chunks) exactly as
// embed_tokens_kernel does and parks them in its wave's LDS row; layernorm_row then reads that row, so every lane reads back only what it wrote itself (no
// barrier) and the fp32 result has the bits of ffn_layernorm(ffn_embed_tokens(..., FFN_F32)).
template <typename T, int MAXCH>
__global__ __launch_bounds__(256) void embed_tokens_ln_kernel(const int* __restrict__ ids, const float* __restrict__ table, const float* __restrict__ pos,
                                                              T* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta, int M, int S,
                                                              int C, int V, float eps) {
    __shared__ __attribute__((aligned(16))) float rowbuf[4][MAXCH * 64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x * 4 + wave;
    if (m >= M) return;
    const int id = ids[m], cch = C / 4;
    const float* prow = pos + (long)(m % S) * C;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int cc = lane + 64 * i;
        if (cc < cch) {
            float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4];
            if ((unsigned)id < (unsigned)V) load4(table + (long)id * C + cc * 4, a);      // (the host refuses ids outside the table before upload)
            load4(prow + cc * 4, b);
            const float v[4] = {a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]};
            store4(&rowbuf[wave][cc * 4], v);
        }
    }
    layernorm_row<float, MAXCH, false, T>(rowbuf[wave], 0l, y, (long)m, gamma, beta, C, eps, lane);
}

extern "C" int ffn_embed_tokens_ln(void* stream, int dtype, const int* ids, const float* table, const float* pos, void* out, const float* gamma, const float* beta,
                                   long M, int S, int C, int V, float eps) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "embed_tokens_ln: bad dtype %d", dtype);
    REQUIRE(ids && table && pos && out && gamma && beta && aligned16(table) && aligned16(pos) && aligned16(out) && (reinterpret_cast<uintptr_t>(ids) & 3) == 0,
            "embed_tokens_ln: null / unaligned pointer");
    const int epc = dtype == FFN_F32 ? 4 : 8;
    REQUIRE(M > 0 && S > 0 && V > 0 && C > 0 && C % epc == 0 && C / 4 <= 64 * 6 && M < (1l << 31) - 4,
            "embed_tokens_ln: bad shape M=%ld S=%d C=%d V=%d (C %% %d == 0, C <= %d)", M, S, C, V, epc, 64 * 6 * 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((M + 3) / 4));
#define EMBED_LN(T, MAXCH) LAUNCH((embed_tokens_ln_kernel<T, MAXCH>), grid, dim3(256), 0, s, ids, table, pos, (T*)out, gamma, beta, (int)M, S, C, V, eps)
    if (dtype == FFN_BF16) {
        if (C / 4 <= 128) EMBED_LN(bf16, 2);
        else EMBED_LN(bf16, 6);
    } else {
        if (C / 4 <= 128) EMBED_LN(float, 2);
        else EMBED_LN(float, 6);
    }
#undef EMBED_LN
    return check_launch("embed_tokens_ln");
}

// ---- ffn_affine_chain: out[b] = ((W_L ( ... (W_1 x_b + b_1) ... ) + b_L) - shift) / scale, layer after layer (ImageReward's reward head: five Linears with
// nothing but dropout between them).  One workgroup of sixteen waves per row; the activations ping-pong between two LDS rows.  A wave takes four neighbouring
// outputs at a time (four independent sums over one read of the activations: the loads of a step do not wait for each other).  For EVERY output, lane j sums
// the products k = j, j + 64, ... in ascending order, the 64 partial sums go through a fixed xor tree, the bias is added last.  That order depends on neither
// B nor the row nor which wave owns the output: deterministic, and equal rows give equal bits.  Scalar loads and stores: widths and offsets need no alignment.
struct AffineChain {
    int L, dims[FFN_CHAIN_MAXL + 1];
};
constexpr int CHAIN_WAVES = 16, CHAIN_OUTS = 4;
__global__ __launch_bounds__(64 * CHAIN_WAVES) void affine_chain_kernel(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ out,
                                                                        AffineChain c, int ldx, float shift, float scale) {
    __shared__ float act[2][FFN_CHAIN_MAXW];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < c.dims[0]; k += 64 * CHAIN_WAVES) act[0][k] = x[(long)b * ldx + k];
    __syncthreads();
    const float* w = params;
    int cur = 0;
    for (int l = 0; l < c.L; ++l) {
        const int K = c.dims[l], N = c.dims[l + 1];
        const float* bias = w + (long)N * K;
        const bool last = l == c.L - 1;
        for (int n0 = wave * CHAIN_OUTS; n0 < N; n0 += CHAIN_WAVES * CHAIN_OUTS) {      // (uniform per wave: every lane reaches the shuffles)
            const float* wr[CHAIN_OUTS];
#pragma unroll
            for (int j = 0; j < CHAIN_OUTS; ++j) wr[j] = w + (long)(n0 + j < N ? n0 + j : N - 1) * K;      // past the last output: its row again, never stored
            float s[CHAIN_OUTS] = {0.f, 0.f, 0.f, 0.f};
            for (int k = lane; k < K; k += 64) {
                const float a = act[cur][k];
#pragma unroll
                for (int j = 0; j < CHAIN_OUTS; ++j) s[j] += wr[j][k] * a;
            }
#pragma unroll
            for (int j = 0; j < CHAIN_OUTS; ++j)
                for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_xor(s[j], off);
            if (lane < CHAIN_OUTS && n0 + lane < N) {
                const int n = n0 + lane;
                float v = s[0];
#pragma unroll
                for (int j = 1; j < CHAIN_OUTS; ++j) v = lane == j ? s[j] : v;
                v += bias[n];
                if (last) out[(long)b * N + n] = (v - shift) / scale;
                else act[cur ^ 1][n] = v;
            }
        }
        __syncthreads();
        w = bias + N;
        cur ^= 1;
    }
}

extern "C" int ffn_affine_chain(void* stream, const float* x, const float* params, float* out, int B, int ldx, const int* dims, int L, float shift, float scale) {
    REQUIRE(x && params && out && dims, "affine_chain: null pointer");
    REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, "affine_chain: x, params, out must be 4-byte aligned");
    REQUIRE(L >= 1 && L <= FFN_CHAIN_MAXL, "affine_chain: L=%d layers (1 .. %d)", L, FFN_CHAIN_MAXL);
    AffineChain c;
    c.L = L;
    for (int l = 0; l <= FFN_CHAIN_MAXL; ++l) c.dims[l] = l <= L ? dims[l] : 0;
    for (int l = 0; l <= L; ++l) REQUIRE(c.dims[l] >= 1 && c.dims[l] <= FFN_CHAIN_MAXW, "affine_chain: width %d of layer boundary %d (1 .. %d)", c.dims[l], l, FFN_CHAIN_MAXW);
    REQUIRE(B > 0 && ldx >= c.dims[0], "affine_chain: bad shape B=%d ldx=%d (ldx >= %d)", B, ldx, c.dims[0]);
    REQUIRE(scale != 0.f && scale == scale && shift == shift, "affine_chain: shift / scale must be numbers, scale non-zero");
    LAUNCH(affine_chain_kernel, dim3((unsigned)B), dim3(64 * CHAIN_WAVES), 0, reinterpret_cast<hipStream_t>(stream), x, params, out, c, ldx, shift, scale);
    return check_launch("affine_chain");
}
