// attn_causal_kernel: causal self attention over a SHORT sequence (FFN_ATT_CAUSAL: key k is allowed for query q iff k <= q; S == Sk <= 96, head dim 64,
// one pass) -- the attention of the CLIP text tower (77 tokens; transformers' CLIPTextModel as the reference calls it, /root/reference/src/demo/model.py:536-567),
// in all three arithmetic modes:
//   <float, false>  FFN_F32     exact fp32 products on v_mfma_f32_16x16x4_f32, fp32 softmax
//   <bf16,  false>  FFN_BF16    bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 softmax and accumulation (P rounded to bf16 for the second product)
//   <float, true>   FFN_BF16X3  fp32 operands split hi / lo in registers, three bf16 MFMAs per product term (small terms first), P split like the
//                               attn_x3* kernels; fp32 rows or (out_pair) the pair rows the out projection's split-bf16 GEMM reads
// Formulation = attention.h's: S^T = K . Q^T, so a lane owns ONE query (column lane & 15) and four keys (16 f + 4 (lane >> 4) + r) of every 16-key fragment f;
// the exponentiated P^T fragments are the B operand of O^T = V^T . P^T as they stand.
// Work split: one workgroup per (row, head), one WAVE per 16 queries (ceil(S / 16) <= 6 waves).  K (<= 96 x 64) and V^T (64 x <= 96) of a (row, head) are 48 KiB at
// most and stay in L2 / the vector cache for the workgroup's waves, which read their fragments straight into registers: no LDS, no barrier, no key loop ring.
// Wave w needs key fragments 0 .. w only -- fragments wholly above the diagonal are never loaded or multiplied; the diagonal fragment f == w is masked before the
// row maximum.  Key 0 is allowed for every query, so no row is empty.  V^T columns at or beyond Sk (row padding, ldvt > Sk) are replaced by zeros in registers
// and columns at or beyond ldvt are never read.
#pragma once
#include "attention_x3.h"

template <typename T, bool X3>
__global__ __launch_bounds__(384) void attn_causal_kernel(const AttnParams p) {
    constexpr bool F32 = std::is_same<T, float>::value && !X3;
    constexpr int NF = 6;                              // key fragments of 16 (Sk <= 96)
    constexpr int NQ = F32 ? 4 : 2;                    // contraction steps over the head dim: 16 fp32 / 32 bf16 elements each
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x / p.heads, head = blockIdx.x - b * p.heads;
    const int l15 = lane & 15, g = lane >> 4;
    const AttnEntry& e = p.e[b];
    const int q = 16 * w + l15;                        // this lane's query (also: the key / head-dim row it loads as an A operand is 16 f + l15)
    const bool qok = q < p.S;
    const int C = p.heads * 64;
    const u32x4 zero4 = u32x4{0u, 0u, 0u, 0u};
    const f32x4 zerof = f32x4{0.f, 0.f, 0.f, 0.f};

    if (ATT_ENTRY_SKIPPED(e)) {               // skipped entry: the row's sum over passes is empty
        if (qok) {
            const float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int df = 0; df < 4; ++df) {
                const int col = head * 64 + 16 * df + 4 * g;
                if (X3 && p.out_pair) store_pair_row4(reinterpret_cast<bf16*>(p.out) + ((long)b * p.S + q) * p.ldo, col, p.ldo / 2, z);
                else store4(reinterpret_cast<T*>(p.out) + ((long)b * p.S + q) * p.ldo + col, z);
            }
        }
        return;
    }

    const T* __restrict__ Q = reinterpret_cast<const T*>(p.q) + ((long)e.q_row * p.S + (qok ? q : 0)) * p.ldq + head * 64;
    const T* __restrict__ K = reinterpret_cast<const T*>(p.k) + (long)e.kv_row * p.Sk * p.ldk + head * 64;
    const T* __restrict__ V = reinterpret_cast<const T*>(p.vt) + ((long)e.kv_row * C + head * 64) * p.ldvt;
    auto ld16 = [&](const T* ptr, bool ok) { return ok ? *reinterpret_cast<const u32x4*>(ptr) : zero4; };

    // ---- Q fragments of this wave's 16 queries -----------------------------------------------------------------------------------------------
    u32x4 qh[NQ], ql[X3 ? NQ : 1];
#pragma unroll
    for (int ks = 0; ks < NQ; ++ks) {
        if constexpr (X3) {
            const u32x4 a = ld16(Q + 32 * ks + 8 * g, qok), c = ld16(Q + 32 * ks + 8 * g + 4, qok);
            x3_split8(__builtin_bit_cast(f32x4, a), __builtin_bit_cast(f32x4, c), qh[ks], ql[ks]);
        } else {
            qh[ks] = ld16(Q + (F32 ? 16 * ks + 4 * g : 32 * ks + 8 * g), qok);
        }
    }

    // ---- S^T fragments 0 .. w: lane holds S^T[key 16 f + 4 g + r][query q] -----------------------------------------------------------------------
    f32x4 st[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        st[f] = zerof;
        if (f <= w) {
            const int key = 16 * f + l15;
            const bool kok = key < p.Sk;
            const T* kr = K + (long)(kok ? key : 0) * p.ldk;
#pragma unroll
            for (int ks = 0; ks < NQ; ++ks) {
                if constexpr (X3) {
                    const u32x4 a = ld16(kr + 32 * ks + 8 * g, kok), c = ld16(kr + 32 * ks + 8 * g + 4, kok);
                    u32x4 kh, kl;
                    x3_split8(__builtin_bit_cast(f32x4, a), __builtin_bit_cast(f32x4, c), kh, kl);
                    x3_mma(kl, qh[ks], st[f]);         // small terms first
                    x3_mma(kh, ql[ks], st[f]);
                    x3_mma(kh, qh[ks], st[f]);
                } else {
                    DT<T>::mma(ld16(kr + (F32 ? 16 * ks + 4 * g : 32 * ks + 8 * g), kok), qh[ks], st[f]);
                }
            }
            if (f == w) {                              // the diagonal fragment (keys at or beyond Sk = S lie above every valid query as well)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * f + 4 * g + r > q) st[f][r] = -__builtin_inff();
            }
        }
    }

    // ---- fp32 softmax over the allowed keys of the lane's query (its four key groups sit on lanes l15, l15 + 16, + 32, + 48) ----------------------------
    const float c = p.scale * 1.44269504088896340736f;
    float m = st[0][0];                                // (-inf where 4 g > q: key 0 on group 0 keeps the combined maximum finite)
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (f <= w) {
            if (f) m = att_max(m, st[f][0]);
            m = att_max3(m, st[f][1], st[f][2]);
            m = att_max(m, st[f][3]);
        }
    m = att_max_groups(m);
    const float mc = -m * c;
    float l = 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (f <= w) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(st[f][r], c, mc));      // exp2(-inf) = 0 on the masked keys
                st[f][r] = pv;
                l += pv;
            }
        }
    {
        auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
        l = __uint_as_float(a[0]) + __uint_as_float(a[1]);
        auto d2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(l), __float_as_uint(l), false, false);
        l = __uint_as_float(d2[0]) + __uint_as_float(d2[1]);
    }
    const float sc = e.w_const / l;

    // ---- O^T = V^T . P^T: lane holds O^T[d 16 df + 4 g + r][query q] = four consecutive columns of the query's output row -------------------------------
    // V^T A operand of head-dim fragment df: row 16 df + l15; fp32: keys 16 f + 4 g + i of fragment f; bf16 / split-bf16: keys {32 s + 4 g + i, 32 s + 16 + 4 g + i}
    // of the fragment pair s -- the order in which the lane holds P
    u32x4 ph[F32 ? 1 : NF / 2], pl[X3 ? NF / 2 : 1];
    if constexpr (!F32) {
#pragma unroll
        for (int s = 0; s < NF / 2; ++s) {
            const f32x4 hi2 = 2 * s + 1 <= w ? st[2 * s + 1] : zerof;
            if constexpr (X3) {
                x3_split8(st[2 * s], hi2, ph[s], pl[s]);
            } else {
                ph[s] = u32x4{pack_bf16x2(st[2 * s][0], st[2 * s][1]), pack_bf16x2(st[2 * s][2], st[2 * s][3]), pack_bf16x2(hi2[0], hi2[1]), pack_bf16x2(hi2[2], hi2[3])};
            }
        }
    }
    // four V^T values of keys k0 .. k0 + 3 of row `vr` as floats: zeros at or beyond Sk (padding must not reach the result), nothing read at or beyond ldvt
    auto ldv4 = [&](const T* vr, int k0, float* v) {
        if (k0 < p.ldvt) load4(vr + k0, v);
        else v[0] = v[1] = v[2] = v[3] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (k0 + i >= p.Sk) v[i] = 0.f;
    };
#pragma unroll
    for (int df = 0; df < 4; ++df) {
        const T* vr = V + (long)(16 * df + l15) * p.ldvt;
        f32x4 o = zerof;
        if constexpr (F32) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
                if (f <= w) {
                    float v[4];
                    ldv4(vr, 16 * f + 4 * g, v);
                    DT<float>::mma(DT<float>::pack(v), __builtin_bit_cast(u32x4, st[f]), o);
                }
        } else {
#pragma unroll
            for (int s = 0; s < NF / 2; ++s)
                if (2 * s <= w) {
                    float v0[4], v1[4];
                    ldv4(vr, 32 * s + 4 * g, v0);
                    ldv4(vr, 32 * s + 16 + 4 * g, v1);
                    if constexpr (X3) {
                        u32x4 vh, vl;
                        x3_split8(f32x4{v0[0], v0[1], v0[2], v0[3]}, f32x4{v1[0], v1[1], v1[2], v1[3]}, vh, vl);
                        x3_mma(vl, ph[s], o);
                        x3_mma(vh, pl[s], o);
                        x3_mma(vh, ph[s], o);
                    } else {
                        const u32x4 vb = u32x4{pack_bf16x2(v0[0], v0[1]), pack_bf16x2(v0[2], v0[3]), pack_bf16x2(v1[0], v1[1]), pack_bf16x2(v1[2], v1[3])};
                        DT<bf16>::mma(vb, ph[s], o);
                    }
                }
        }
        if (qok) {
            const float v[4] = {o[0] * sc, o[1] * sc, o[2] * sc, o[3] * sc};
            const int col = head * 64 + 16 * df + 4 * g;
            if (X3 && p.out_pair) store_pair_row4(reinterpret_cast<bf16*>(p.out) + ((long)b * p.S + q) * p.ldo, col, p.ldo / 2, v);
            else store4(reinterpret_cast<T*>(p.out) + ((long)b * p.S + q) * p.ldo + col, v);
        }
    }
}

// ---- token + position embedding lookup of the text tower: out[m] = table[ids[m]] + pos[m % S] (fp32 add), four columns per thread --------------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int* __restrict__ ids, const float* __restrict__ table, const float* __restrict__ pos,
                                                           T* __restrict__ out, long n4, int S, int C, int V) {
    const int c4 = C / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const long m = i / c4;
        const int c = (int)(i - m * c4) * 4;
        const int id = ids[m];
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4];
        if ((unsigned)id < (unsigned)V) load4(table + (long)id * C + c, a);      // (the host refuses ids outside the table before upload)
        load4(pos + (long)(m % S) * C + c, b);
        const float v[4] = {a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]};
        store4(out + m * C + c, v);
    }
}
