// The attention entries of libfreefine_hip.so (ffn_attn*): the one plan of which kernel runs (attn_plan) and the launches (kernels: the attention*.h
// headers; attn_x3w_kernel and attn_causal_kernel are compiled in units of their own and reached through attn_units.h).  Host-side launch glue only.
#include <stdio.h>

#include "capi_common.h"
#include "attention.h"
#include "attention_pp.h"
#include "attention_x.h"
#include "attention_x3.h"
#include "attention_x3p.h"
#include "attention_xx3.h"
#include "attn_units.h"

// attn_kernel's instantiations (attention.h), by head dim: the first row whose padded head dim DP >= D (the last row also answers
// ffn_attn_variant for larger D, which ffn_attn refuses)
struct AttnTile { int dp, qf, kt, occ; };      // padded head dim, 16-query fragments per wave, keys per tile, workgroups per CU
static const AttnTile kAttnTileF32[] = {{48, 2, 64, 1}, {64, 2, 64, 1}, {80, 2, 64, 1}, {160, 1, 32, 1}};
static const AttnTile kAttnTileBf16[] = {{64, 2, 64, 2}, {96, 2, 64, 1}, {160, 1, 64, 1}};
static AttnTile attn_tile(bool f32, int D) {
    const AttnTile* t = f32 ? kAttnTileF32 : kAttnTileBf16;
    const int n = f32 ? 4 : 3;
    int i = 0;
    while (i + 1 < n && D > t[i].dp) ++i;
    return t[i];
}
extern "C" int ffn_attn_variant(int dtype, int D, int* dp, int* qf) {
    REQUIRE(dp && qf, "attn_variant: null argument");
    const AttnTile t = attn_tile(dtype == FFN_F32, D);
    *dp = t.dp;
    *qf = t.qf;
    return FFN_OK;
}

enum AttnKind { ATT_KERNEL, ATT_PP, ATT_X, ATT_X_MP, ATT_X3, ATT_X3P, ATT_X3W, ATT_XX3, ATT_CAUSAL_K };
struct AttnPlan {
    AttnKind kind;
    bool f32;           // ATT_KERNEL: fp32 (else bf16) operands
    bool masks;         // the instantiation for launches with key masks
    AttnTile tile;      // ATT_KERNEL
    int nkf, nw;        // xattn*: 16-key fragments; waves that share a workgroup's work split (xattn_kernel: 1, its waves work alone)
    int lds;
    dim3 grid, block;   // (xattn*: the grid depends on the CU count and is set at launch)
};
// The one statement of which kernel ffn_attn launches for a descriptor: ffn_attn launches from it, ffn_attn_kernel_name spells it.
//   FFN_BF16X3, D <= 64 (split-bf16 arithmetic on fp32 operands):
//     xattn_x3_kernel (attention_xx3.h) for short unmasked key sequences (the text cross attention) whose fragment images fit the LDS;
//     else on the ping-pong preconditions (D = 64, Sk % 64 == 0, S >= 128, no degenerate uniform-softmax entry): attn_x3w_kernel
//     (attention_x3w.h) on pre-split K / V^T images (kv_pair), attn_x3p_kernel (attention_x3p.h) on fp32 K / V^T;
//     else attn_x3_kernel (attention_x3.h).
//   FFN_BF16: xattn_kernel / xattn_mp_kernel (attention_x.h) for short unmasked key sequences; attn_pp_kernel (attention_pp.h) on the
//     ping-pong preconditions; else attn_kernel (attention.h).
//   FFN_F32, and FFN_BF16X3 with larger heads: the exact fp32 attn_kernel.
//   Any dtype, an active entry carrying FFN_ATT_CAUSAL: attn_causal_kernel (attention_causal.h) under the flag's preconditions, FFN_EINVAL outside them; a
//     descriptor without the flag never reaches that branch.
// FFN_EINVAL: kv_pair for a launch that does not run attn_x3w_kernel; FFN_ENOSYS: head dim beyond 160.
// The dynamic LDS of a launch is its kernel's own size function, stated beside the kernel from the constants it uses (attn_kernel_lds, attn_pp_lds_bytes,
// attn_x3_lds_bytes, attn_x3p_lds_bytes, xattn_mp_lds_bytes, xattn_x3_lds_bytes; attn_x3w_lds_bytes through fx3w_lds_bytes) and checked there against the layout.
static int attn_plan(int dtype, const ffn_attn_desc& d, AttnPlan* p) {
    bool masks = false, uniform = false, xok = true, multi = d.npass != 1;
    bool causal = false, causal_ok = true;
    int maxq = 0, maxkv = 0;
    for (int pi = 0; pi < d.npass; ++pi)
        for (int b = 0; b < d.Bo; ++b) {
            const ffn_attn_entry& e = d.e[pi * FFN_ATT_MAXB + b];
            if (ATT_ENTRY_SKIPPED(e)) { multi = true; continue; }
            causal |= (e.flags & FFN_ATT_CAUSAL) != 0;
            causal_ok &= (e.flags & FFN_ATT_CAUSAL) && !e.kmask && !e.qsel && !e.wq && e.w_slope == 0.f;
            masks |= e.kmask != nullptr;
            uniform |= e.kmask != nullptr && (e.flags & (FFN_ATT_UNIFORM_SEL1 | FFN_ATT_UNIFORM_SEL0));
            xok &= !e.kmask && !e.qsel && (e.w_slope == 0.f || d.w_dev);      // (flags only qualify a key mask)
            multi |= e.wq != nullptr;
            maxq = e.q_row > maxq ? e.q_row : maxq;
            maxkv = e.kv_row > maxkv ? e.kv_row : maxkv;
        }
    const bool pp = d.D == 64 && d.Sk % 64 == 0 && d.S >= 128 && !uniform;
    // the short-key kernels: D = 64, Sk <= 96, 32-bit byte offsets into every operand (esz = bytes per operand element); key-fragment count
    auto xattn_nkf = [&](int esz) {
        const long lim = (1l << 31) - 65536;
        if (!xok || d.D != 64 || d.Sk > 96 || (esz == 2 && d.ldo % 8 != 0) || (long)(maxq + 1) * d.S * d.ldq * esz >= lim ||
            (long)d.Bo * d.S * d.ldo * esz >= lim || (long)(maxkv + 1) * d.Sk * d.ldk * esz >= lim || (long)(maxkv + 1) * d.heads * 64 * d.ldvt * esz >= lim)
            return 0;
        const int need = (d.Sk + 15) / 16;
        return need <= 2 ? 2 : (need <= 5 ? 5 : 6);
    };
    *p = AttnPlan{};
    if (causal) {
        REQUIRE(causal_ok && d.npass == 1 && d.S == d.Sk && d.Sk <= 96 && d.D == 64 && !d.kv_pair && d.scale > 0.f,
                "attn: FFN_ATT_CAUSAL needs S == Sk <= 96, D = 64, one pass, kv_pair = 0, scale > 0 and on every active entry the flag and no kmask / qsel / wq / "
                "w_slope (S=%d, Sk=%d, D=%d, npass=%d, kv_pair=%d)", d.S, d.Sk, d.D, d.npass, d.kv_pair);
        p->kind = ATT_CAUSAL_K;
        p->grid = dim3(d.Bo * d.heads);                        // one workgroup per (row, head), one wave per 16 queries
        p->block = dim3(64 * ((d.S + 15) / 16));
        return FFN_OK;
    }
    p->masks = masks;
    p->grid = dim3(((d.S + 255) / 256) * d.heads * d.Bo);      // the 256-query workgroups of the ping-pong and split-bf16 kernels
    p->block = dim3(512);
    if (dtype == FFN_BF16X3 && d.D <= 64) {
        p->nkf = xattn_nkf(4);
        if (p->nkf && xattn_x3_lds_bytes(p->nkf, d.npass) <= ATT_LDS_MAX) {
            // 8 waves per workgroup where the fragment images are large against a workgroup's share of the queries (two passes: 88 KiB, one workgroup
            // per CU either way) or the launch is long; 4 (two workgroups per CU) for the short single-pass launches (profiles/r5_xattn_x3_waves_and_stores.txt)
            p->kind = ATT_XX3;
            p->nw = (d.npass >= 2 || d.S >= 4096) ? 8 : 4;
            p->lds = xattn_x3_lds_bytes(p->nkf, d.npass);
            p->block = dim3(64 * p->nw);
        } else if (pp && d.kv_pair) {                           // one wave per SIMD on 32x32x16 MFMAs
            p->kind = ATT_X3W;
            p->lds = fx3w_lds_bytes();
            p->block = dim3(256);
        } else if (pp) {
            p->kind = ATT_X3P;
            p->lds = attn_x3p_lds_bytes();
        } else {
            p->kind = ATT_X3;
            p->lds = attn_x3_lds_bytes();
        }
    } else if (dtype == FFN_BF16 && (p->nkf = xattn_nkf(2))) {
        // one pass of plain active entries: K / V^T of a (row, head) in a wave's registers; several passes, skipped entries or per-query
        // weights: one workgroup of 4 waves per (row, head, chunk) with the fragment images of every pass in LDS
        p->kind = multi ? ATT_X_MP : ATT_X;
        p->nw = multi ? 4 : 1;
        p->lds = multi ? xattn_mp_lds_bytes(p->nkf, d.npass) : 0;
        p->block = dim3(256);
    } else if (dtype == FFN_BF16 && pp) {
        p->kind = ATT_PP;
        p->lds = attn_pp_lds_bytes();
    } else {
        p->kind = ATT_KERNEL;
        p->f32 = dtype != FFN_BF16;
        p->masks |= p->f32;                                     // (one fp32 instantiation, with key masks)
        p->tile = attn_tile(p->f32, d.D);
        p->lds = attn_kernel_lds(p->f32 ? 4 : 2, p->tile.dp, p->tile.qf, p->tile.kt);
        // 1-D grid, decoded in the kernel through xcd_remap: the query blocks of one (row, head) run on ONE XCD, whose 4 MiB L2 then
        // serves that head's K / V^T (1 MiB at S = 4096) to all of them (measured before: 721 MB fetched for 126 MB of operands)
        p->grid = dim3(((d.S + 64 * p->tile.qf - 1) / (64 * p->tile.qf)) * d.heads * d.Bo);
        p->block = dim3(256);
    }
    REQUIRE(!d.kv_pair || p->kind == ATT_X3W, "attn: kv_pair is for launches that run attn_x3w_kernel (FFN_BF16X3, D = 64, Sk %% 64 == 0, S >= 128, "
                                              "no uniform-softmax entry, not the short-key kernel)");
    if (p->kind == ATT_KERNEL && d.D > 160) return fail(FFN_ENOSYS, "attn: head dim %d not supported (max 160; use the GEMM path)", d.D);
    return FFN_OK;
}
// the xattn kernels' work split over (row, head) pairs: wpp workgroups (xattn_kernel: waves) per pair, bpw 32-query blocks per wave, the chip's
// 8 waves per CU filled once
static dim3 xattn_grid(const ffn_attn_desc& d, int nw, int* wpp, int* bpw) {
    const int pairs = d.Bo * d.heads, nblk = (d.S + 31) / 32;
    int w = (8 * device_cus()) / pairs / nw;
    if (w < 1) w = 1;
    if (w > (nblk + nw - 1) / nw) w = (nblk + nw - 1) / nw;
    *bpw = (nblk + nw * w - 1) / (nw * w);
    *wpp = (nblk + nw * *bpw - 1) / (nw * *bpw);
    return dim3(nw == 1 ? (pairs * *wpp + 3) / 4 : pairs * *wpp);
}
template <typename K, typename... A>
static int attn_launch(const AttnPlan& p, K kern, hipStream_t s, A... args) {
    if (int rc = set_lds(kern, p.lds)) return rc;       // memoised under a mutex: safe from several host threads
    LAUNCH(kern, p.grid, p.block, p.lds, s, args...);
    return check_launch("attn");
}

extern "C" int ffn_attn_presplit(void* stream, const float* k, const float* vt, void* k_pair, void* vt_pair, int rows, int Sk, int heads, int ldk, int ldvt) {
    REQUIRE(k && vt && k_pair && vt_pair && aligned16(k) && aligned16(vt) && aligned16(k_pair) && aligned16(vt_pair), "attn_presplit: null / unaligned pointer");
    REQUIRE(rows > 0 && heads > 0 && Sk > 0 && Sk % 64 == 0 && ldk >= heads * 64 && ldk % 4 == 0 && ldvt >= Sk && ldvt % 4 == 0,
            "attn_presplit: rows=%d Sk=%d heads=%d ldk=%d ldvt=%d (head dim 64, Sk %% 64 == 0)", rows, Sk, heads, ldk, ldvt);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long nk = (long)rows * Sk * heads * 8, nv = (long)rows * heads * 64 * (Sk / 64) * 8;
    LAUNCH(attn_presplit_k_kernel, dim3(grid_for(nk)), dim3(256), 0, s, k, (bf16*)k_pair, nk, heads, ldk);
    LAUNCH(attn_presplit_vt_kernel, dim3(grid_for(nv)), dim3(256), 0, s, vt, (bf16*)vt_pair, nv, Sk / 64, ldvt);
    return check_launch("attn_presplit");
}
extern "C" int ffn_attn_kernel_name(int dtype, const ffn_attn_desc* d, char* buf, int len) {
    REQUIRE(d && buf && len > 0, "attn_kernel_name: null argument");
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16 || dtype == FFN_BF16X3, "attn_kernel_name: bad dtype %d", dtype);
    AttnPlan p;
    if (int rc = attn_plan(dtype, *d, &p)) return rc;
    const char* m = p.masks ? "true" : "false";
    switch (p.kind) {
    case ATT_KERNEL: snprintf(buf, len, "void attn_kernel<%s, %d, %d, %d, %d, %s>(ffn_attn_desc)", p.f32 ? "float" : "bf16", p.tile.dp, p.tile.qf, p.tile.kt, p.tile.occ, m); break;
    case ATT_PP: snprintf(buf, len, "void attn_pp_kernel<%s>(ffn_attn_desc)", m); break;
    case ATT_X: snprintf(buf, len, "void xattn_kernel<%d>(ffn_attn_desc, int, int)", p.nkf); break;
    case ATT_X_MP: snprintf(buf, len, "void xattn_mp_kernel<%d>(ffn_attn_desc, int, int)", p.nkf); break;
    case ATT_X3: snprintf(buf, len, "void attn_x3_kernel<%s>(ffn_attn_desc)", m); break;
    case ATT_X3P: snprintf(buf, len, "void attn_x3p_kernel<%s>(ffn_attn_desc)", m); break;
    case ATT_X3W: snprintf(buf, len, "void attn_x3w_kernel<%s>(ffn_attn_desc)", m); break;
    case ATT_XX3: snprintf(buf, len, "void xattn_x3_kernel<%d, %d>(ffn_attn_desc, int, int)", p.nkf, p.nw); break;
    case ATT_CAUSAL_K: snprintf(buf, len, "void attn_causal_kernel<%s, %s>(ffn_attn_desc)", dtype == FFN_BF16 ? "bf16" : "float", dtype == FFN_BF16X3 ? "true" : "false"); break;
    }
    return FFN_OK;
}
extern "C" int ffn_attn(void* stream, int dtype, const ffn_attn_desc* d) {
    REQUIRE(d, "attn: null descriptor");
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16 || dtype == FFN_BF16X3, "attn: bad dtype %d", dtype);
    const int epc = dtype == FFN_BF16 ? 8 : 4;
    REQUIRE(d->q && d->k && d->vt && d->out, "attn: null q/k/vt/out");
    REQUIRE(aligned16(d->q) && aligned16(d->k) && aligned16(d->vt) && aligned16(d->out), "attn: pointers must be 16-byte aligned");
    REQUIRE(d->Bo > 0 && d->Bo <= FFN_ATT_MAXB, "attn: Bo=%d out of range (max %d)", d->Bo, FFN_ATT_MAXB);
    REQUIRE(d->npass > 0 && d->npass <= FFN_ATT_MAXP, "attn: npass=%d out of range (max %d)", d->npass, FFN_ATT_MAXP);
    REQUIRE(d->S > 0 && d->Sk > 0 && d->heads > 0 && d->D > 0, "attn: empty problem");
    REQUIRE(d->D % epc == 0, "attn: D=%d must be a multiple of %d", d->D, epc);
    REQUIRE(d->ldq % epc == 0 && d->ldk % epc == 0 && d->ldvt % epc == 0 && d->ldo % 4 == 0, "attn: leading dims must be chunk aligned");
    REQUIRE(d->ldvt >= d->Sk, "attn: ldvt=%d < Sk=%d", d->ldvt, d->Sk);
    if (d->out_pair) {
        REQUIRE(dtype == FFN_BF16X3 && d->D <= 64 && d->ldo % 16 == 0 && d->ldo / 2 >= d->heads * d->D, "attn: pair output needs FFN_BF16X3, D <= 64, ldo %% 16 == 0");
        // the cross-attention kernel places pair columns by heads * D, the others by ldo / 2: the two agree in these cases only
        REQUIRE(d->ldo / 2 == d->heads * d->D || ((d->ldo / 2) % 32 == 0 && (d->heads * d->D) % 32 == 0), "attn: pair output into a wider row needs 32-column blocks (ldo=%d, heads*D=%d)", d->ldo, d->heads * d->D);
    }
    AttnPlan p;
    if (int rc = attn_plan(dtype, *d, &p)) return rc;
    if (d->kv_pair) {
        long maxkv = 0;
        for (int pi = 0; pi < d->npass; ++pi)
            for (int b = 0; b < d->Bo; ++b) maxkv = d->e[pi * FFN_ATT_MAXB + b].kv_row > maxkv ? d->e[pi * FFN_ATT_MAXB + b].kv_row : maxkv;
        REQUIRE(d->ldk >= d->heads * 64 && d->ldk % 64 == 0 && d->ldvt >= d->Sk && d->ldvt % 64 == 0,
                "attn: pre-split images need ldk >= heads * 64, ldvt >= Sk, both %% 64 == 0 (ldk=%d, ldvt=%d)", d->ldk, d->ldvt);
        REQUIRE((maxkv + 1) * d->Sk * (long)d->ldk * 4 < (1l << 31) - 65536 && (maxkv + 1) * d->heads * 64 * (long)d->ldvt * 4 < (1l << 31) - 65536,
                "attn: pre-split K / V^T images beyond 2 GiB (32-bit byte offsets)");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int wpp = 0, bpw = 0;
    if (p.kind == ATT_X || p.kind == ATT_X_MP || p.kind == ATT_XX3) p.grid = xattn_grid(*d, p.nw, &wpp, &bpw);
    switch (p.kind) {
    case ATT_KERNEL:
        if (p.f32) {
            switch (p.tile.dp) {
            case 48: return attn_launch(p, attn_kernel<float, 48, 2, 64, 1, true>, s, *d);
            case 64: return attn_launch(p, attn_kernel<float, 64, 2, 64, 1, true>, s, *d);
            case 80: return attn_launch(p, attn_kernel<float, 80, 2, 64, 1, true>, s, *d);
            default: return attn_launch(p, attn_kernel<float, 160, 1, 32, 1, true>, s, *d);
            }
        }
        switch (p.tile.dp) {
        case 64: return p.masks ? attn_launch(p, attn_kernel<bf16, 64, 2, 64, 2, true>, s, *d) : attn_launch(p, attn_kernel<bf16, 64, 2, 64, 2, false>, s, *d);
        case 96: return p.masks ? attn_launch(p, attn_kernel<bf16, 96, 2, 64, 1, true>, s, *d) : attn_launch(p, attn_kernel<bf16, 96, 2, 64, 1, false>, s, *d);
        default: return p.masks ? attn_launch(p, attn_kernel<bf16, 160, 1, 64, 1, true>, s, *d) : attn_launch(p, attn_kernel<bf16, 160, 1, 64, 1, false>, s, *d);
        }
    case ATT_PP: return p.masks ? attn_launch(p, attn_pp_kernel<true>, s, *d) : attn_launch(p, attn_pp_kernel<false>, s, *d);
    case ATT_X:
        return p.nkf == 2 ? attn_launch(p, xattn_kernel<2>, s, *d, wpp, bpw)
             : p.nkf == 5 ? attn_launch(p, xattn_kernel<5>, s, *d, wpp, bpw) : attn_launch(p, xattn_kernel<6>, s, *d, wpp, bpw);
    case ATT_X_MP:
        return p.nkf == 2 ? attn_launch(p, xattn_mp_kernel<2>, s, *d, wpp, bpw)
             : p.nkf == 5 ? attn_launch(p, xattn_mp_kernel<5>, s, *d, wpp, bpw) : attn_launch(p, xattn_mp_kernel<6>, s, *d, wpp, bpw);
    case ATT_X3: return p.masks ? attn_launch(p, attn_x3_kernel<true>, s, *d) : attn_launch(p, attn_x3_kernel<false>, s, *d);
    case ATT_X3P: return p.masks ? attn_launch(p, attn_x3p_kernel<true>, s, *d) : attn_launch(p, attn_x3p_kernel<false>, s, *d);
    case ATT_X3W: return attn_launch(p, fx3w_kernel(p.masks), s, *d);
    case ATT_CAUSAL_K: return attn_launch(p, fcausal_kernel(dtype), s, *d);
    case ATT_XX3:
        if (p.nw == 8)
            return p.nkf == 2 ? attn_launch(p, xattn_x3_kernel<2, 8>, s, *d, wpp, bpw)
                 : p.nkf == 5 ? attn_launch(p, xattn_x3_kernel<5, 8>, s, *d, wpp, bpw) : attn_launch(p, xattn_x3_kernel<6, 8>, s, *d, wpp, bpw);
        return p.nkf == 2 ? attn_launch(p, xattn_x3_kernel<2, 4>, s, *d, wpp, bpw)
             : p.nkf == 5 ? attn_launch(p, xattn_x3_kernel<5, 4>, s, *d, wpp, bpw) : attn_launch(p, xattn_x3_kernel<6, 4>, s, *d, wpp, bpw);
    }
    return fail(FFN_EINVAL, "attn: no kernel planned");
}
