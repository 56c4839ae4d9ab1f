// The implicit-GEMM entries of libfreefine_hip.so (ffn_igemm*): the tile rules, the configurations and their first-use tuner, the tune table, the one
// plan of which kernel runs (igemm_plan) and the launches (kernels: igemm.h, igemm_p8.h).  Host-side launch glue only, on the caller's stream.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "capi_common.h"
#include "igemm.h"
#include "igemm_p8.h"

static bool can_split(const ffn_igemm_desc& d) {
    return d.ws && d.splitk != 1 && !(d.flags & (FFN_IG_GEGLU | FFN_IG_OUT_TRANSPOSED | FFN_IG_OUT_KV64));
}
// the rule-based tile + number of K slices.  Without split-K small-M problems take small tiles to fill the chip (256 CUs, 2 workgroups/CU);
// with it they keep the 128x128 tile (operand reuse) and the K loop is cut so that ~2 workgroups per CU exist.
static void igemm_rule_for(int dtype, const ffn_igemm_desc& d, int* bm, int* bn, int* splitk) {
    const long t128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
    const long t12864 = (long)((d.M + 127) / 128) * ((d.N + 63) / 64);
    *splitk = 1;
    if (!d.conv && !(d.flags & FFN_IG_GEGLU) && d.M >= 128 && (!can_split(d) || t12864 >= 128)) {
        *bm = 128; *bn = 64;      // dense Linear layers (short K, memory/latency bound): measured 5-25% faster than 128x128
    } else if (d.N > 64 && (t128 >= 256 || (can_split(d) && d.M > 512 && d.N >= 128))) {
        *bm = 128; *bn = 128;     // measured (tools/bench_kernels.py): from M = 1024 up, 128x128 + split-K beats 128x64 without it
    } else if (t12864 >= 256 || d.M >= 4096 || (can_split(d) && d.M >= 96 && d.N >= 64)) {
        *bm = 128; *bn = 64;      // M <= 512: half the K slices (and slab traffic) of 128x128 for the same number of workgroups
    } else { *bm = 64; *bn = 64; }
    if (can_split(d)) {
        const int kstage = dtype == FFN_F32 ? 32 : 64;
        const int nk = (d.K + kstage - 1) / kstage;
        const long tiles = (long)((d.M + *bm - 1) / *bm) * ((d.N + *bn - 1) / *bn);
        int s = d.splitk > 1 ? d.splitk : (tiles >= 224 ? 1 : (int)((448 + tiles - 1) / tiles));
        if (d.splitk <= 1 && s > nk / 6) s = nk / 6;            // keep >= 6 K stages per slice
        const long per = (long)d.M * d.N * 4;
        if ((long)s * per > d.ws_bytes) s = (int)(d.ws_bytes / per);
        if (s > nk) s = nk;
        if (s < 1) s = 1;
        *splitk = s;
    }
}

// ---- bf16 tile configurations and first-use autotuning ------------------------------------------------------------------
// The SD shapes span M = 4 ... 4M rows and N = 4 ... 10240 columns; which (tile, K-split) wins depends on how the tile count
// quantises over 256 CUs as much as on the tile's own efficiency (measured, tools/bench_kernels.py: at M = 98304 the 128x320 tile
// runs the N = 320 convs at 850-1000 TFLOP/s where 128x128 -- 17% of its third column tile wasted -- gives 690-760; 256x256
// reaches 1190 on N = 1280 but loses 20% on N = 640).  So the first time a problem shape is seen outside stream capture, the
// few plausible configurations are timed on the caller's stream with the caller's buffers and the winner is cached.
enum { CFG_64x64, CFG_128x64, CFG_128x128_8, CFG_128x128_16, CFG_256x128, CFG_256x256, CFG_128x320, CFG_128x160, CFG_192x320, CFG_H_128x320, CFG_H_256x128, CFG_H_256x256, CFG_H_128x128, CFG_PP_256x320, CFG_PP_256x256, CFG_PP_192x320, CFG_PP_192x256, CFG_PP_256x128, CFG_COUNT };
struct IgCfgInfo { int bm, bn, nwm, nwn; };
static const IgCfgInfo kCfg[CFG_COUNT] = {{64, 64, 2, 2}, {128, 64, 4, 2}, {128, 128, 2, 4}, {128, 128, 4, 4},
                                          {256, 128, 4, 4}, {256, 256, 4, 4}, {128, 320, 4, 4}, {128, 160, 4, 2}, {192, 320, 3, 4},
                                          {128, 320, 4, 4}, {256, 128, 4, 4}, {256, 256, 4, 4}, {128, 128, 4, 4},    // halo kernel (3x3 stride-1 convs)
                                          {256, 320, 2, 4}, {256, 256, 2, 4}, {192, 320, 2, 4}, {192, 256, 2, 4},      // ping-pong kernel (igemm_p8.h)
                                          {256, 128, 2, 4}};    // its 128-column tile: split-bf16 3x3 convolutions to N % 128 == 0 channels (the VAE's 128-channel layers)
struct IgChoice { int cfg, splitk; };
struct TunedEntry { IgChoice ch; bool validated; };   // imported entries (file / another rank) are checked against the problem at first use

static bool is_halo_cfg(int cfg) { return cfg == CFG_H_128x320 || cfg == CFG_H_256x128 || cfg == CFG_H_256x256 || cfg == CFG_H_128x128; }
static bool is_pp_cfg(int cfg) { return cfg >= CFG_PP_256x320 && cfg <= CFG_PP_256x128; }
// whether the ping-pong kernel (igemm_p8.h) handles this problem on a bm x bn tile: its restrictions are listed in that header
static bool pp_ok(const ffn_igemm_desc& d, int bm, int bn, int splitk = 1) {
    const long lim = (1l << 31) - 4096;
    // K tiles of the kernel: 64 bf16 elements; split-bf16 (d.K = the virtual 3 K): one 128-byte block [hi(32) | lo(32)] = 32 real elements
    const int nkt = d.x3 ? d.K / 96 : d.K / 64;
    // the 128-column tile exists for unsplit split-bf16 3x3 convolutions with a plain / residual epilogue only
    // (and only where neither wider tile divides N: the UNet's N = 640 / 1280 convolutions keep their 320- / 256-column tiles, no extra tuner candidate there)
    if (bn == 128 && (bm != 256 || !d.x3 || d.conv != 1 || splitk > 1 || d.N % 256 == 0 || d.N % 320 == 0 || (d.flags & (FFN_IG_GEGLU | FFN_IG_OUT_PAIR | FFN_IG_OUT_KV64 | FFN_IG_OUT_TRANSPOSED)))) return false;
    if (d.x3) {
        if (d.x3 != 2 || d.K % 96 != 0 || d.a_lo != 32) return false;             // blocked operands only
    } else if (d.K % 64 != 0) return false;
    if (nkt < 2 || d.N % bn != 0 || d.M < bm) return false;
    const int osz = d.x3 ? 4 : 2;                                  // bytes per output / residual element
    if (splitk > 1) {       // split-K: raw fp32 slabs + igemm_splitk_reduce_kernel (which applies every plain epilogue option); slices of whole K tiles
        if (!can_split(d) || nkt % splitk != 0 || nkt / splitk < 2 || (long)splitk * d.M * d.N * 4 > d.ws_bytes || (long)splitk * d.M * d.N * 4 >= lim) return false;
    } else {
        // GELU / RELU: applied by the plain bf16 epilogue, whose accumulators start at the bias -- not beside a residual (it starts there too)
        const int act_ok = (!d.residual && !d.x3 && !d.f8 && !(d.flags & FFN_IG_GEGLU)) ? (FFN_IG_OUT_GELU | FFN_IG_OUT_RELU) : 0;
        if ((d.alpha != 1.0f && !d.f8) || (d.flags & ~(FFN_IG_GEGLU | act_ok | (d.x3 ? (FFN_IG_OUT_F32 | FFN_IG_OUT_PAIR | FFN_IG_OUT_KV64) : 0)))) return false;
        if (d.f8 && (!d.conv || (d.flags & FFN_IG_GEGLU))) return false;
        if (d.x3 && (d.flags & FFN_IG_GEGLU) && !(d.flags & FFN_IG_OUT_PAIR)) return false;      // the split-bf16 GEGLU tile writes the pair form only
        if ((d.flags & FFN_IG_OUT_PAIR) && !(d.flags & FFN_IG_GEGLU) && (d.N % 32 != 0 || (d.ldo / 2) % 32 != 0 || (d.flags & FFN_IG_OUT_TRANSPOSED))) return false;      // plain tile: blocked pair rows only
        if ((d.flags & FFN_IG_GEGLU) && bn != 256) return false;
        if (d.rowbias && d.rows_per_batch < 128) return false;      // a wave's rows (bm / 2) may straddle two images, not three
    }
    long a_bytes;
    if (d.conv) {
        const int pix = d.x3 ? d.lda : d.Cin;                      // elements per input pixel
        const int cpt = d.x3 ? d.Cin / 32 : d.Cin / 64;            // K tiles per tap
        if (d.Cin % (d.x3 ? 32 : 64) != 0 || d.K != (d.conv == 2 ? 4 : 9) * (d.x3 ? 3 : 1) * d.Cin) return false;
        if (d.x3 && d.lda != 2 * d.Cin) return false;
        if (d.conv == 2 && (d.f8 || d.stride != 1 || d.upsample)) return false;
        if ((long)cpt * 9 * cpt >= 65536) return false;            // exactness range of the tap reciprocal
        a_bytes = (long)(d.M / (d.Hout * d.Wout)) * d.Hin * d.Win * pix * 2;
        if (2 * d.Hin + 2 >= 32768 || 2 * d.Win + 2 >= 32768) return false;
        if (a_bytes + 256l * pix * 2 >= lim) return false;
    } else {
        a_bytes = (long)d.M * d.lda * 2;
        if (a_bytes + 256l * d.lda * 2 >= lim) return false;
    }
    if ((long)d.N * d.Kpad * 2 >= lim || (long)(d.M + 256) * d.ldo * ((d.flags & FFN_IG_OUT_PAIR) ? 2 : osz) >= lim) return false;
    if (d.residual && (long)(d.M + 256) * d.ldr * osz >= lim) return false;
    return true;
}
// LDS bytes of ONE halo buffer of the halo conv kernel for tile height bm, or 0 if the problem does not fit the kernel: 3x3,
// stride 1, pad 1, no upsample, whole 64-channel chunks, and a tile = whole image rows (W <= bm) or a piece of one row
static int halo_bytes_for(const ffn_igemm_desc& d, int bm) {
    if (!d.conv || d.stride != 1 || d.upsample || d.pad != 1 || d.Hin != d.Hout || d.Win != d.Wout) return 0;
    if (d.Cin % 64 != 0 || d.Cin > 30000 || d.K != 9 * d.Cin || d.M % bm != 0) return 0;
    const int H = d.Hin, W = d.Win;
    int tw, tr;
    if (W <= bm) {
        if (bm % W != 0 || (H * W) % bm != 0) return 0;
        tw = W; tr = bm / W;
    } else {
        if (W % bm != 0) return 0;
        tw = bm; tr = 1;
    }
    const int nq = ((tr + 2) * (tw + 2) + 7) / 8;
    if (nq > 4 * 16) return 0;                      // 4 halo wave-instructions per wave, 16 waves
    return nq * 8 * 128;
}
// X3 (split-bf16, FFN_BF16X3) problems run the generic 64x64 / 128x64 / 128x128 tiles (recomputing loader) and the ping-pong tiles
static bool x3_cfg(int cfg) { return cfg == CFG_64x64 || cfg == CFG_128x64 || cfg == CFG_128x128_8 || is_pp_cfg(cfg); }
// the library's private view of a split-bf16 problem: the kernels and the tile / split-K logic see the VIRTUAL contraction 3K
static ffn_igemm_desc x3_view(const ffn_igemm_desc& d) {
    ffn_igemm_desc v = d;
    v.x3 = d.x3 == 2 ? 2 : 1;          // operand layout: 1 = planes, 2 = 128-byte blocks [hi(32) | lo(32)] (include/freefine_hip.h)
    v.f8 = 0;
    v.K = 3 * d.K;
    v.flags |= FFN_IG_OUT_F32;
    return v;
}
// fp8 problems: the kernels and every tile / split-K decision see a bf16-SHAPED view (two e4m3 bytes = one "element")
static ffn_igemm_desc f8_view(const ffn_igemm_desc& d) {
    ffn_igemm_desc v = d;
    v.f8 = 1;
    v.x3 = 0;
    v.K = d.K / 2;
    v.Cin = d.Cin / 2;
    v.Kpad = d.Kpad / 2;
    v.lda = d.lda / 2;
    return v;
}
static ffn_igemm_desc igemm_view(int dtype, const ffn_igemm_desc& d) {
    if (dtype == FFN_BF16X3) return x3_view(d);
    if (dtype == FFN_FP8) return f8_view(d);
    ffn_igemm_desc v = d;
    v.x3 = v.f8 = 0;
    return v;
}
// the ping-pong tile height for bn-column tiles: of `heights`, among those the kernel takes (transposed form: M >= h is all that is left to ask) and
// whose tiles fill at least min_fill4 quarters of the chip, the one whose tile count wastes the least of the last round of workgroups; 0 = none
static int pp_tile_height(const ffn_igemm_desc& d, int bn, std::initializer_list<int> heights, int min_fill4, bool trans = false) {
    long best = -1;
    int bh = 0;
    for (int h : heights) {
        if (trans ? d.M < h : !pp_ok(d, h, bn)) continue;
        const long tiles = (long)((d.M + h - 1) / h) * (d.N / bn);
        if (tiles * 4 < (long)device_cus() * min_fill4) continue;
        const long cost = ((tiles + device_cus() - 1) / device_cus()) * h;
        if (best < 0 || cost < best) { best = cost; bh = h; }
    }
    return bh;
}
static int pp_cfg(int bm, int bn) {
    for (int cfg = CFG_PP_256x320; cfg <= CFG_PP_256x128; ++cfg)
        if (kCfg[cfg].bm == bm && kCfg[cfg].bn == bn) return cfg;
    return -1;
}
// 2x2 sub-pixel convolutions exist in the ping-pong kernel only: the first of its tiles that applies, wide and tall first
static bool conv2_tile(const ffn_igemm_desc& d, int* bm, int* bn) {
    for (int n : {320, 256})
        for (int h : {256, 192})
            if (pp_tile_height(d, n, {h}, 0)) { *bm = h; *bn = n; return true; }
    return false;
}
// transposed-output (V^T) launches on the ping-pong kernel: deterministic tile choice (no tuning)
static bool pp_trans_tile(const ffn_igemm_desc& d, int* bm, int* bn) {
    const long lim = (1l << 31) - 4096;
    *bn = d.N % 320 == 0 ? 320 : (d.N % 256 == 0 ? 256 : 0);
    if (!*bn || d.alpha != 1.0f || d.rows_per_batch % 16 != 0 || d.M % 4 != 0) return false;
    if (d.x3) {         // split-bf16: blocked operands, K tiles of 32 real elements (d.K = the virtual 3 K), fp32 V^T
        if (d.x3 != 2 || d.K % 96 != 0 || d.K < 192 || d.a_lo != 32) return false;
    } else if (d.K % 64 != 0 || d.K < 128) return false;
    if ((long)(d.M + 256) * d.lda * 2 >= lim || (long)d.N * d.Kpad * 2 >= lim) return false;
    if ((long)((d.M + d.rows_per_batch - 1) / d.rows_per_batch) * d.N * d.ldo * (d.x3 ? 4 : 2) >= lim) return false;
    return (*bm = pp_tile_height(d, *bn, {256, 192}, 0, true)) != 0;
}
// igemm_rule_for as a configuration.  Waves per workgroup, measured on MI355X (tools/bench_kernels.py): occupancy beats prefetch depth for these
// compiler-scheduled loops -- 2 workgroups/CU with a 2-deep ring win over 1 workgroup/CU with a 3-4 deep ring by ~35%; on the 128x128 tile 8 waves
// (4 waves/SIMD) beat 4 waves by 5-30%, and 16 waves win once the K loop is short (split-bf16 / fp8: no 16-wave instantiation)
static IgChoice rule_choice(int dtype, const ffn_igemm_desc& d) {
    int bm, bn, sk;
    igemm_rule_for(dtype, d, &bm, &bn, &sk);
    const int kstage = dtype == FFN_F32 ? 32 : 64;
    const int nk = ((d.K + kstage - 1) / kstage + sk - 1) / sk;    // K stages per workgroup
    int cfg = CFG_64x64;
    if (bm == 128 && bn == 64) cfg = CFG_128x64;
    if (bm == 128 && bn == 128) cfg = (!d.conv && nk <= 24 && !d.x3 && !d.f8) ? CFG_128x128_16 : CFG_128x128_8;
    return IgChoice{cfg, sk};
}
// the deterministic rule-based choice of the tuned family (bf16 / split-bf16 / fp8 problems, row-major output)
static IgChoice heuristic_choice(const ffn_igemm_desc& d) {
    int bm, bn;
    if (d.conv == 2 && conv2_tile(d, &bm, &bn)) return IgChoice{pp_cfg(bm, bn), 1};      // (igemm_validate has checked that a tile applies)
    // the ping-pong tile first, where its unsplit form applies and its tiles fill at least 3/4 of the chip.  Without this, every launch that
    // cannot be tuned (FFN_IGEMM_TUNE=0, stream capture before a shape was seen, out aliasing residual) fell back to the 2-stage kernels
    if (d.splitk <= 1) {
        for (int n : {320, 256})
            if ((bm = pp_tile_height(d, n, {256, 192}, 3))) return IgChoice{pp_cfg(bm, n), 1};
        if (pp_tile_height(d, 128, {256}, 3)) return IgChoice{CFG_PP_256x128, 1};
    }
    return rule_choice(FFN_BF16, d);
}

struct TuneKey {
    int M, N, K, conv, Cin, Hin, Win, stride, upsample, flags, lda, splitk, ptrs, wslabs, rpb, alpha1, ldo, pad, Hout, Wout, Kpad, ldr, dtype;
    bool operator==(const TuneKey& o) const { return memcmp(this, &o, sizeof(TuneKey)) == 0; }
};
struct TuneKeyHash {
    size_t operator()(const TuneKey& k) const {
        const int* p = reinterpret_cast<const int*>(&k);
        size_t h = 1469598103934665603ull;
        for (size_t i = 0; i < sizeof(TuneKey) / sizeof(int); ++i) h = (h ^ (size_t)(unsigned)p[i]) * 1099511628211ull;
        return h;
    }
};
static TuneKey tune_key(const ffn_igemm_desc& d) {
    TuneKey k;
    memset(&k, 0, sizeof(k));
    k.M = d.M; k.N = d.N; k.K = d.K; k.conv = d.conv; k.flags = d.flags; k.lda = d.lda; k.splitk = d.splitk;
    if (d.conv) { k.Cin = d.Cin; k.Hin = d.Hin; k.Win = d.Win; k.stride = d.stride; k.upsample = d.upsample; k.pad = d.pad; k.Hout = d.Hout; k.Wout = d.Wout; }
    k.Kpad = d.Kpad;
    k.ldr = d.residual ? d.ldr : 0;
    k.dtype = d.x3 ? (FFN_BF16X3 | (d.x3 << 8)) : (d.f8 ? FFN_FP8 : FFN_BF16);
    k.ptrs = (d.bias ? 1 : 0) | (d.rowbias ? 2 : 0) | (d.residual ? 4 : 0) | (d.ws && d.ws_bytes > 0 ? 8 : 0);
    const long per = (long)d.M * d.N * 4;
    k.wslabs = d.ws ? (int)(d.ws_bytes / per > 1024 ? 1024 : d.ws_bytes / per) : 0;      // how many split-K slabs the workspace holds
    k.rpb = d.rows_per_batch;
    k.alpha1 = d.alpha == 1.0f;
    k.ldo = d.ldo;
    return k;
}
static std::mutex g_tune_mu;
static std::unordered_map<TuneKey, TunedEntry, TuneKeyHash> g_tuned;
static int g_tune_runtime = 1;      // ffn_igemm_tune_enable(0): no more timing-based tuning in this process (after a table sync)
static bool tune_enabled() {
    static const bool on = [] { const char* e = getenv("FFN_IGEMM_TUNE"); return !(e && atoi(e) == 0); }();
    return on && g_tune_runtime;
}
static constexpr int kPpSplitBelow = 160;      // ping-pong configurations: unsplit tile counts below this get split-K candidates
static int candidates_for(const ffn_igemm_desc& d, IgChoice* out, int cap) {
    int n = 0;
    const IgChoice h = heuristic_choice(d);
    out[n++] = h;
    const int nk = (d.K + 63) / 64;
    const long per = (long)d.M * d.N * 4;
    for (int cfg = 0; cfg < CFG_COUNT; ++cfg) {
        const IgCfgInfo& c = kCfg[cfg];
        if ((d.x3 || d.f8) && !x3_cfg(cfg)) continue;
        if (d.conv == 2 && !is_pp_cfg(cfg)) continue;
        if ((cfg == CFG_128x320 || cfg == CFG_128x160 || cfg == CFG_192x320) && (d.flags & FFN_IG_GEGLU)) continue;   // odd number of column blocks per wave
        if (is_halo_cfg(cfg)) {
            const int hb = halo_bytes_for(d, c.bm);
            if (hb <= 0 || d.splitk > 1 || 2 * hb + 2 * c.bn * 128 > 160 * 1024) continue;
            if ((cfg == CFG_H_128x320) && (d.flags & FFN_IG_GEGLU)) continue;
        }
        const bool halo = is_halo_cfg(cfg) || is_pp_cfg(cfg);                      // no generic split-K variants
        if (is_pp_cfg(cfg)) {
            // ping-pong: unsplit where its epilogue applies; split-K (a divisor of the K-tile count, >= 2 K tiles per slice) where the
            // output tiles alone leave most of the chip idle
            const long pt = (long)((d.M + c.bm - 1) / c.bm) * (d.N / (c.bn > 0 ? c.bn : 1));
            if (d.splitk <= 1 && pp_ok(d, c.bm, c.bn) && n < cap) out[n++] = IgChoice{cfg, 1};
            if (cfg != CFG_PP_256x128 && d.splitk != 1 && pt > 0 && pt < kPpSplitBelow && d.N % c.bn == 0) {
                const int nkt = d.x3 ? d.K / 96 : d.K / 64;
                int added = 0;
                for (int sgo = (int)((384 + pt - 1) / pt); sgo >= 2 && added < 2; --sgo) {
                    if (d.splitk > 1 && sgo != d.splitk) continue;
                    if (nkt % sgo != 0 || nkt / sgo < 2 || !pp_ok(d, c.bm, c.bn, sgo)) continue;
                    if (n < cap) out[n++] = IgChoice{cfg, sgo};
                    ++added;
                }
            }
            continue;
        }
        if (c.bm > 64 && c.bm >= 2 * d.M) continue;                                // tile mostly empty
        if (c.bn > 64 && c.bn >= 2 * d.N) continue;
        if (cfg == CFG_64x64 && (long)d.M * d.N > (1l << 22)) continue;
        const long tiles = (long)((d.M + c.bm - 1) / c.bm) * ((d.N + c.bn - 1) / c.bn);
        int splits[3] = {1, 0, 0};
        if (d.splitk > 1) {              // caller-forced split: only where a split launch is legal and the workspace holds the slabs
            int sf = (can_split(d) && !halo) ? d.splitk : 1;
            if ((long)sf * per > d.ws_bytes) sf = (int)(d.ws_bytes / per);
            if (sf > nk) sf = nk;
            splits[0] = sf >= 2 ? sf : 1;
        } else if (can_split(d) && !halo) {
            for (int t = 0; t < 2; ++t) {
                int sgo = (int)(((t ? 512 : 256) + tiles / 2) / tiles);
                if (sgo > nk / 4) sgo = nk / 4;
                if ((long)sgo * per > d.ws_bytes) sgo = (int)(d.ws_bytes / per);
                if (sgo >= 2) splits[1 + t] = sgo;
            }
            if (splits[2] == splits[1]) splits[2] = 0;
        }
        for (int t = 0; t < 3 && n < cap; ++t) {
            if (!splits[t]) continue;
            bool dup = false;
            for (int j = 0; j < n; ++j) dup |= out[j].cfg == cfg && out[j].splitk == splits[t];
            if (!dup) out[n++] = IgChoice{cfg, splits[t]};
        }
    }
    return n;
}
static int g_force_cfg = -1;     // testing hook (ffn_igemm_force_config): run every bf16 problem on this configuration where it is valid
extern "C" int ffn_igemm_num_configs(void) { return CFG_COUNT; }
extern "C" int ffn_igemm_force_config(int cfg) {
    const int prev = g_force_cfg;
    g_force_cfg = (cfg >= 0 && cfg < CFG_COUNT) ? cfg : -1;
    return prev;
}
// the configuration of a tuned-family problem where no timing is needed to know it: the forced one (the first candidate on it, else -- not valid
// for this problem -- the rule's), then the table's.  false: neither (ffn_igemm tunes or takes heuristic_choice, ffn_igemm_kernel_name the latter)
static bool known_choice(const ffn_igemm_desc& d, IgChoice* ch) {
    IgChoice cand[40];
    if (g_force_cfg >= 0) {
        *ch = heuristic_choice(d);
        for (int i = candidates_for(d, cand, 40) - 1; i >= 0; --i)
            if (cand[i].cfg == g_force_cfg) *ch = cand[i];
        return true;
    }
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tuned.find(tune_key(d));
    if (it == g_tuned.end()) return false;
    if (!it->second.validated) {
        // an entry that came in as data (a tune file, another rank's table): launch it only if this build would have
        // offered exactly that (configuration, K split) for THIS problem -- workspace capacity, split legality, tile
        // applicability are all decided in candidates_for; anything else is dropped and the problem is tuned afresh
        const int nc = candidates_for(d, cand, 40);
        bool ok = false;
        for (int i = 0; i < nc; ++i) ok |= cand[i].cfg == it->second.ch.cfg && cand[i].splitk == it->second.ch.splitk;
        if (!ok) return g_tuned.erase(it), false;
        it->second.validated = true;
    }
    *ch = it->second.ch;
    return true;
}

enum IgKind { IG_RING, IG_HALO, IG_PP, IG_PP_TRANS };
struct IgemmPlan {
    IgKind kind;
    bool f32;                          // fp32 (else bf16: what split-bf16 and fp8 operands ride on, too) elements
    int bm, bn, amode, nwm, nwn;       // tile, AMODE_*, wave grid (IG_RING: the ring depth NS is 2)
    bool swap, fastk, x3, f8;
    bool res, geglu, split;            // IG_PP: the instantiation's epilogue form
    int splitk, halo_bytes, lds;
    bool reduce_f32;                   // splitk > 1: igemm_splitk_reduce_kernel<float> (else <bf16>) finishes
    dim3 grid, block;
};
// The one statement of which kernel ffn_igemm launches for a (validated, viewed: igemm_view) descriptor: igemm_run launches from it,
// ffn_igemm_kernel_name spells it.
//   The rule-based family (ch = nullptr): FFN_F32, and every transposed output (V^T for ffn_attn).  igemm_pp_kernel's transposed form where
//     pp_trans_tile finds a tile (bf16 / split-bf16 elements); else igemm_glds_kernel on rule_choice's tile, K split and waves (the split-bf16
//     V^T: 4 waves on every tile).
//   The tuned family (bf16 / split-bf16 / fp8 elements, row-major output): the configuration `ch` -- forced, from the table, timed or
//     heuristic_choice's -- on igemm_glds_kernel (walking its tiles from a co-resident grid), igemm_halo_kernel or igemm_pp_kernel.
// FFN_EINVAL: a configuration that does not apply to the problem (candidates_for offers none such).
static int igemm_plan(int dtype, const ffn_igemm_desc& d, const IgChoice* ch, IgemmPlan* p) {
    *p = IgemmPlan{};
    p->f32 = dtype == FFN_F32;
    p->x3 = d.x3 != 0;
    p->f8 = d.f8 != 0;
    p->amode = d.conv ? AMODE_CONV3 : AMODE_DENSE;
    p->swap = !(d.flags & FFN_IG_OUT_TRANSPOSED);
    p->reduce_f32 = p->f32 || p->x3;
    p->splitk = 1;
    p->block = dim3(512);
    const bool tuned = ch != nullptr;
    IgChoice rule;
    if (!tuned && !p->f32 && pp_trans_tile(d, &p->bm, &p->bn)) {
        p->kind = IG_PP_TRANS;
    } else {
        if (!tuned) ch = &(rule = rule_choice(p->f32 ? FFN_F32 : FFN_BF16, d));
        REQUIRE(ch->cfg >= 0 && ch->cfg < CFG_COUNT, "igemm: bad configuration %d", ch->cfg);
        REQUIRE(!(p->x3 || p->f8) || x3_cfg(ch->cfg), "igemm: configuration %d is not built for split-bf16 / fp8 problems", ch->cfg);
        const IgCfgInfo& c = kCfg[ch->cfg];
        p->kind = is_halo_cfg(ch->cfg) ? IG_HALO : (is_pp_cfg(ch->cfg) ? IG_PP : IG_RING);
        p->bm = c.bm; p->bn = c.bn; p->nwm = c.nwm; p->nwn = c.nwn;
        p->splitk = ch->splitk;
        p->block = dim3(64 * c.nwm * c.nwn);
        if (!tuned && p->x3) p->nwm = p->nwn = 2, p->block = dim3(256);
    }
    const int ntm = (d.M + p->bm - 1) / p->bm, ntn = (d.N + p->bn - 1) / p->bn;
    switch (p->kind) {
    case IG_RING: {
        // FASTK kernels (streaming loader) need every 128-byte K stage inside K / inside one conv tap
        // the streaming loader's zero-page pointers (N-tail columns, rows past M, conv padding) walk 128 B per K stage over the WHOLE K
        // range of the launch: K * 2 bytes must stay inside the 64 KiB zero page
        p->fastk = tuned && !p->x3 && !p->f8 && (d.conv ? d.Cin % 64 == 0 : d.K % 64 == 0) && (long)d.K * 2 + 256 <= (long)sizeof(g_zero_page);
        p->lds = 2 * (p->bm + p->bn) * 128;
        int gx = ntm * ntn;
        if (tuned || p->x3) {
            // these instantiations walk several output tiles per workgroup (igemm.h): launch only as many workgroups as are co-resident
            // (LDS / thread limits per CU) and let each stride over the tile list
            int per_cu = (160 * 1024) / p->lds;
            if (per_cu > 2048 / (int)p->block.x) per_cu = 2048 / (int)p->block.x;
            const int cap = (device_cus() * per_cu) / p->splitk;
            if (gx > cap && cap >= 8) gx = cap;
        }
        p->grid = dim3(gx, p->splitk);
        break;
    }
    case IG_HALO:
        p->halo_bytes = halo_bytes_for(d, p->bm);
        REQUIRE(p->halo_bytes > 0 && p->splitk == 1 && !p->x3 && !p->f8, "igemm: halo kernel not applicable");
        p->lds = 2 * p->halo_bytes + 2 * p->bn * 128;
        p->grid = dim3((d.M / p->bm) * ntn);
        break;
    case IG_PP:
        REQUIRE(pp_ok(d, p->bm, p->bn, p->splitk), "igemm: ping-pong kernel not applicable");
        p->split = p->splitk > 1;
        p->res = !p->split && d.residual;
        p->geglu = !p->split && !d.conv && (d.flags & FFN_IG_GEGLU);
        [[fallthrough]];
    case IG_PP_TRANS: {
        p->lds = 2 * (p->bm + p->bn) * 128 + 12288;
        const int nt = ntm * (d.N / p->bn) * p->splitk;
        p->grid = dim3(nt < device_cus() ? nt : device_cus());
        break;
    }
    }
    return FFN_OK;
}
template <typename K, typename... A>
static int igemm_launch(const IgemmPlan& p, K kern, hipStream_t s, A... args) {
    static const char* const what[] = {"igemm", "igemm(halo)", "igemm(ping-pong)", "igemm(ping-pong, transposed)"};
    if (int rc = set_lds(kern, p.lds)) return rc;
    LAUNCH(kern, p.grid, p.block, p.lds, s, args...);
    return check_launch(what[p.kind]);
}
// the instantiations of igemm_glds_kernel: the 4-wave tiles of the split-bf16 V^T; else the three tiles every element type has, the 16-wave
// 128x128 tile and -- bf16 operands, row-major output -- the wide tiles of the tuned family
template <typename T, int AMODE, bool SWAP, bool FASTK = false, bool X3 = false, bool F8 = false>
static int launch_ring(const IgemmPlan& p, hipStream_t s, const ffn_igemm_desc& d) {
#define FFN_RING(BM_, BN_, WM_, WN_) \
    if (p.bm == BM_ && p.bn == BN_ && p.nwm == WM_ && p.nwn == WN_) return igemm_launch(p, igemm_glds_kernel<T, BM_, BN_, AMODE, SWAP, 2, WM_, WN_, FASTK, X3, F8>, s, d)
    if constexpr (X3 && !SWAP) {
        FFN_RING(64, 64, 2, 2);
        FFN_RING(128, 64, 2, 2);
        FFN_RING(128, 128, 2, 2);
    } else {
        FFN_RING(64, 64, 2, 2);
        FFN_RING(128, 64, 4, 2);
        FFN_RING(128, 128, 2, 4);
        if constexpr (!X3 && !F8) FFN_RING(128, 128, 4, 4);
        if constexpr (sizeof(T) == 2 && SWAP && !X3 && !F8) {
            FFN_RING(256, 128, 4, 4);
            FFN_RING(256, 256, 4, 4);
            FFN_RING(128, 320, 4, 4);
            FFN_RING(128, 160, 4, 2);
            FFN_RING(192, 320, 3, 4);      // 12 waves: 168 registers per wave (spills at 16 waves x 128)
        }
    }
#undef FFN_RING
    return fail(FFN_EINVAL, "igemm: no %d x %d tile on %d x %d waves for this problem", p.bm, p.bn, p.nwm, p.nwn);
}
// the instantiations of igemm_pp_kernel: per tile the plain / residual / split-K forms; dense A also the transposed form and, 256 columns wide,
// GEGLU; the 256x128 tile for split-bf16 3x3 convolutions, plain / residual (pp_ok)
template <int AMODE, bool X3 = false, bool F8 = false>
static int launch_pp(const IgemmPlan& p, hipStream_t s, const ffn_igemm_desc& d) {
    const bool trans = p.kind == IG_PP_TRANS;
#define FFN_PP(BM_, BN_, RES_, GEGLU_, SPLIT_, TRANS_)                                                                       \
    if (p.bm == BM_ && p.bn == BN_ && p.res == RES_ && p.geglu == GEGLU_ && p.split == SPLIT_ && trans == TRANS_) \
        return igemm_launch(p, igemm_pp_kernel<BM_, BN_, AMODE, RES_, GEGLU_, SPLIT_, TRANS_, X3, F8>, s, d, p.splitk)
#define FFN_PP_TILE(BM_, BN_)                                                                   \
    FFN_PP(BM_, BN_, false, false, false, false);                                               \
    FFN_PP(BM_, BN_, true, false, false, false);                                                \
    FFN_PP(BM_, BN_, false, false, true, false);                                                \
    if constexpr (AMODE == AMODE_DENSE && !F8) {                                                \
        FFN_PP(BM_, BN_, false, false, false, true);                                            \
        if constexpr (BN_ == 256) FFN_PP(BM_, BN_, false, true, false, false);                  \
    }
    FFN_PP_TILE(256, 320)
    FFN_PP_TILE(256, 256)
    FFN_PP_TILE(192, 320)
    FFN_PP_TILE(192, 256)
    if constexpr (X3 && AMODE == AMODE_CONV3) {
        FFN_PP(256, 128, false, false, false, false);
        FFN_PP(256, 128, true, false, false, false);
    }
#undef FFN_PP_TILE
#undef FFN_PP
    return fail(FFN_EINVAL, "igemm: no %d x %d ping-pong tile of this form", p.bm, p.bn);
}
// plan and launch: the rule-based family (ch = nullptr) or configuration `ch` of the tuned family; the split-K reduce behind either
static int igemm_run(hipStream_t s, int dtype, const ffn_igemm_desc& d, const IgChoice* ch) {
    IgemmPlan p;
    int rc = igemm_plan(dtype, d, ch, &p);
    if (rc) return rc;
    const bool conv = p.amode == AMODE_CONV3;
    switch (p.kind) {
    case IG_RING:
        if (p.f32) rc = conv ? launch_ring<float, AMODE_CONV3, true>(p, s, d) : (p.swap ? launch_ring<float, AMODE_DENSE, true>(p, s, d) : launch_ring<float, AMODE_DENSE, false>(p, s, d));
        else if (!p.swap) rc = p.x3 ? launch_ring<bf16, AMODE_DENSE, false, false, true>(p, s, d) : launch_ring<bf16, AMODE_DENSE, false>(p, s, d);
        else if (p.x3) rc = conv ? launch_ring<bf16, AMODE_CONV3, true, false, true>(p, s, d) : launch_ring<bf16, AMODE_DENSE, true, false, true>(p, s, d);
        else if (p.f8) rc = launch_ring<bf16, AMODE_CONV3, true, false, false, true>(p, s, d);
        else if (p.fastk) rc = conv ? launch_ring<bf16, AMODE_CONV3, true, true>(p, s, d) : launch_ring<bf16, AMODE_DENSE, true, true>(p, s, d);
        else rc = conv ? launch_ring<bf16, AMODE_CONV3, true>(p, s, d) : launch_ring<bf16, AMODE_DENSE, true>(p, s, d);
        break;
    case IG_HALO:
#define FFN_HALO(BM_, BN_) \
    if (p.bm == BM_ && p.bn == BN_) rc = igemm_launch(p, igemm_halo_kernel<bf16, BM_, BN_, 4, 4>, s, d, p.halo_bytes)
        FFN_HALO(128, 320);
        FFN_HALO(256, 128);
        FFN_HALO(256, 256);
        FFN_HALO(128, 128);
#undef FFN_HALO
        break;
    case IG_PP:
    case IG_PP_TRANS:
        if (p.x3) rc = conv ? launch_pp<AMODE_CONV3, true>(p, s, d) : launch_pp<AMODE_DENSE, true>(p, s, d);
        else if (p.f8) rc = launch_pp<AMODE_CONV3, false, true>(p, s, d);
        else rc = conv ? launch_pp<AMODE_CONV3>(p, s, d) : launch_pp<AMODE_DENSE>(p, s, d);
        break;
    }
    if (rc || p.splitk == 1) return rc;
    const dim3 grid(grid_for((long)d.M * (d.N / 4)));
    if (p.reduce_f32) LAUNCH(igemm_splitk_reduce_kernel<float>, grid, dim3(256), 0, s, d, p.splitk);
    else LAUNCH(igemm_splitk_reduce_kernel<bf16>, grid, dim3(256), 0, s, d, p.splitk);
    return check_launch("igemm_splitk_reduce");
}
// first use of a problem shape outside stream capture: time its candidates on the caller's stream with the caller's buffers, cache the winner
static int igemm_tune_now(hipStream_t s, int dtype, const ffn_igemm_desc& d) {
    std::lock_guard<std::mutex> lk(g_tune_mu);       // one tuning at a time
    IgChoice cand[40];
    const int nc = candidates_for(d, cand, 40);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return igemm_run(s, dtype, d, &cand[0]);
    IgChoice best = cand[0];
    float best_ms = 1e30f;
    const int reps = 3;
    for (int i = 0; i < nc; ++i) {
        int rc = igemm_run(s, dtype, d, &cand[i]);      // warm (LDS opt-in, code load)
        if (rc) continue;
        float ms = 1e30f;
        for (int round = 0; round < 2 && !rc; ++round) {       // min of two timed groups: one noisy group must not pick the configuration
            (void)hipEventRecord(e0, s);
            for (int r = 0; r < reps && !rc; ++r) rc = igemm_run(s, dtype, d, &cand[i]);
            (void)hipEventRecord(e1, s);
            if (rc || hipEventSynchronize(e1) != hipSuccess) { rc = rc ? rc : FFN_EHIP; break; }
            float t = 0.f;
            (void)hipEventElapsedTime(&t, e0, e1);
            if (t < ms) ms = t;
        }
        if (rc) continue;
        if (ms < best_ms) { best_ms = ms; best = cand[i]; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    g_tuned[tune_key(d)] = TunedEntry{best, true};
    static const bool verbose = getenv("FFN_IGEMM_TUNE_VERBOSE") != nullptr;
    if (verbose)
        fprintf(stderr, "[ffn tune] %s M=%d N=%d K=%d flags=%d -> %dx%d split %d (%.1f us, %d candidates)\n", d.conv ? "conv" : "dense", d.M, d.N,
                d.K, d.flags, kCfg[best.cfg].bm, kCfg[best.cfg].bn, best.splitk, best_ms * 1e3f / reps, nc);
    return igemm_run(s, dtype, d, &best);       // the output now holds the winner's result
}
// ---- the tuned table as data: export / import (persist it across processes, broadcast rank 0's table so that every rank of a
// sharded run launches the same configurations -- bf16 results then are bit-identical across ranks)
// entry = [stamp | TuneKey | cfg | splitk]; the stamp names the layout of this build's table (key size, configuration list, arch):
// entries written by a different build are ignored on import
static constexpr int kTuneEntryInts = (int)(sizeof(TuneKey) / sizeof(int)) + 3;
static constexpr int kTuneStamp = 0x67780000 ^ (950 << 4) ^ ((int)sizeof(TuneKey) << 8) ^ CFG_COUNT ^ (4 << 24);      // gfx950, table layout 4 (round 5: blocked split-bf16 operands)
extern "C" int ffn_igemm_tune_entry_ints(void) { return kTuneEntryInts; }
extern "C" int ffn_igemm_tune_stamp(void) { return kTuneStamp; }
extern "C" int ffn_igemm_tune_clear(void) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    const int n = (int)g_tuned.size();
    g_tuned.clear();
    return n;
}
extern "C" int ffn_igemm_tune_enable(int on) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    const int prev = g_tune_runtime;
    g_tune_runtime = on ? 1 : 0;
    return prev;
}
extern "C" int ffn_igemm_tune_export(int* buf, int max_entries) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    int n = 0;
    for (const auto& kv : g_tuned) {
        if (buf && n < max_entries) {
            int* e = buf + (long)n * kTuneEntryInts;
            e[0] = kTuneStamp;
            memcpy(e + 1, &kv.first, sizeof(TuneKey));
            e[kTuneEntryInts - 2] = kv.second.ch.cfg;
            e[kTuneEntryInts - 1] = kv.second.ch.splitk;
        }
        ++n;
    }
    return n;       // number of entries in the table (may exceed max_entries: call again with a larger buffer)
}
extern "C" int ffn_igemm_tune_import(const int* buf, int n_entries) {
    REQUIRE(buf || n_entries == 0, "igemm_tune_import: null buffer");
    std::lock_guard<std::mutex> lk(g_tune_mu);
    int n = 0;
    for (int i = 0; i < n_entries; ++i) {
        const int* e = buf + (long)i * kTuneEntryInts;
        if (e[0] != kTuneStamp) continue;                                       // a table from another build / layout / arch
        TuneKey k;
        memcpy(&k, e + 1, sizeof(TuneKey));
        const IgChoice ch{e[kTuneEntryInts - 2], e[kTuneEntryInts - 1]};
        if (ch.cfg < 0 || ch.cfg >= CFG_COUNT || ch.splitk < 1) continue;
        g_tuned[k] = TunedEntry{ch, false};      // validated against the actual problem (candidates_for) at its first lookup
        ++n;
    }
    return n;
}
// shape and flag checks of a descriptor (no buffer is looked at: ffn_igemm_kernel_name asks too)
static int igemm_validate(int dtype, const ffn_igemm_desc& d) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16 || dtype == FFN_BF16X3 || dtype == FFN_FP8, "igemm: bad dtype %d", dtype);
    if (dtype == FFN_FP8) {
        REQUIRE(d.conv && d.Cin > 0 && d.Cin % 16 == 0 && d.K == 9 * d.Cin && d.Kpad >= d.K && d.Kpad % 16 == 0 && d.lda == d.Cin,
                "igemm(fp8): 3x3 convolutions with Cin %% 16 == 0 only (Cin=%d, K=%d, Kpad=%d, lda=%d)", d.Cin, d.K, d.Kpad, d.lda);
        REQUIRE(d.M > 0 && d.N > 0 && d.N % 4 == 0 && d.ldo % 4 == 0 && d.rows_per_batch > 0 && d.M % (d.Hout * d.Wout) == 0, "igemm(fp8): bad shape");
        REQUIRE(!(d.flags & (FFN_IG_GEGLU | FFN_IG_OUT_TRANSPOSED | FFN_IG_OUT_PAIR | FFN_IG_OUT_F32)), "igemm(fp8): plain / SiLU / residual epilogues only");
        REQUIRE(d.stride == 1 || d.stride == 2, "igemm(fp8): stride %d", d.stride);
        int ex = 0;
        REQUIRE(d.alpha > 0.f && frexpf(d.alpha, &ex) == 0.5f, "igemm(fp8): alpha must be a power of two (the un-scaling of two power-of-two operand scales)");
        if (d.residual) REQUIRE(d.ldr % 4 == 0 && d.ldr >= d.N, "igemm(fp8): ldr=%d must be a multiple of 4 and >= N=%d", d.ldr, d.N);
        REQUIRE(d.ldo >= d.N, "igemm(fp8): ldo=%d must be >= N=%d", d.ldo, d.N);
        return FFN_OK;
    }
    const int epc = dtype == FFN_F32 ? 4 : 8;
    const int kmul = dtype == FFN_BF16X3 ? (d.x3 == 2 ? 2 : 3) : 1;       // W row: [hi | lo | hi] planes (3 K) or [hi(32) | lo(32)] blocks (2 K)
    REQUIRE(d.M > 0 && d.N > 0 && d.K > 0, "igemm: empty problem M=%d N=%d K=%d", d.M, d.N, d.K);
    REQUIRE(d.Kpad >= kmul * d.K && d.Kpad % epc == 0, "igemm: Kpad=%d (row stride of W) must be >= %d x K=%d and a multiple of %d", d.Kpad, kmul, d.K, epc);
    if (dtype == FFN_BF16X3) {
        const int plane = d.conv ? d.Cin : d.K;
        if (d.x3 == 2) {
            REQUIRE(plane % 32 == 0 && d.a_lo == 32 && d.lda >= 2 * plane, "igemm: blocked split-bf16 operands need K (conv: Cin) %% 32 == 0, a_lo = 32, lda >= 2 x that (%d, a_lo=%d, lda=%d)", plane, d.a_lo, d.lda);
        } else {
            REQUIRE(d.a_lo % 8 == 0 && d.a_lo >= plane && d.a_lo + plane <= d.lda, "igemm: split-bf16 A needs planes of %d elements: a_lo=%d, lda=%d", plane, d.a_lo, d.lda);
        }
        REQUIRE(d.lda % 8 == 0, "igemm: lda=%d must be a multiple of 8", d.lda);
        REQUIRE(d.alpha == 1.0f, "igemm: split-bf16 problems take alpha = 1");
    }
    REQUIRE(d.K % epc == 0, "igemm: K=%d must be a multiple of %d", d.K, epc);
    REQUIRE(d.rows_per_batch > 0, "igemm: rows_per_batch must be > 0");
    if (d.conv) {
        REQUIRE(d.Cin % epc == 0, "igemm: Cin=%d must be a multiple of %d", d.Cin, epc);
        if (d.conv == 2) {
            REQUIRE((dtype == FFN_BF16 || dtype == FFN_BF16X3) && d.K == 4 * d.Cin && d.stride == 1 && d.upsample == 0 && d.pad >= 0 && d.pad <= 3 && d.splitk <= 1,
                    "igemm: 2x2 convolution needs FFN_BF16 / FFN_BF16X3, K = 4*Cin, stride 1, no upsample, pad in 0..3, no forced split");
            int bm, bn;
            REQUIRE(conv2_tile(igemm_view(dtype, d), &bm, &bn), "igemm: 2x2 convolution M=%d N=%d Cin=%d fits no ping-pong tile (Cin %% 64 (split-bf16: 32), N %% 256 / 320, M >= 192)", d.M, d.N, d.Cin);
        } else {
            REQUIRE(d.conv == 1, "igemm: conv=%d", d.conv);
            REQUIRE(d.K == 9 * d.Cin, "igemm: conv K=%d != 9*Cin=%d", d.K, 9 * d.Cin);
        }
        REQUIRE(d.stride == 1 || d.stride == 2, "igemm: stride %d", d.stride);
        REQUIRE(d.upsample == 0 || d.upsample == 1, "igemm: upsample %d", d.upsample);
        REQUIRE(d.M % (d.Hout * d.Wout) == 0, "igemm: M=%d not a multiple of Hout*Wout", d.M);
    } else {
        REQUIRE(d.lda % epc == 0, "igemm: lda=%d must be a multiple of %d", d.lda, epc);
    }
    if (d.flags & FFN_IG_OUT_KV64) {
        REQUIRE(dtype == FFN_BF16X3 && !d.conv && !d.residual && !d.rowbias && d.splitk <= 1 &&
                    !(d.flags & (FFN_IG_GEGLU | FFN_IG_OUT_PAIR | FFN_IG_OUT_SILU | FFN_IG_OUT_GELU | FFN_IG_OUT_RELU | FFN_IG_OUT_QGELU)),
                "igemm: FFN_IG_OUT_KV64 needs FFN_BF16X3, dense A, the plain epilogue and no forced split-K");
        if (d.flags & FFN_IG_OUT_TRANSPOSED) REQUIRE(d.rows_per_batch % 64 == 0 && d.M % d.rows_per_batch == 0 && d.ldo >= d.rows_per_batch && d.ldo % 64 == 0,
                                                     "igemm: KV64 transposed output needs rows_per_batch %% 64 == 0, whole batches, ldo %% 64 == 0 (rows_per_batch=%d, ldo=%d)", d.rows_per_batch, d.ldo);
        else REQUIRE(d.kv64_from >= 0 && d.kv64_from < d.N && d.kv64_from % 64 == 0 && d.N % 64 == 0 && d.ldo % 4 == 0,
                     "igemm: KV64 output needs kv64_from and N %% 64 == 0 (kv64_from=%d, N=%d)", d.kv64_from, d.N);
    }
    if (d.flags & FFN_IG_OUT_TRANSPOSED) {
        REQUIRE(!d.conv, "igemm: transposed output is only supported for dense A");
        REQUIRE(d.ldo % 4 == 0, "igemm: transposed ldo=%d must be a multiple of 4", d.ldo);
        REQUIRE(!(d.flags & (FFN_IG_GEGLU | FFN_IG_OUT_F32 | FFN_IG_OUT_SILU | FFN_IG_OUT_GELU | FFN_IG_OUT_RELU | FFN_IG_OUT_QGELU)) && !d.residual && !d.rowbias,
                "igemm: transposed output supports bias only");
    } else {
        REQUIRE(d.N % 4 == 0 && d.ldo % 4 == 0, "igemm: N=%d and ldo=%d must be multiples of 4", d.N, d.ldo);
        if (d.residual) REQUIRE(d.ldr % 4 == 0, "igemm: ldr=%d must be a multiple of 4", d.ldr);
        if (d.flags & FFN_IG_OUT_PAIR) {
            const int nout = (d.flags & FFN_IG_GEGLU) ? d.N / 2 : d.N;
            REQUIRE(dtype == FFN_BF16X3 && d.ldo % 16 == 0 && d.ldo / 2 >= nout, "igemm: pair output needs FFN_BF16X3, ldo %% 16 == 0, ldo/2 >= columns");
            REQUIRE(d.residual != d.out, "igemm: pair output cannot overwrite its fp32 residual");
            REQUIRE((d.ldo / 2) % 32 != 0 || nout % 32 == 0 || nout == d.ldo / 2, "igemm: blocked pair output (ldo/2 %% 32 == 0) needs whole 32-column blocks");
            // every producer derives the layout (blocked / planes) from the ROW WIDTH ldo / 2; the ping-pong GEGLU epilogue always writes blocked rows
            REQUIRE(nout == d.ldo / 2 || (d.ldo / 2) % 32 == 0, "igemm: pair output into a wider row needs ldo/2 %% 32 == 0 (ldo=%d, columns=%d)", d.ldo, nout);
        }
        if (d.flags & FFN_IG_GEGLU) {
            REQUIRE(d.N % 64 == 0, "igemm: GEGLU needs N %% 64 == 0 (N=%d)", d.N);
            REQUIRE(!d.residual && !d.rowbias && !(d.flags & (FFN_IG_OUT_F32 | FFN_IG_OUT_SILU | FFN_IG_OUT_GELU | FFN_IG_OUT_RELU | FFN_IG_OUT_QGELU)), "igemm: GEGLU epilogue is exclusive");
        }
    }
    const int act = d.flags & (FFN_IG_OUT_SILU | FFN_IG_OUT_GELU | FFN_IG_OUT_RELU | FFN_IG_OUT_QGELU);
    REQUIRE((act & (act - 1)) == 0, "igemm: SILU / GELU / QGELU / RELU are mutually exclusive");
    REQUIRE(d.splitk >= 0, "igemm: splitk must be >= 0");
    // row strides cover what a row holds (no kernel looks at them for overlap: a short stride would make neighbouring rows share memory)
    if (!d.conv && dtype != FFN_BF16X3) REQUIRE(d.lda >= d.K, "igemm: lda=%d must be >= K=%d", d.lda, d.K);
    if (d.flags & FFN_IG_OUT_TRANSPOSED) {
        const int cols = d.rows_per_batch < d.M ? d.rows_per_batch : d.M;
        REQUIRE(d.ldo >= cols, "igemm: transposed ldo=%d must be >= the %d rows of a batch", d.ldo, cols);
    } else if (!(d.flags & FFN_IG_OUT_PAIR)) {
        const int nout = (d.flags & FFN_IG_GEGLU) ? d.N / 2 : d.N;
        REQUIRE(d.ldo >= nout, "igemm: ldo=%d must be >= the %d output columns", d.ldo, nout);
    }
    if (d.residual) REQUIRE(d.ldr >= d.N, "igemm: ldr=%d must be >= N=%d", d.ldr, d.N);
    return FFN_OK;
}
static bool tuned_family(int dtype, const ffn_igemm_desc& d) { return dtype != FFN_F32 && !(d.flags & FFN_IG_OUT_TRANSPOSED); }
extern "C" int ffn_igemm_kernel_name(int dtype, const ffn_igemm_desc* d0, char* buf, int len) {
    REQUIRE(d0 && buf && len > 0, "igemm_kernel_name: null argument");
    if (int rc = igemm_validate(dtype, *d0)) return rc;
    const ffn_igemm_desc d = igemm_view(dtype, *d0);
    const bool tuned = tuned_family(dtype, d);
    IgChoice ch;
    if (tuned && !known_choice(d, &ch)) ch = heuristic_choice(d);
    IgemmPlan p;
    if (int rc = igemm_plan(dtype, d, tuned ? &ch : nullptr, &p)) return rc;
    auto b = [](bool v) { return v ? "true" : "false"; };
    switch (p.kind) {
    case IG_RING:
        snprintf(buf, len, "void igemm_glds_kernel<%s, %d, %d, %d, %s, 2, %d, %d, %s, %s, %s>(ffn_igemm_desc)", p.f32 ? "float" : "bf16", p.bm, p.bn, p.amode,
                 b(p.swap), p.nwm, p.nwn, b(p.fastk), b(p.x3), b(p.f8));
        break;
    case IG_HALO: snprintf(buf, len, "void igemm_halo_kernel<bf16, %d, %d, %d, %d>(ffn_igemm_desc, int)", p.bm, p.bn, p.nwm, p.nwn); break;
    case IG_PP:
    case IG_PP_TRANS:
        snprintf(buf, len, "void igemm_pp_kernel<%d, %d, %d, %s, %s, %s, %s, %s, %s>(ffn_igemm_desc, int)", p.bm, p.bn, p.amode, b(p.res), b(p.geglu), b(p.split),
                 b(p.kind == IG_PP_TRANS), b(p.x3), b(p.f8));
        break;
    }
    return FFN_OK;
}
extern "C" int ffn_igemm(void* stream, int dtype, const ffn_igemm_desc* d0) {
    REQUIRE(d0, "igemm: null descriptor");
    if (int rc = igemm_validate(dtype, *d0)) return rc;
    if (dtype == FFN_FP8) {
        REQUIRE(d0->A && d0->W && d0->out && aligned16(d0->A) && aligned16(d0->W) && aligned16(d0->out), "igemm(fp8): A/W/out must be non-null and 16-byte aligned");
    } else {
        REQUIRE(d0->A && d0->W && d0->out, "igemm: null A/W/out");
        REQUIRE(aligned16(d0->A) && aligned16(d0->W) && aligned16(d0->out), "igemm: A/W/out must be 16-byte aligned");
    }
    // the residual is read four columns per lane: 16 bytes of fp32 (FFN_F32, FFN_BF16X3), 8 bytes of bf16 (FFN_BF16, FFN_FP8)
    if ((dtype == FFN_BF16X3 || dtype == FFN_F32) && d0->residual) REQUIRE(aligned16(d0->residual), "igemm: fp32 residual must be 16-byte aligned");
    if ((dtype == FFN_BF16 || dtype == FFN_FP8) && d0->residual)
        REQUIRE((reinterpret_cast<uintptr_t>(d0->residual) & 7) == 0, "igemm%s: bf16 residual must be 8-byte aligned", dtype == FFN_FP8 ? "(fp8)" : "");
    if (d0->ws) REQUIRE(aligned16(d0->ws) && d0->ws_bytes >= 0, "igemm%s: workspace must be 16-byte aligned", dtype == FFN_FP8 ? "(fp8)" : "");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const ffn_igemm_desc d = igemm_view(dtype, *d0);
    if (!tuned_family(dtype, d)) return igemm_run(s, dtype, d, nullptr);
    IgChoice ch;
    if (!known_choice(d, &ch)) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &cap);
        // (out aliasing residual: repeated launches would accumulate -- never time such a call)
        if (tune_enabled() && cap == hipStreamCaptureStatusNone && d.residual != d.out) return igemm_tune_now(s, dtype, d);
        ch = heuristic_choice(d);
    }
    return igemm_run(s, dtype, d, &ch);
}

extern "C" int ffn_igemm_tune(void* stream, int dtype, const ffn_igemm_desc* d) { return ffn_igemm(stream, dtype, d); }
