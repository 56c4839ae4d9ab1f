// C ABI of libfreefine_hip.so (see include/freefine_hip.h).  Host-side launch glue only: argument validation,
// tile selection, dynamic-LDS opt-in.  No allocation, no synchronisation, everything on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <initializer_list>
#include <mutex>
#include <unordered_map>
#include <stdlib.h>
#include <string.h>

#include "../../include/freefine_hip.h"
#include "attention.h"
#include "attention_pp.h"
#include "attention_x.h"
#include "attention_x3.h"
#include "attention_x3p.h"
#include "attention_xx3.h"
#include "conv_small.h"
#include "elementwise.h"
#include "igemm.h"
#include "igemm_p8.h"
#include "norms.h"
#include "splat.h"

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FFN_EHIP, "%s: %s", what, hipGetErrorString(e));
    return FFN_OK;
}
// a stale error left behind by an unrelated earlier HIP call (e.g. a tool's probe) must not be blamed on our launch
#define LAUNCH(...)                  \
    do {                             \
        (void)hipGetLastError();     \
        hipLaunchKernelGGL(__VA_ARGS__); \
    } while (0)
#define REQUIRE(cond, ...) \
    do {                   \
        if (!(cond)) return fail(FFN_EINVAL, __VA_ARGS__); \
    } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int grid_for(long n, int per_block = 256, int cap = 4096) {
    long g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

template <typename K>
static int set_lds(K kernel, int bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, int> done;   // one opt-in per (kernel, size)
    if (bytes > 48 * 1024) {
        std::lock_guard<std::mutex> lk(mu);
        int& have = done[reinterpret_cast<const void*>(kernel)];
        if (have >= bytes) return FFN_OK;
        have = bytes;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return fail(FFN_EHIP, "hipFuncSetAttribute(%d): %s", bytes, hipGetErrorString(e));
    }
    return FFN_OK;
}

extern "C" int ffn_version(void) { return 14; }      // 14: automatic mask generation (ffn_upsample_bicubic_stats, ffn_box_nms); 13: the GeoDiffuser warp of GeoBench-3D (ffn_geo_project, ffn_splat_composite, ffn_mesh_cover); 12: SIFT keypoints for Mean Distance (ffn_sift_base, ffn_gauss_blur_f32, ffn_decimate2_f32, ffn_sift_extrema, ffn_sift_refine_orient, ffn_sift_describe, ffn_knn2_u8; FFN_ENOSPC); 11: click-to-mask (ffn_sam_patch_rows, ffn_sam_patch_rows_pair, ffn_hyper_masks, ffn_upsample_bicubic, FFN_ELT_GELU); 10: the correspondence map of the point-cloud warp (ffn_splat_ids, ffn_splat_correspond); 9: the case preparation of the GeoBench harness (ffn_resize_taps8_u8, ffn_resize_gather_u8, ffn_dilate_u8, ffn_mask_bbox_u8, ffn_coarse_edit_2d); 8: ffn_pool_layernorm, ffn_cosine_rows; 2: FFN_ATT_CAUSAL, FFN_IG_OUT_QGELU, ffn_embed_tokens; 3: the igemm tile query is gone (ffn_igemm_kernel_name answers); 4: ffn_dift_match; 5: ffn_resize_pil_bilinear_u8, ffn_vit_patch_rows; 6: ffn_resize_pil_u8; 7: ffn_vit_patch_rows_pair
extern "C" const char* ffn_last_error(void) { return g_err; }
extern "C" int ffn_device_info(int device, char* name, int name_len) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(FFN_EHIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (name && name_len > 0) {
        strncpy(name, prop.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    return prop.multiProcessorCount;
}

extern "C" int ffn_graph_launch(void* stream, void* graph_exec) {
    REQUIRE(graph_exec, "graph_launch: null graph");
    hipError_t e = hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(graph_exec), reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(FFN_EHIP, "hipGraphLaunch: %s", hipGetErrorString(e));
    return FFN_OK;
}

// ---- igemm -------------------------------------------------------------------------------------------------------
static int device_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}
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
extern "C" int ffn_split_pair(void* stream, const float* src, void* dst, long rows, int C, int ld_src) {
    REQUIRE(src && dst && rows > 0 && C > 0 && C % 4 == 0 && ld_src >= C && ld_src % 4 == 0, "split_pair: bad arguments (C=%d, ld_src=%d)", C, ld_src);
    REQUIRE(aligned16(src) && aligned16(dst), "split_pair: pointers must be 16-byte aligned");
    static const int wide = [] { const char* e = getenv("FFN_PAIR8"); return e ? atoi(e) : 1; }();
    if (wide && C % 8 == 0 && ld_src % 4 == 0) LAUNCH(split_pair8_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, (bf16*)dst, rows, C, ld_src);
    else LAUNCH(split_pair_kernel, dim3(grid_for(rows * (C / 4))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, (bf16*)dst, rows, C, ld_src);
    return check_launch("split_pair");
}
extern "C" int ffn_conv3x3_n4(void* stream, int dtype, const void* x, const float* w, const float* bias, float* out, int B, int H, int W, int Cin) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "conv3x3_n4: fp32 or bf16 activations");
    REQUIRE(x && w && out && aligned16(x) && aligned16(w) && aligned16(out) && (!bias || aligned16(bias)), "conv3x3_n4: null / unaligned pointer");
    REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 16 == 0 && Cin <= 448, "conv3x3_n4: B=%d H=%d W=%d Cin=%d (Cin %% 16 == 0, <= 448)", B, H, W, Cin);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long npix = (long)B * H * W;
    const int lds = 36 * Cin * 4;
    dim3 grid((unsigned)((npix + 63) / 64));
    int rc;
    if (dtype == FFN_F32) {
        if ((rc = set_lds(conv3x3_n4_kernel<float>, lds))) return rc;
        LAUNCH(conv3x3_n4_kernel<float>, grid, dim3(256), lds, s, (const float*)x, w, bias, out, B, H, W, Cin);
    } else {
        if ((rc = set_lds(conv3x3_n4_kernel<bf16>, lds))) return rc;
        LAUNCH(conv3x3_n4_kernel<bf16>, grid, dim3(256), lds, s, (const bf16*)x, w, bias, out, B, H, W, Cin);
    }
    return check_launch("conv3x3_n4");
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

// ---- attention ---------------------------------------------------------------------------------------------------
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
// double-buffered K and V^T tiles + the per-wave multi-pass accumulator + the key-mask bytes of the two staged tiles
static constexpr int attn_kernel_lds(int esz, int dp, int qf, int kt) {
    return 2 * (kt * (dp * esz == 128 ? 128 : dp * esz + 16) + dp * ((dp * esz == 128 && kt * esz == 128) ? 128 : kt * esz + 16)) + 4 * (dp / 16) * qf * 64 * 16 + 2 * kt;
}
static_assert(attn_kernel_lds(4, 160, 1, 32) <= 160 * 1024 && attn_kernel_lds(2, 160, 1, 64) <= 160 * 1024, "attention tile does not fit the 160 KiB LDS");

// attn_x3w_kernel lives in its own translation unit (attn_x3w.hip: different code generation flags)
typedef void (*attn_x3w_t)(ffn_attn_desc);
extern "C" __attribute__((visibility("hidden"))) attn_x3w_t fx3w_kernel(int masks);
extern "C" __attribute__((visibility("hidden"))) int fx3w_lds_bytes(void);
// attn_causal_kernel and embed_tokens_kernel live in a third one (attn_causal.hip)
extern "C" __attribute__((visibility("hidden"))) attn_x3w_t fcausal_kernel(int dtype);
extern "C" __attribute__((visibility("hidden"))) void fembed_launch(hipStream_t s, int bf16_out, const int* ids, const float* table, const float* pos, void* out,
                                                                    long M, int S, int C, int V);

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
static int attn_plan(int dtype, const ffn_attn_desc& d, AttnPlan* p) {
    bool masks = false, uniform = false, xok = true, multi = d.npass != 1;
    bool causal = false, causal_ok = true;
    int maxq = 0, maxkv = 0;
    for (int pi = 0; pi < d.npass; ++pi)
        for (int b = 0; b < d.Bo; ++b) {
            const ffn_attn_entry& e = d.e[pi * FFN_ATT_MAXB + b];
            if (e.w_const == 0.f && e.w_slope == 0.f) { multi = true; continue; }
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
        const int nfr = p->nkf * 2 + 4 * ((p->nkf + 1) / 2);   // 1 KiB fragment images per pass: hi and lo each
        if (p->nkf && d.npass * 2 * nfr * 1024 <= 160 * 1024) {
            // 8 waves per workgroup where the fragment images are large against a workgroup's share of the queries (two passes: 88 KiB, one workgroup
            // per CU either way) or the launch is long; 4 (two workgroups per CU) for the short single-pass launches (profiles/r5_xattn_x3_waves_and_stores.txt)
            p->kind = ATT_XX3;
            p->nw = (d.npass >= 2 || d.S >= 4096) ? 8 : 4;
            p->lds = d.npass * 2 * nfr * 1024;
            p->block = dim3(64 * p->nw);
        } else if (pp && d.kv_pair) {                           // one wave per SIMD on 32x32x16 MFMAs
            p->kind = ATT_X3W;
            p->lds = fx3w_lds_bytes();
            p->block = dim3(256);
        } else if (pp) {
            p->kind = ATT_X3P;
            p->lds = 5 * (2 * 8192) + 8 * 4 * 2 * 64 * 16;      // K ring of 2 + V^T ring of 3 [hi | lo] images, multi-pass sums
        } else {
            p->kind = ATT_X3;
            p->lds = 2 * (4 * 8192) + 8 * 4 * 2 * 64 * 16;
        }
    } else if (dtype == FFN_BF16 && (p->nkf = xattn_nkf(2))) {
        // one pass of plain active entries: K / V^T of a (row, head) in a wave's registers; several passes, skipped entries or per-query
        // weights: one workgroup of 4 waves per (row, head, chunk) with the fragment images of every pass in LDS
        p->kind = multi ? ATT_X_MP : ATT_X;
        p->nw = multi ? 4 : 1;
        p->lds = multi ? d.npass * (p->nkf * 2 + 4 * ((p->nkf + 1) / 2)) * 1024 : 0;
        p->block = dim3(256);
    } else if (dtype == FFN_BF16 && pp) {
        p->kind = ATT_PP;
        p->lds = 4 * 8192 + 4 * 8192 + 4 * 256 + 8 * 4 * 2 * 64 * 16;
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

// ---- token + position embedding of the text tower ------------------------------------------------------------------------
extern "C" int ffn_embed_tokens(void* stream, int dtype, const int* ids, const float* table, const float* pos, void* out, long M, int S, int C, int V) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16 || dtype == FFN_BF16X3, "embed_tokens: bad dtype %d", dtype);
    REQUIRE(ids && table && pos && out && aligned16(table) && aligned16(pos) && aligned16(out), "embed_tokens: null / unaligned pointer");
    REQUIRE(M > 0 && S > 0 && V > 0 && C > 0 && C % 4 == 0 && M < (1l << 31), "embed_tokens: bad shape M=%ld S=%d C=%d V=%d (C %% 4 == 0)", M, S, C, V);
    fembed_launch(reinterpret_cast<hipStream_t>(stream), dtype == FFN_BF16, ids, table, pos, out, M, S, C, V);
    return check_launch("embed_tokens");
}

// ---- pooled LayerNorm and cosine of the CLIP towers' projections (kernels: attn_causal.hip) ------------------------------------------------
extern "C" __attribute__((visibility("hidden"))) void fpool_ln_launch(hipStream_t s, int bf16_in, int pair, const void* x, const int* ids, void* y,
                                                                      const float* gamma, const float* beta, int N, int S, int C, float eps);
extern "C" __attribute__((visibility("hidden"))) void fcosine_launch(hipStream_t s, const float* a, const float* b, float* out, int B, int P, int b_rows);

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
    fpool_ln_launch(reinterpret_cast<hipStream_t>(stream), dtype == FFN_BF16, pair, x, ids, y, gamma, beta, N, S, C, eps);
    return check_launch("pool_layernorm");
}

extern "C" int ffn_cosine_rows(void* stream, const float* a, const float* b, float* out, int B, int P, int b_rows) {
    REQUIRE(a && b && out, "cosine_rows: null pointer");
    REQUIRE(aligned16(a) && aligned16(b) && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "cosine_rows: a, b must be 16-byte aligned, out 4-byte aligned");
    REQUIRE(B > 0 && P > 0 && P % 4 == 0, "cosine_rows: bad shape B=%d P=%d (P %% 4 == 0)", B, P);
    REQUIRE(b_rows == 1 || b_rows == B, "cosine_rows: b has %d rows (1 or B=%d)", b_rows, B);
    fcosine_launch(reinterpret_cast<hipStream_t>(stream), a, b, out, B, P, b_rows);
    return check_launch("cosine_rows");
}

// ---- DIFT correspondence search (kernels and launch sequence: dift.hip / dift_match.h) -----------------------------------------------------------
extern "C" __attribute__((visibility("hidden"))) long fdift_ws_bytes(int C, int h, int w, int K);
extern "C" __attribute__((visibility("hidden"))) void fdift_launch(hipStream_t s, const ffn_dift_desc* d);

extern "C" long ffn_dift_workspace_bytes(int C, int h, int w, int K) {
    REQUIRE(C > 0 && C % 4 == 0 && h >= 1 && w >= 1 && K >= 1 && (long)h * w < (1l << 31), "dift_workspace_bytes: bad shape C=%d h=%d w=%d K=%d (C %% 4 == 0)", C, h, w, K);
    return fdift_ws_bytes(C, h, w, K);
}

extern "C" int ffn_dift_match(void* stream, const ffn_dift_desc* dp) {
    REQUIRE(dp, "dift_match: null descriptor");
    const ffn_dift_desc& d = *dp;
    REQUIRE(d.dtype == FFN_F32 || d.dtype == FFN_BF16, "dift_match: bad dtype %d", d.dtype);
    const int epc = d.dtype == FFN_F32 ? 4 : 8;
    REQUIRE(d.C > 0 && d.C % 4 == 0 && d.E >= 1 && d.K >= 1 && d.h >= 1 && d.w >= 1 && d.H >= 1 && d.W >= 1,
            "dift_match: bad shape E=%d C=%d h=%d w=%d H=%d W=%d K=%d (C %% 4 == 0, everything else >= 1)", d.E, d.C, d.h, d.w, d.H, d.W, d.K);
    REQUIRE((long)d.H * d.W < (1l << 31) && (long)d.h * d.w < (1l << 31), "dift_match: H * W and h * w must be below 2^31");
    REQUIRE(d.ld >= d.C && d.ld % epc == 0 && d.es >= 0 && d.es % epc == 0, "dift_match: ld=%d (>= C=%d) and es=%ld must be multiples of %d", d.ld, d.C, d.es, epc);
    REQUIRE(d.src && d.tgt && d.kps && d.ws && d.out_rc && d.out_cos && aligned16(d.src) && aligned16(d.tgt) && aligned16(d.ws), "dift_match: null / unaligned pointer");
    const long need = fdift_ws_bytes(d.C, d.h, d.w, d.K);
    REQUIRE(d.ws_bytes >= need, "dift_match: workspace of %ld bytes, %ld needed (ffn_dift_workspace_bytes)", d.ws_bytes, need);
    for (int k = 0; k < d.K; ++k)
        REQUIRE(d.kps[2 * k] >= 0 && d.kps[2 * k] < d.H && d.kps[2 * k + 1] >= 0 && d.kps[2 * k + 1] < d.W, "dift_match: keypoint %d = (%d, %d) outside [0, %d) x [0, %d)", k,
                d.kps[2 * k], d.kps[2 * k + 1], d.H, d.W);
    fdift_launch(reinterpret_cast<hipStream_t>(stream), &d);
    return check_launch("dift_match");
}

// ---- SIFT keypoints, descriptors and matching of the Mean Distance metric (kernels: sift.h, compiled in dift.hip) -------------------------------------------

extern "C" __attribute__((visibility("hidden"))) void fsift_base(hipStream_t s, const uint8_t* img, float* out, int H, int W, int C);
extern "C" __attribute__((visibility("hidden"))) void fsift_blur(hipStream_t s, const float* src, float* dst, float* tmp, int H, int W, const float* taps, int T);
extern "C" __attribute__((visibility("hidden"))) void fsift_decimate(hipStream_t s, const float* src, float* dst, int H, int W);
extern "C" __attribute__((visibility("hidden"))) int fsift_extrema(hipStream_t s, const float* G, float* D, int h, int w, int* cand, int cap, int* counter, int* found);
extern "C" __attribute__((visibility("hidden"))) void fsift_refine(hipStream_t s, const float* D, const float* G, int h, int w, int o, const int* cand, int n, float* out);
extern "C" __attribute__((visibility("hidden"))) void fsift_describe(hipStream_t s, const float* G, int h, int w, int o, const float* kp, int n, uint8_t* desc, float* raw);
extern "C" __attribute__((visibility("hidden"))) void fknn2_u8(hipStream_t s, const uint8_t* des1, int n1, const uint8_t* des2, int n2, int* idx, int* dist);

static inline bool sift_side_ok(int h, int w) { return h >= 1 && w >= 1 && h <= FFN_SIFT_MAX_SIDE && w <= FFN_SIFT_MAX_SIDE; }

extern "C" int ffn_sift_base(void* stream, const uint8_t* img, float* out, int H, int W, int C) {
    REQUIRE(img && out, "sift_base: null pointer");
    REQUIRE(H >= 1 && W >= 1 && 2 * H <= FFN_SIFT_MAX_SIDE && 2 * W <= FFN_SIFT_MAX_SIDE && (C == 1 || C == 3), "sift_base: bad shape H=%d W=%d C=%d (C in {1, 3}, sides <= %d)", H, W,
            C, FFN_SIFT_MAX_SIDE / 2);
    fsift_base(reinterpret_cast<hipStream_t>(stream), img, out, H, W, C);
    return check_launch("sift_base");
}

extern "C" int ffn_gauss_blur_f32(void* stream, const float* src, float* dst, float* tmp, int H, int W, const float* taps, int T) {
    REQUIRE(src && dst && tmp && taps, "gauss_blur_f32: null pointer");
    REQUIRE(tmp != src && tmp != dst, "gauss_blur_f32: tmp must be a buffer of its own");
    REQUIRE(sift_side_ok(H, W), "gauss_blur_f32: bad shape H=%d W=%d (sides 1 .. %d)", H, W, FFN_SIFT_MAX_SIDE);
    REQUIRE(T >= 1 && T <= FFN_SIFT_MAX_TAPS && (T & 1), "gauss_blur_f32: %d taps (odd, 1 .. %d)", T, FFN_SIFT_MAX_TAPS);
    fsift_blur(reinterpret_cast<hipStream_t>(stream), src, dst, tmp, H, W, taps, T);
    return check_launch("gauss_blur_f32");
}

extern "C" int ffn_decimate2_f32(void* stream, const float* src, float* dst, int H, int W) {
    REQUIRE(src && dst && src != dst, "decimate2_f32: null or aliased pointer");
    REQUIRE(sift_side_ok(H, W) && H >= 2 && W >= 2, "decimate2_f32: bad shape H=%d W=%d (sides 2 .. %d)", H, W, FFN_SIFT_MAX_SIDE);
    fsift_decimate(reinterpret_cast<hipStream_t>(stream), src, dst, H, W);
    return check_launch("decimate2_f32");
}

extern "C" int ffn_sift_extrema(void* stream, const float* gauss, float* dog, int h, int w, int* cand, int cap, int* counter, int* count) {
    REQUIRE(gauss && dog && cand && counter && count, "sift_extrema: null pointer");
    REQUIRE(sift_side_ok(h, w) && cap >= 1, "sift_extrema: bad shape h=%d w=%d cap=%d (sides 1 .. %d, cap >= 1)", h, w, cap, FFN_SIFT_MAX_SIDE);
    *count = 0;
    const int e = fsift_extrema(reinterpret_cast<hipStream_t>(stream), gauss, dog, h, w, cand, cap, counter, count);
    if (e != 0) return fail(FFN_EHIP, "sift_extrema: %s", hipGetErrorString((hipError_t)e));
    if (*count > cap) return fail(FFN_ENOSPC, "sift_extrema: %d extrema but room for %d: call again with a longer list", *count, cap);
    return check_launch("sift_extrema");
}

extern "C" int ffn_sift_refine_orient(void* stream, const float* dog, const float* gauss, int h, int w, int octave, const int* cand, int n, float* out) {
    REQUIRE(n >= 0, "sift_refine_orient: n=%d", n);
    if (n == 0) return FFN_OK;
    REQUIRE(dog && gauss && cand && out, "sift_refine_orient: null pointer");
    REQUIRE(sift_side_ok(h, w) && octave >= 0 && octave < 24, "sift_refine_orient: bad shape h=%d w=%d octave=%d", h, w, octave);
    fsift_refine(reinterpret_cast<hipStream_t>(stream), dog, gauss, h, w, octave, cand, n, out);
    return check_launch("sift_refine_orient");
}

extern "C" int ffn_sift_describe(void* stream, const float* gauss, int h, int w, int octave, const float* kp, int n, uint8_t* desc, float* raw) {
    REQUIRE(n >= 0, "sift_describe: n=%d", n);
    if (n == 0) return FFN_OK;
    REQUIRE(gauss && kp && desc, "sift_describe: null pointer");
    REQUIRE(sift_side_ok(h, w) && octave >= 0 && octave < 24, "sift_describe: bad shape h=%d w=%d octave=%d", h, w, octave);
    fsift_describe(reinterpret_cast<hipStream_t>(stream), gauss, h, w, octave, kp, n, desc, raw);
    return check_launch("sift_describe");
}

extern "C" int ffn_knn2_u8(void* stream, const uint8_t* des1, int n1, const uint8_t* des2, int n2, int* idx, int* dist) {
    REQUIRE(n1 >= 0 && n2 >= 0, "knn2_u8: n1=%d n2=%d", n1, n2);
    if (n1 == 0) return FFN_OK;
    REQUIRE(des1 && idx && dist && (des2 || n2 == 0), "knn2_u8: null pointer");
    REQUIRE((reinterpret_cast<uintptr_t>(des1) & 3) == 0 && (reinterpret_cast<uintptr_t>(des2) & 3) == 0, "knn2_u8: descriptor rows are read as 32-bit words: 4-byte alignment");
    fknn2_u8(reinterpret_cast<hipStream_t>(stream), des1, n1, des2, n2, idx, dist);
    return check_launch("knn2_u8");
}

// ---- device image preparation of the DINOv2 feature metrics (kernels and launches: imgprep.hip / imgprep.h) ----------------------------------------
extern "C" __attribute__((visibility("hidden"))) void fimgprep_resize(hipStream_t s, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int oh, int ow,
                                                                      const int* hb, const int* hk, int hks, const int* vb, const int* vk, int vks);
extern "C" __attribute__((visibility("hidden"))) void fimgprep_patch_rows(hipStream_t s, int dtype, const uint8_t* src, const float* lut, void* out, int B, int H, int W,
                                                                          int ps, int ldo);

static inline int pil_ksize(int in, int out) { return 2 * (in > out ? (in + out - 1) / out : 1) + 1; }      // 2 ceil(max(in / out, 1)) + 1

extern "C" int ffn_resize_pil_bilinear_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int oh, int ow,
                                          const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef, int vksize) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && dst && scratch && hbounds && hcoef && vbounds && vcoef, "resize_pil_bilinear_u8: null pointer");
    REQUIRE(B >= 1 && B <= 65535, "resize_pil_bilinear_u8: B=%d outside 1 .. 65535", B);
    REQUIRE(H >= 1 && W >= 1 && H <= lim && W <= lim, "resize_pil_bilinear_u8: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", H, W, lim);
    REQUIRE(oh >= 1 && ow >= 1 && oh <= lim && ow <= lim, "resize_pil_bilinear_u8: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", oh, ow, lim);
    REQUIRE(hksize == pil_ksize(W, ow) && vksize == pil_ksize(H, oh), "resize_pil_bilinear_u8: table widths %d, %d; %d -> %d and %d -> %d need %d, %d", hksize, vksize, W, ow,
            H, oh, pil_ksize(W, ow), pil_ksize(H, oh));
    fimgprep_resize(reinterpret_cast<hipStream_t>(stream), src, dst, scratch, B, H, W, oh, ow, hbounds, hcoef, hksize, vbounds, vcoef, vksize);
    return check_launch("resize_pil_bilinear_u8");
}

extern "C" __attribute__((visibility("hidden"))) void fimgprep_resize_win(hipStream_t s, const ffn_resize_pil_desc* d);

extern "C" int ffn_resize_pil_u8(void* stream, const ffn_resize_pil_desc* d) {
    const int lim = FFN_IMGPREP_MAX_SIDE, taps = FFN_IMGPREP_MAX_TAPS;
    REQUIRE(d, "resize_pil_u8: null descriptor");
    REQUIRE(d->src && d->dst && d->scratch && d->hbounds && d->hcoef && d->vbounds && d->vcoef, "resize_pil_u8: null pointer");
    REQUIRE(d->B >= 1 && d->B <= 65535, "resize_pil_u8: B=%d outside 1 .. 65535", d->B);
    REQUIRE(d->C == 1 || d->C == 3, "resize_pil_u8: C=%d channels (1 or 3)", d->C);
    REQUIRE(d->H >= 1 && d->W >= 1 && d->H <= lim && d->W <= lim, "resize_pil_u8: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", d->H, d->W, lim);
    REQUIRE(d->oh >= 1 && d->ow >= 1 && d->oh <= lim && d->ow <= lim, "resize_pil_u8: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", d->oh, d->ow, lim);
    REQUIRE(d->hksize >= 1 && d->vksize >= 1 && d->hksize <= taps && d->vksize <= taps, "resize_pil_u8: table widths %d, %d outside 1 .. %d (FFN_IMGPREP_MAX_TAPS)",
            d->hksize, d->vksize, taps);
    REQUIRE(d->y0 >= 0 && d->x0 >= 0 && d->ch >= 1 && d->cw >= 1 && d->ch <= d->oh - d->y0 && d->cw <= d->ow - d->x0,
            "resize_pil_u8: window (%d, %d, %d, %d) outside the %d x %d destination", d->y0, d->x0, d->ch, d->cw, d->oh, d->ow);
    REQUIRE(d->rule == FFN_KEEP_NONE || d->rule == FFN_KEEP_SUM_LT128 || d->rule == FFN_KEEP_GT128, "resize_pil_u8: unknown keep rule %d", d->rule);
    REQUIRE(d->rule == FFN_KEEP_NONE || d->C == 3, "resize_pil_u8: a keep mask needs C=3 (C=%d)", d->C);
    REQUIRE(d->rule == FFN_KEEP_NONE || d->m1, "resize_pil_u8: keep rule %d without m1 (null pointer)", d->rule);
    fimgprep_resize_win(reinterpret_cast<hipStream_t>(stream), d);
    return check_launch("resize_pil_u8");
}

extern "C" int ffn_vit_patch_rows(void* stream, int dtype, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int patch, int ldo) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "vit_patch_rows: bad dtype %d", dtype);
    REQUIRE(src && lut && out, "vit_patch_rows: null pointer");
    REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= lim && W <= lim, "vit_patch_rows: bad shape B=%d, %d x %d (sides 1 .. %d, FFN_IMGPREP_MAX_SIDE)", B, H, W, lim);
    REQUIRE(patch >= 1 && patch <= 256 && H % patch == 0 && W % patch == 0, "vit_patch_rows: %d x %d is not whole patches of %d (1 .. 256)", H, W, patch);
    REQUIRE(ldo >= 3 * patch * patch, "vit_patch_rows: ldo=%d below the %d columns of a patch", ldo, 3 * patch * patch);
    fimgprep_patch_rows(reinterpret_cast<hipStream_t>(stream), dtype, src, lut, out, B, H, W, patch, ldo);
    return check_launch("vit_patch_rows");
}

extern "C" __attribute__((visibility("hidden"))) void fimgprep_patch_rows_pair(hipStream_t s, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int ps,
                                                                               int K);

// the same rows as the pair operand of an FFN_BF16X3 GEMM (ABI version 7): 8 columns per thread, 16-byte stores
extern "C" int ffn_vit_patch_rows_pair(void* stream, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int patch, int K) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && lut && out, "vit_patch_rows_pair: null pointer");
    REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= lim && W <= lim, "vit_patch_rows_pair: bad shape B=%d, %d x %d (sides 1 .. %d, FFN_IMGPREP_MAX_SIDE)", B, H, W, lim);
    REQUIRE(patch >= 1 && patch <= 256 && H % patch == 0 && W % patch == 0, "vit_patch_rows_pair: %d x %d is not whole patches of %d (1 .. 256)", H, W, patch);
    REQUIRE(K >= 3 * patch * patch, "vit_patch_rows_pair: K=%d below the %d columns of a patch", K, 3 * patch * patch);
    REQUIRE(K % 8 == 0, "vit_patch_rows_pair: K=%d is not a multiple of 8 (16-byte stores of both halves)", K);
    REQUIRE(aligned16(out), "vit_patch_rows_pair: out must be 16-byte aligned");
    fimgprep_patch_rows_pair(reinterpret_cast<hipStream_t>(stream), src, lut, out, B, H, W, patch, K);
    return check_launch("vit_patch_rows_pair");
}

// ---- device case preparation of the GeoBench harness (kernels: caseprep.h, launches: imgprep.hip) ---------------------------------------------------
extern "C" __attribute__((visibility("hidden"))) void fcaseprep_taps8(hipStream_t s, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow,
                                                                      const int* iy, const double* wy, const int* ix, const double* wx);
extern "C" __attribute__((visibility("hidden"))) void fcaseprep_gather(hipStream_t s, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow,
                                                                       const int* iy, const int* ix, int binarise);
extern "C" __attribute__((visibility("hidden"))) void fcaseprep_dilate(hipStream_t s, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int C, int k);
extern "C" __attribute__((visibility("hidden"))) hipError_t fcaseprep_bbox(hipStream_t s, const uint8_t* mask, int* box, int B, int H, int W, int C);
extern "C" __attribute__((visibility("hidden"))) void fcaseprep_edit(hipStream_t s, const ffn_coarse_edit_desc* d);

// the common rules of the case-preparation entries: batch, channels, one image's sides
#define CASEPREP_IMAGE(what, B, H, W, C)                                                                                                                  \
    do {                                                                                                                                                  \
        REQUIRE((B) >= 1 && (B) <= 65535, what ": B=%d outside 1 .. 65535", (B));                                                                       \
        REQUIRE((C) == 1 || (C) == 3, what ": C=%d channels (1 or 3)", (C));                                                                            \
        REQUIRE((H) >= 1 && (W) >= 1 && (H) <= FFN_IMGPREP_MAX_SIDE && (W) <= FFN_IMGPREP_MAX_SIDE, what ": image %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", (H), (W), \
                FFN_IMGPREP_MAX_SIDE);                                                                                                                    \
    } while (0)

extern "C" int ffn_resize_taps8_u8(void* stream, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow, const int* iy, const double* wy,
                                   const int* ix, const double* wx) {
    REQUIRE(src && dst && iy && wy && ix && wx, "resize_taps8_u8: null pointer");
    CASEPREP_IMAGE("resize_taps8_u8", B, H, W, C);
    CASEPREP_IMAGE("resize_taps8_u8", B, oh, ow, C);
    fcaseprep_taps8(reinterpret_cast<hipStream_t>(stream), src, dst, B, H, W, C, oh, ow, iy, wy, ix, wx);
    return check_launch("resize_taps8_u8");
}

extern "C" int ffn_resize_gather_u8(void* stream, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow, const int* iy, const int* ix, int binarise) {
    REQUIRE(src && dst && iy && ix, "resize_gather_u8: null pointer");
    CASEPREP_IMAGE("resize_gather_u8", B, H, W, C);
    CASEPREP_IMAGE("resize_gather_u8", B, oh, ow, C);
    fcaseprep_gather(reinterpret_cast<hipStream_t>(stream), src, dst, B, H, W, C, oh, ow, iy, ix, binarise);
    return check_launch("resize_gather_u8");
}

extern "C" int ffn_dilate_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int C, int k) {
    REQUIRE(src && dst && scratch, "dilate_u8: null pointer");
    CASEPREP_IMAGE("dilate_u8", B, H, W, C);
    REQUIRE(k >= 1 && k <= 255, "dilate_u8: k=%d outside 1 .. 255", k);
    REQUIRE(dst != src && dst != scratch && scratch != src, "dilate_u8: src, scratch and dst must be three buffers");
    fcaseprep_dilate(reinterpret_cast<hipStream_t>(stream), src, dst, scratch, B, H, W, C, k);
    return check_launch("dilate_u8");
}

extern "C" int ffn_mask_bbox_u8(void* stream, const uint8_t* mask, int* box, int B, int H, int W, int C) {
    REQUIRE(mask && box, "mask_bbox_u8: null pointer");
    CASEPREP_IMAGE("mask_bbox_u8", B, H, W, C);
    hipError_t e = fcaseprep_bbox(reinterpret_cast<hipStream_t>(stream), mask, box, B, H, W, C);
    if (e != hipSuccess) return fail(FFN_EHIP, "mask_bbox_u8: hipMemsetAsync: %s", hipGetErrorString(e));
    return check_launch("mask_bbox_u8");
}

extern "C" int ffn_coarse_edit_2d(void* stream, const ffn_coarse_edit_desc* d) {
    REQUIRE(d, "coarse_edit_2d: null descriptor");
    REQUIRE(d->src_img && d->src_mask && d->bg && d->inv && d->final_img && d->tmask && d->trans_hole, "coarse_edit_2d: null pointer");
    CASEPREP_IMAGE("coarse_edit_2d", d->B, d->H, d->W, d->mask_c);
    REQUIRE(!d->hole_mask || d->hole_mask_c == 1 || d->hole_mask_c == 3, "coarse_edit_2d: hole_mask_c=%d channels (1 or 3)", d->hole_mask_c);
    fcaseprep_edit(reinterpret_cast<hipStream_t>(stream), d);
    return check_launch("coarse_edit_2d");
}

// ---- click-to-mask: image preparation, mask product, bicubic upsampling (kernels: sam.h, launches: imgprep.hip) -----------------------------------
extern "C" __attribute__((visibility("hidden"))) void fsam_patch_rows(hipStream_t s, int dtype, const uint8_t* src, void* out, int B, int H, int W, int side, int ps, int ldo,
                                                                      const float* mean, const float* std);
extern "C" __attribute__((visibility("hidden"))) void fsam_patch_rows_pair(hipStream_t s, const uint8_t* src, void* out, int B, int H, int W, int side, int ps, int K,
                                                                           const float* mean, const float* std);
extern "C" __attribute__((visibility("hidden"))) void fsam_hyper_masks(hipStream_t s, const float* up, const float* hyper, float* out, int N, int hw, int C, int M);
extern "C" __attribute__((visibility("hidden"))) void fsam_bicubic(hipStream_t s, const float* src, float* dst, uint8_t* mask, int N, int h, int w, int H, int W);

// the common rules of the two patch-row entries
#define SAM_PATCH_ROWS(what, cols)                                                                                                                        \
    do {                                                                                                                                                  \
        const int lim = FFN_IMGPREP_MAX_SIDE;                                                                                                             \
        REQUIRE(src && out && mean && std, what ": null pointer");                                                                                       \
        REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= lim && W <= lim, what ": bad shape B=%d, %d x %d (sides 1 .. %d, FFN_IMGPREP_MAX_SIDE)", B, H, W, lim); \
        REQUIRE(side >= 1 && side <= lim, what ": side=%d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", side, lim);                                           \
        REQUIRE(patch >= 1 && patch <= 256 && side % patch == 0, what ": side %d is not whole patches of %d (1 .. 256)", side, patch);                   \
        REQUIRE((cols) >= 3 * patch * patch, what ": %d columns below the %d of a patch", (cols), 3 * patch * patch);                                    \
        REQUIRE(std[0] > 0.f && std[1] > 0.f && std[2] > 0.f, what ": std must be positive");                                                            \
    } while (0)

extern "C" int ffn_sam_patch_rows(void* stream, int dtype, const uint8_t* src, void* out, int B, int H, int W, int side, int patch, int ldo, const float* mean,
                                  const float* std) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "sam_patch_rows: bad dtype %d", dtype);
    SAM_PATCH_ROWS("sam_patch_rows", ldo);
    fsam_patch_rows(reinterpret_cast<hipStream_t>(stream), dtype, src, out, B, H, W, side, patch, ldo, mean, std);
    return check_launch("sam_patch_rows");
}

extern "C" int ffn_sam_patch_rows_pair(void* stream, const uint8_t* src, void* out, int B, int H, int W, int side, int patch, int K, const float* mean, const float* std) {
    SAM_PATCH_ROWS("sam_patch_rows_pair", K);
    REQUIRE(K % 8 == 0, "sam_patch_rows_pair: K=%d is not a multiple of 8 (16-byte stores of both halves)", K);
    REQUIRE(aligned16(out), "sam_patch_rows_pair: out must be 16-byte aligned");
    fsam_patch_rows_pair(reinterpret_cast<hipStream_t>(stream), src, out, B, H, W, side, patch, K, mean, std);
    return check_launch("sam_patch_rows_pair");
}

extern "C" int ffn_hyper_masks(void* stream, const float* up, const float* hyper, float* out, int N, int hw, int C, int M) {
    REQUIRE(up && hyper && out, "hyper_masks: null pointer");
    REQUIRE(aligned16(up), "hyper_masks: up must be 16-byte aligned");
    REQUIRE(N >= 1 && N <= 65535, "hyper_masks: N=%d outside 1 .. 65535", N);
    REQUIRE(hw >= 1 && hw <= FFN_IMGPREP_MAX_SIDE * FFN_IMGPREP_MAX_SIDE, "hyper_masks: hw=%d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE squared)", hw,
            FFN_IMGPREP_MAX_SIDE * FFN_IMGPREP_MAX_SIDE);
    REQUIRE(C >= 4 && C <= 64 && C % 4 == 0, "hyper_masks: C=%d channels (a multiple of 4, at most 64)", C);
    REQUIRE(M >= 1 && M <= 8, "hyper_masks: M=%d masks outside 1 .. 8", M);
    fsam_hyper_masks(reinterpret_cast<hipStream_t>(stream), up, hyper, out, N, hw, C, M);
    return check_launch("hyper_masks");
}

extern "C" int ffn_upsample_bicubic(void* stream, const float* src, float* dst, uint8_t* mask, int N, int h, int w, int H, int W) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && dst, "upsample_bicubic: null pointer");
    REQUIRE(N >= 1 && N <= 65535, "upsample_bicubic: N=%d outside 1 .. 65535", N);
    REQUIRE(h >= 1 && w >= 1 && h <= lim && w <= lim, "upsample_bicubic: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", h, w, lim);
    REQUIRE(H >= 1 && W >= 1 && H <= lim && W <= lim, "upsample_bicubic: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", H, W, lim);
    fsam_bicubic(reinterpret_cast<hipStream_t>(stream), src, dst, mask, N, h, w, H, W);
    return check_launch("upsample_bicubic");
}

// ---- automatic mask generation: the statistics of the upsampled candidates, box NMS (kernels: sam.h, launches: imgprep.hip) ------------------------
extern "C" __attribute__((visibility("hidden"))) void fsam_bicubic_stats(hipStream_t s, const float* src, int* stats, uint8_t* mask, int N, int h, int w, int H, int W,
                                                                         float offset);
extern "C" __attribute__((visibility("hidden"))) void fsam_box_nms(hipStream_t s, const float* boxes, unsigned long long* suppress, int M, float thresh);

extern "C" int ffn_upsample_bicubic_stats(void* stream, const float* src, int32_t* stats, uint8_t* mask, int N, int h, int w, int H, int W, float offset) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && stats, "upsample_bicubic_stats: null pointer");
    REQUIRE(N >= 1 && N <= 65535, "upsample_bicubic_stats: N=%d outside 1 .. 65535", N);
    REQUIRE(h >= 1 && w >= 1 && h <= lim && w <= lim, "upsample_bicubic_stats: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", h, w, lim);
    REQUIRE(H >= 1 && W >= 1 && H <= lim && W <= lim, "upsample_bicubic_stats: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", H, W, lim);
    REQUIRE(__builtin_isfinite(offset) && offset >= 0.f, "upsample_bicubic_stats: offset=%g must be finite and >= 0", (double)offset);
    fsam_bicubic_stats(reinterpret_cast<hipStream_t>(stream), src, stats, mask, N, h, w, H, W, offset);
    return check_launch("upsample_bicubic_stats");
}

extern "C" int ffn_box_nms(void* stream, const float* boxes, uint64_t* suppress, int M, float thresh) {
    REQUIRE(boxes && suppress, "box_nms: null pointer");
    REQUIRE(M >= 1 && M <= FFN_BOX_NMS_MAX, "box_nms: M=%d outside 1 .. %d (FFN_BOX_NMS_MAX)", M, FFN_BOX_NMS_MAX);
    REQUIRE(__builtin_isfinite(thresh), "box_nms: thresh=%g is not finite", (double)thresh);
    fsam_box_nms(reinterpret_cast<hipStream_t>(stream), boxes, reinterpret_cast<unsigned long long*>(suppress), M, thresh);
    return check_launch("box_nms");
}

// ---- elementwise / resampling helpers of the depth front end ----------------------------------------------------------
extern "C" int ffn_eltwise(void* stream, int dtype, int op, const void* a, const void* b, void* y, long n) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "eltwise: bad dtype %d", dtype);
    REQUIRE(op == FFN_ELT_RELU || op == FFN_ELT_ADD || op == FFN_ELT_GELU, "eltwise: bad op %d", op);
    REQUIRE(a && y && (op != FFN_ELT_ADD || b), "eltwise: null operand");
    REQUIRE(n > 0 && n % 4 == 0, "eltwise: n=%ld must be a positive multiple of 4", n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n4 = n / 4;
    const int grid = grid_for(n4);
    if (dtype == FFN_F32) {
        if (op == FFN_ELT_RELU) LAUNCH((eltwise_kernel<float, FFN_ELT_RELU>), dim3(grid), dim3(256), 0, s, (const float*)a, (const float*)b, (float*)y, n4);
        else if (op == FFN_ELT_GELU) LAUNCH((eltwise_kernel<float, FFN_ELT_GELU>), dim3(grid), dim3(256), 0, s, (const float*)a, (const float*)b, (float*)y, n4);
        else LAUNCH((eltwise_kernel<float, FFN_ELT_ADD>), dim3(grid), dim3(256), 0, s, (const float*)a, (const float*)b, (float*)y, n4);
    } else {
        if (op == FFN_ELT_RELU) LAUNCH((eltwise_kernel<bf16, FFN_ELT_RELU>), dim3(grid), dim3(256), 0, s, (const bf16*)a, (const bf16*)b, (bf16*)y, n4);
        else if (op == FFN_ELT_GELU) LAUNCH((eltwise_kernel<bf16, FFN_ELT_GELU>), dim3(grid), dim3(256), 0, s, (const bf16*)a, (const bf16*)b, (bf16*)y, n4);
        else LAUNCH((eltwise_kernel<bf16, FFN_ELT_ADD>), dim3(grid), dim3(256), 0, s, (const bf16*)a, (const bf16*)b, (bf16*)y, n4);
    }
    return check_launch("eltwise");
}
extern "C" int ffn_resize_bilinear(void* stream, int dtype, const void* x, void* y, int B, int Hin, int Win, int Hout, int Wout, int C, int relu) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "resize_bilinear: bad dtype %d", dtype);
    REQUIRE(x && y, "resize_bilinear: null operand");
    REQUIRE(B > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && C > 0 && C % 4 == 0, "resize_bilinear: bad shape (C=%d must be a multiple of 4)", C);
    REQUIRE((long)B * Hout * Wout * C < (1l << 40) && (long)Hin * Win < (1l << 31), "resize_bilinear: problem too large");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n4 = (long)B * Hout * Wout * (C / 4);
    const int grid = grid_for(n4);
    if (dtype == FFN_F32) {
        if (relu) LAUNCH((resize_bilinear_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, n4, Hin, Win, Hout, Wout, C);
        else LAUNCH((resize_bilinear_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, n4, Hin, Win, Hout, Wout, C);
    } else {
        if (relu) LAUNCH((resize_bilinear_kernel<bf16, true>), dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, n4, Hin, Win, Hout, Wout, C);
        else LAUNCH((resize_bilinear_kernel<bf16, false>), dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, n4, Hin, Win, Hout, Wout, C);
    }
    return check_launch("resize_bilinear");
}

// ---- norms -------------------------------------------------------------------------------------------------------
extern "C" int ffn_gn_nchunk(int HW) {
    int n = HW / 128;
    if (n < 1) n = 1;
    if (n > 256) n = 256;
    return n;
}
// one fused launch (statistics + normalise + SiLU by the workgroup that owns a (row, group) slice) or stats + finalize + apply?
// Measured (tools/bench_kernels.py --only norm): the fused kernel reads 20-120 byte per-pixel group segments, so it only wins while
// the tensor is small enough for launch latency to dominate -- up to 8x8 positions at any batch, 16x16 up to 32 rows (at 48 rows,
// the image-batched guided pass, the three-launch form is 7-18 % faster there: 34.9 vs 37.5 us at C = 1280, 56.6 vs 66.1 at 2560),
// 32x32 below ~3M elements.
extern "C" int ffn_gn_fused(int B, int HW, int C, int G) {
    const long slice = (long)HW * (C / (G > 0 ? G : 1));
    if (slice > 131072) return 0;
    if (HW <= 64) return 1;
    if (HW <= 256) return B <= 32 ? 1 : 0;
    return (HW <= 1024 && (long)B * HW * C <= 3000000l) ? 1 : 0;
}
extern "C" int ffn_groupnorm(void* stream, int dtype, const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C,
                             int G, float eps, int silu, float* partial_ws, float* scale, float* shift) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "groupnorm: bad dtype");
    REQUIRE(x && y && gamma && beta && C % G == 0 && (C / G) % 2 == 0, "groupnorm: bad arguments (C=%d, G=%d)", C, G);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long slice = (long)HW * (C / G);
    (void)slice;
    const bool fused = ffn_gn_fused(B, HW, C, G) != 0;
    const bool pair = silu & FFN_NORM_OUT_PAIR;
    REQUIRE(!pair || (dtype == FFN_F32 && C % 4 == 0), "groupnorm: pair output needs fp32 input and C %% 4 == 0");
    silu &= FFN_NORM_SILU;
    if (fused && pair) {
        dim3 grid(G, B);
        if (silu) LAUNCH((gn_fused_kernel<float, true, true>), grid, dim3(1024), 0, s, (const float*)x, (float*)y, gamma, beta, HW, C, G, eps);
        else LAUNCH((gn_fused_kernel<float, false, true>), grid, dim3(1024), 0, s, (const float*)x, (float*)y, gamma, beta, HW, C, G, eps);
        return check_launch("gn_fused(pair)");
    }
    if (fused) {   // one workgroup owns a whole (batch, group) slice: statistics + normalise + SiLU in ONE launch
                                           // (measured: wins up to 32x32 latents; at 64x64 the 20-60 byte per-pixel group segments coalesce badly)
        dim3 grid(G, B);
        if (dtype == FFN_F32) {
            if (silu) LAUNCH((gn_fused_kernel<float, true>), grid, dim3(1024), 0, s, (const float*)x, (float*)y, gamma, beta, HW, C, G, eps);
            else LAUNCH((gn_fused_kernel<float, false>), grid, dim3(1024), 0, s, (const float*)x, (float*)y, gamma, beta, HW, C, G, eps);
        } else {
            if (silu) LAUNCH((gn_fused_kernel<bf16, true>), grid, dim3(1024), 0, s, (const bf16*)x, (bf16*)y, gamma, beta, HW, C, G, eps);
            else LAUNCH((gn_fused_kernel<bf16, false>), grid, dim3(1024), 0, s, (const bf16*)x, (bf16*)y, gamma, beta, HW, C, G, eps);
        }
        return check_launch("gn_fused");
    }
    REQUIRE(partial_ws && scale && shift, "groupnorm: workspace required beyond 32x32 positions");
    int rc = ffn_gn_stats(stream, dtype, x, gamma, beta, B, HW, C, G, eps, partial_ws, scale, shift);
    if (rc) return rc;
    return ffn_gn_apply(stream, dtype, x, y, scale, shift, B, HW, C, silu | (pair ? FFN_NORM_OUT_PAIR : 0));
}
extern "C" int ffn_groupnorm_pair_raw(void* stream, const void* x, void* y, void* yraw, const float* gamma, const float* beta, int B, int HW, int C, int G,
                                      float eps, int silu, float* partial_ws, float* scale, float* shift) {
    REQUIRE(x && y && yraw && gamma && beta && partial_ws && scale && shift, "groupnorm_pair_raw: null pointer (the workspace is always needed)");
    REQUIRE(C % 8 == 0 && C % G == 0 && (C / G) % 2 == 0 && aligned16(x) && aligned16(y) && aligned16(yraw), "groupnorm_pair_raw: bad arguments (C=%d, G=%d)", C, G);
    REQUIRE(y != yraw && yraw != x && y != x, "groupnorm_pair_raw: x, y and yraw must be distinct buffers");
    int rc = ffn_gn_stats(stream, FFN_F32, x, gamma, beta, B, HW, C, G, eps, partial_ws, scale, shift);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n8 = (long)B * HW * (C / 8);
    if (silu & FFN_NORM_SILU) LAUNCH((gn_apply_pair8_kernel<true, true>), dim3(grid_for(n8)), dim3(256), 0, s, (const float*)x, (bf16*)y, scale, shift, n8, HW, C, (bf16*)yraw);
    else LAUNCH((gn_apply_pair8_kernel<false, true>), dim3(grid_for(n8)), dim3(256), 0, s, (const float*)x, (bf16*)y, scale, shift, n8, HW, C, (bf16*)yraw);
    return check_launch("gn_apply(pair + raw pair)");
}
extern "C" int ffn_groupnorm_f8(void* stream, const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int Cp, int G,
                                float eps, int silu, float qscale, float* partial_ws, float* scale, float* shift) {
    REQUIRE(x && y && gamma && beta && partial_ws && scale && shift, "groupnorm_f8: null pointer (the workspace is always needed)");
    REQUIRE(C % 16 == 0 && C % G == 0 && Cp >= C && Cp % 16 == 0 && aligned16(x) && aligned16(y) && qscale > 0.f, "groupnorm_f8: bad arguments (C=%d, Cp=%d)", C, Cp);
    int rc = ffn_gn_stats(stream, FFN_BF16, x, gamma, beta, B, HW, C, G, eps, partial_ws, scale, shift);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long nch = (long)B * HW * (Cp / 16);
    if (silu & FFN_NORM_SILU) LAUNCH(gn_apply_f8_kernel<true>, dim3(grid_for(nch)), dim3(256), 0, s, (const bf16*)x, (uint8_t*)y, scale, shift, nch, HW, C, Cp, qscale);
    else LAUNCH(gn_apply_f8_kernel<false>, dim3(grid_for(nch)), dim3(256), 0, s, (const bf16*)x, (uint8_t*)y, scale, shift, nch, HW, C, Cp, qscale);
    return check_launch("gn_apply_f8");
}
extern "C" int ffn_gn_stats(void* stream, int dtype, const void* x, const float* gamma, const float* beta, int B, int HW, int C,
                            int G, float eps, float* partial_ws, float* scale, float* shift) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "gn_stats: bad dtype");
    const int epc = dtype == FFN_F32 ? 4 : 8;
    REQUIRE(x && gamma && beta && partial_ws && scale && shift, "gn_stats: null pointer");
    REQUIRE(C % epc == 0 && C % G == 0 && aligned16(x), "gn_stats: C=%d must be a multiple of %d and of G=%d", C, epc, G);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nchunk = ffn_gn_nchunk(HW);
    const int ppc = (HW + nchunk - 1) / nchunk;
    const int epc_ = dtype == FFN_F32 ? 4 : 8;
    const int cols_ = C / epc_ < 256 ? C / epc_ : 256;
    const int lds = (256 / cols_ > 0 ? 256 / cols_ : 1) * cols_ * 2 * epc_ * (int)sizeof(float);      // [pixel rows of threads][columns][2 x EPC]
    if (dtype == FFN_F32)
        LAUNCH(gn_partial_kernel<float>, dim3(nchunk, B), dim3(256), lds, s, (const float*)x, partial_ws, HW, C, ppc);
    else
        LAUNCH(gn_partial_kernel<bf16>, dim3(nchunk, B), dim3(256), lds, s, (const bf16*)x, partial_ws, HW, C, ppc);
    if (int rc = check_launch("gn_partial")) return rc;      // the next LAUNCH clears the error state: check before it
    LAUNCH(gn_finalize_kernel, dim3(G, B), dim3(64), 0, s, partial_ws, gamma, beta, scale, shift, HW, C, G, nchunk, ppc, eps);
    return check_launch("gn_stats");
}
extern "C" int ffn_gn_apply(void* stream, int dtype, const void* x, void* y, const float* scale, const float* shift, int B, int HW,
                            int C, int silu) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "gn_apply: bad dtype");
    const int epc = dtype == FFN_F32 ? 4 : 8;
    REQUIRE(x && y && scale && shift && C % epc == 0 && aligned16(x) && aligned16(y), "gn_apply: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long nch = (long)B * HW * (C / epc);
    const int grid = grid_for(nch);
    if (silu & FFN_NORM_OUT_PAIR) {
        REQUIRE(dtype == FFN_F32, "gn_apply: pair output needs fp32 input");
        static const int wide = [] { const char* e = getenv("FFN_PAIR8"); return e ? atoi(e) : 1; }();      // 0: the round-5 kernels (8-byte stores, libm SiLU)
        if (wide && C % 8 == 0) {
            const long n8 = (long)B * HW * (C / 8);
            if (silu & FFN_NORM_SILU) LAUNCH(gn_apply_pair8_kernel<true>, dim3(grid_for(n8)), dim3(256), 0, s, (const float*)x, (bf16*)y, scale, shift, n8, HW, C);
            else LAUNCH(gn_apply_pair8_kernel<false>, dim3(grid_for(n8)), dim3(256), 0, s, (const float*)x, (bf16*)y, scale, shift, n8, HW, C);
            return check_launch("gn_apply(pair, 8 wide)");
        }
        if (silu & FFN_NORM_SILU) LAUNCH((gn_apply_kernel<float, true, true>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, scale, shift, nch, HW, C);
        else LAUNCH((gn_apply_kernel<float, false, true>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, scale, shift, nch, HW, C);
        return check_launch("gn_apply(pair)");
    }
    if (dtype == FFN_F32) {
        if (silu) LAUNCH((gn_apply_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, scale, shift, nch, HW, C);
        else LAUNCH((gn_apply_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, scale, shift, nch, HW, C);
    } else {
        if (silu) LAUNCH((gn_apply_kernel<bf16, true>), dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, scale, shift, nch, HW, C);
        else LAUNCH((gn_apply_kernel<bf16, false>), dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, scale, shift, nch, HW, C);
    }
    return check_launch("gn_apply");
}
extern "C" int ffn_layernorm(void* stream, int dtype, const void* x, void* y, const float* gamma, const float* beta, int M, int C,
                             float eps) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "layernorm: bad dtype");
    const int epc = dtype == FFN_F32 ? 4 : 8;
    REQUIRE(x && y && gamma && beta && C % epc == 0 && aligned16(x) && aligned16(y), "layernorm: bad arguments");
    const int cch = C / epc;
    REQUIRE(cch <= 64 * 6, "layernorm: C=%d too large", C);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = (M + 3) / 4;
    if (dtype == FFN_F32) {
        if (cch <= 128) LAUNCH((layernorm_kernel<float, 2>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, gamma, beta, M, C, eps);
        else LAUNCH((layernorm_kernel<float, 6>), dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, gamma, beta, M, C, eps);
    } else {
        if (cch <= 128) LAUNCH((layernorm_kernel<bf16, 2>), dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, gamma, beta, M, C, eps);
        else LAUNCH((layernorm_kernel<bf16, 6>), dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, gamma, beta, M, C, eps);
    }
    return check_launch("layernorm");
}
extern "C" int ffn_layernorm_pair(void* stream, const float* x, void* y, const float* gamma, const float* beta, int M, int C, float eps) {
    REQUIRE(x && y && gamma && beta && C % 4 == 0 && aligned16(x) && aligned16(y), "layernorm_pair: bad arguments");
    const int cch = C / 4;
    REQUIRE(cch <= 64 * 6, "layernorm_pair: C=%d too large", C);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = (M + 3) / 4;
    if (cch <= 128) LAUNCH((layernorm_kernel<float, 2, true>), dim3(grid), dim3(256), 0, s, x, (float*)y, gamma, beta, M, C, eps);
    else LAUNCH((layernorm_kernel<float, 6, true>), dim3(grid), dim3(256), 0, s, x, (float*)y, gamma, beta, M, C, eps);
    return check_launch("layernorm(pair)");
}
extern "C" int ffn_softmax_rows(void* stream, int dtype, const void* x, void* y, long M, int N, float scale) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "softmax_rows: bad dtype");
    REQUIRE(x && y && M > 0 && N > 0, "softmax_rows: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == FFN_F32) LAUNCH(softmax_rows_kernel<float>, dim3((unsigned)M), dim3(256), 0, s, (const float*)x, (float*)y, N, scale);
    else LAUNCH(softmax_rows_kernel<bf16>, dim3((unsigned)M), dim3(256), 0, s, (const bf16*)x, (bf16*)y, N, scale);
    return check_launch("softmax_rows");
}

// ---- scheduler / guidance ---------------------------------------------------------------------------------------
extern "C" int ffn_cfg_masked(void* stream, const float* eps_u, const float* eps_c, const float* mask, float cfg, float* eps, long n,
                              int HW) {
    REQUIRE(eps_u && eps_c && eps && n > 0 && HW > 0, "cfg_masked: bad arguments");
    LAUNCH(cfg_masked_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), eps_u, eps_c, mask, cfg, eps, n, HW);
    return check_launch("cfg_masked");
}
extern "C" int ffn_ddim_inv_step(void* stream, const float* eps, const float* x, float c_bt, float c_at, float c_an, float c_bn,
                                 float* x_next, float* pred_x0, long n) {
    REQUIRE(eps && x && x_next && n > 0, "ddim_inv_step: bad arguments");
    LAUNCH(ddim_inv_step_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), eps, x, c_bt, c_at, c_an, c_bn, x_next, pred_x0, n);
    return check_launch("ddim_inv_step");
}
extern "C" int ffn_ddim_ctrl_step(void* stream, const ffn_ctrl_step_desc* d) {
    REQUIRE(d && d->eps && d->x && d->x_prev && d->m && d->om, "ddim_ctrl_step: null pointer");
    REQUIRE(d->rows > 0 && d->rows <= 8 && d->CHW > 0 && d->HW > 0 && d->CHW % d->HW == 0, "ddim_ctrl_step: bad shape");
    LAUNCH(ddim_ctrl_step_kernel, dim3(grid_for((long)d->rows * d->CHW)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *d);
    return check_launch("ddim_ctrl_step");
}

// ---- layout / misc -----------------------------------------------------------------------------------------------
extern "C" int ffn_pack_nchw(void* stream, int dtype, const ffn_pack_desc* d) {
    REQUIRE(d && d->src && d->dst && d->B > 0 && d->B <= 16 && d->CP >= d->Cl, "pack_nchw: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n = (long)d->B * d->HW * d->CP;
    if (dtype == FFN_F32) LAUNCH(pack_nchw_kernel<float>, dim3(grid_for(n)), dim3(256), 0, s, *d);
    else if (dtype == FFN_BF16) LAUNCH(pack_nchw_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, s, *d);
    else return fail(FFN_EINVAL, "pack_nchw: bad dtype");
    return check_launch("pack_nchw");
}
extern "C" int ffn_nhwc_to_nchw_f32(void* stream, const float* src, float* dst, int B, int HW, int C, int ld) {
    REQUIRE(src && dst && B > 0 && HW > 0 && C > 0 && ld >= C, "nhwc_to_nchw_f32: bad arguments");
    LAUNCH(nhwc_to_nchw_f32_kernel, dim3(grid_for((long)B * HW * C)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, dst, B, HW, C, ld);
    return check_launch("nhwc_to_nchw_f32");
}
extern "C" int ffn_concat(void* stream, int dtype, const void* a, const void* b, void* out, long rows, int C1, int C2) {
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "concat: bad dtype");
    const int epc = dtype == FFN_F32 ? 4 : 8;
    REQUIRE(b && out && C1 % epc == 0 && C2 % epc == 0 && aligned16(a) && aligned16(b) && aligned16(out), "concat: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n = rows * ((a ? C1 + C2 : C2) / epc);     // a == NULL: out[:, :C1] is already in place, only b moves
    if (dtype == FFN_F32) LAUNCH(concat_kernel<float>, dim3(grid_for(n)), dim3(256), 0, s, (const float*)a, (const float*)b, (float*)out, rows, C1, C2);
    else LAUNCH(concat_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, s, (const bf16*)a, (const bf16*)b, (bf16*)out, rows, C1, C2);
    return check_launch("concat");
}
extern "C" int ffn_timestep_embed(void* stream, int dtype, const float* t_dev, const float* freq, void* out, int B, int half, int flip) {
    REQUIRE(t_dev && freq && out && B > 0 && half > 0, "timestep_embed: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n = B * 2 * half;
    if (dtype == FFN_F32) LAUNCH(timestep_embed_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, s, t_dev, freq, (float*)out, B, half, flip);
    else if (dtype == FFN_BF16) LAUNCH(timestep_embed_kernel<bf16>, dim3((n + 255) / 256), dim3(256), 0, s, t_dev, freq, (bf16*)out, B, half, flip);
    else return fail(FFN_EINVAL, "timestep_embed: bad dtype");
    return check_launch("timestep_embed");
}
extern "C" int ffn_transpose(void* stream, int dtype, const void* src, void* dst, int B, int R, int C, int ld_src, int ld_dst) {
    REQUIRE(src && dst && B > 0 && R > 0 && C > 0, "transpose: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((C + 31) / 32, (R + 31) / 32, B);
    if (dtype == FFN_F32) LAUNCH(transpose_kernel<float>, grid, dim3(256), 0, s, (const float*)src, (float*)dst, R, C, ld_src, ld_dst);
    else if (dtype == FFN_BF16) LAUNCH(transpose_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)src, (bf16*)dst, R, C, ld_src, ld_dst);
    else return fail(FFN_EINVAL, "transpose: bad dtype");
    return check_launch("transpose");
}
extern "C" int ffn_cast(void* stream, int src_dtype, int dst_dtype, const void* src, void* dst, long n) {
    REQUIRE(src && dst && n > 0, "cast: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = grid_for(n);
    if (src_dtype == FFN_F32 && dst_dtype == FFN_BF16) LAUNCH((cast_kernel<float, bf16>), dim3(grid), dim3(256), 0, s, (const float*)src, (bf16*)dst, n);
    else if (src_dtype == FFN_BF16 && dst_dtype == FFN_F32) LAUNCH((cast_kernel<bf16, float>), dim3(grid), dim3(256), 0, s, (const bf16*)src, (float*)dst, n);
    else if (src_dtype == FFN_F32 && dst_dtype == FFN_F32) LAUNCH((cast_kernel<float, float>), dim3(grid), dim3(256), 0, s, (const float*)src, (float*)dst, n);
    else if (src_dtype == FFN_BF16 && dst_dtype == FFN_BF16) LAUNCH((cast_kernel<bf16, bf16>), dim3(grid), dim3(256), 0, s, (const bf16*)src, (bf16*)dst, n);
    else return fail(FFN_EINVAL, "cast: bad dtypes %d -> %d", src_dtype, dst_dtype);
    return check_launch("cast");
}
extern "C" int ffn_image_to_nhwc(void* stream, int dtype, const uint8_t* img, void* dst, long npix, int CP) {
    REQUIRE(img && dst && npix > 0 && CP >= 3, "image_to_nhwc: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = grid_for(npix * CP);
    if (dtype == FFN_F32) LAUNCH(image_to_nhwc_kernel<float>, dim3(grid), dim3(256), 0, s, img, (float*)dst, npix, CP);
    else if (dtype == FFN_BF16) LAUNCH(image_to_nhwc_kernel<bf16>, dim3(grid), dim3(256), 0, s, img, (bf16*)dst, npix, CP);
    else return fail(FFN_EINVAL, "image_to_nhwc: bad dtype");
    return check_launch("image_to_nhwc");
}
extern "C" int ffn_nhwc_to_image(void* stream, int dtype, const void* src, float* dst, int B, int HW, int ld) {
    REQUIRE(src && dst && B > 0 && HW > 0 && ld >= 3, "nhwc_to_image: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = grid_for((long)B * 3 * HW);
    if (dtype == FFN_F32) LAUNCH(nhwc_to_image_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, dst, B, HW, ld);
    else if (dtype == FFN_BF16) LAUNCH(nhwc_to_image_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)src, dst, B, HW, ld);
    else return fail(FFN_EINVAL, "nhwc_to_image: bad dtype");
    return check_launch("nhwc_to_image");
}

// ---- point-cloud warp of the 3-D front end (splat.h) ----------------------------------------------------------------
extern "C" int ffn_splat_lift(void* stream, const float* depth, const int* idx, float* pts, int n, int W, int H, float fx, float fy) {
    REQUIRE(depth && idx && pts, "splat_lift: null operand");
    REQUIRE(n > 0 && W > 0 && H > 0 && (long)W * H < (1l << 31) && fx != 0.f && fy != 0.f, "splat_lift: bad shape / focal length");
    LAUNCH(splat_lift_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth, idx, pts, n, W, H, fx, fy);
    return check_launch("splat_lift");
}
extern "C" int ffn_splat_project(void* stream, const float* pts, float* proj, int n, const ffn_splat_xform* x) {
    REQUIRE(pts && proj && x, "splat_project: null operand");
    REQUIRE(n > 0, "splat_project: empty cloud");
    SplatXform X;
    for (int i = 0; i < 3; ++i) { X.c[i] = x->center[i]; X.t[i] = x->translate[i]; X.s[i] = x->scale[i]; }
    for (int i = 0; i < 9; ++i) X.R[i] = x->rotate[i];
    REQUIRE(x->tan_half_fov > 0.f, "splat_project: tan_half_fov must be positive");
    X.inv_tan = 1.f / x->tan_half_fov;
    LAUNCH(splat_project_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pts, proj, n, X);
    return check_launch("splat_project");
}
extern "C" int ffn_splat_bin(void* stream, int fill, const float* proj, int n, float radius, int W, int H, int* counts, const int* offs, int* list) {
    REQUIRE(proj && counts, "splat_bin: null operand");
    REQUIRE(!fill || (offs && list), "splat_bin: the filling pass needs the tile offsets and the list");
    REQUIRE(n > 0 && W > 0 && H > 0 && radius > 0.f, "splat_bin: bad shape / radius");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (fill) LAUNCH(splat_bin_kernel<true>, dim3(grid_for(n)), dim3(256), 0, s, proj, n, radius, W, H, counts, offs, list);
    else LAUNCH(splat_bin_kernel<false>, dim3(grid_for(n)), dim3(256), 0, s, proj, n, radius, W, H, counts, offs, list);
    return check_launch("splat_bin");
}
extern "C" int ffn_splat_render(void* stream, const float* proj, const float* rgb, const int* offs, const int* list, float radius, int K, int W, int H,
                                float* image, int* idx_sum, uint8_t* covered) {
    REQUIRE(proj && rgb && offs && list && image && idx_sum && covered, "splat_render: null operand");
    REQUIRE(K >= 1 && K <= 32, "splat_render: points per pixel K=%d out of range (1 .. 32)", K);
    REQUIRE(W > 0 && H > 0 && radius > 0.f, "splat_render: bad shape / radius");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    if (K <= 8) LAUNCH(splat_render_kernel<8>, dim3(tiles), dim3(256), 0, s, proj, rgb, offs, list, radius, K, W, H, image, idx_sum, covered);
    else if (K <= 16) LAUNCH(splat_render_kernel<16>, dim3(tiles), dim3(256), 0, s, proj, rgb, offs, list, radius, K, W, H, image, idx_sum, covered);
    else LAUNCH(splat_render_kernel<32>, dim3(tiles), dim3(256), 0, s, proj, rgb, offs, list, radius, K, W, H, image, idx_sum, covered);
    return check_launch("splat_render");
}
extern "C" int ffn_splat_ids(void* stream, const float* proj, const int* offs, const int* list, float radius, int K, int W, int H, int* ids) {
    REQUIRE(proj && offs && list && ids, "splat_ids: null operand");
    REQUIRE(K >= 1 && K <= 32, "splat_ids: points per pixel K=%d out of range (1 .. 32)", K);
    REQUIRE(W > 0 && H > 0 && radius > 0.f, "splat_ids: bad shape / radius");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    if (K <= 8) LAUNCH(splat_ids_kernel<8>, dim3(tiles), dim3(256), 0, s, proj, offs, list, radius, K, W, H, ids);
    else if (K <= 16) LAUNCH(splat_ids_kernel<16>, dim3(tiles), dim3(256), 0, s, proj, offs, list, radius, K, W, H, ids);
    else LAUNCH(splat_ids_kernel<32>, dim3(tiles), dim3(256), 0, s, proj, offs, list, radius, K, W, H, ids);
    return check_launch("splat_ids");
}
extern "C" int ffn_splat_correspond(void* stream, const float* proj, const int* idx, int n, int W, int H, const int* ids, int K, float* map,
                                    uint8_t* visible) {
    REQUIRE(proj && idx && map, "splat_correspond: null operand");
    REQUIRE(!visible || ids, "splat_correspond: the visibility output needs the ids of ffn_splat_ids");
    REQUIRE(n >= 0 && W > 0 && H > 0 && (long)W * H < (1l << 31), "splat_correspond: bad shape");
    REQUIRE(K >= 1 && K <= 32, "splat_correspond: points per pixel K=%d out of range (1 .. 32)", K);
    if (n == 0) return FFN_OK;
    LAUNCH(splat_correspond_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), proj, idx, n, W, H, ids, K, map, visible);
    return check_launch("splat_correspond");
}

// ---- the GeoDiffuser warp of the reference's GeoBench-3D step 2 (geowarp.h) ---------------------------------------------
// included here, after everything else, so that the kernels of the units above keep their place in the code object
#include "geowarp.h"
extern "C" int ffn_geo_project(void* stream, const float* depth, const float* pose, float focal, int H, int W, float* tcoords, float* proj) {
    REQUIRE(depth && pose && tcoords && proj, "geo_project: null operand");
    REQUIRE(H == W, "geo_project: the image must be square (%d x %d): the reference takes sqrt(N) for the side", H, W);
    REQUIRE(H >= 2 && H <= 4096 && focal > 0.f, "geo_project: side %d outside 2 .. 4096, or focal length <= 0", H);
    GeoPose P;
    for (int a = 0; a < 12; ++a) P.m[a] = pose[a];
    LAUNCH(geo_project_kernel, dim3(grid_for((long)H * W)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth, P, focal, H, tcoords, proj);
    return check_launch("geo_project");
}
extern "C" int ffn_splat_composite(void* stream, const float* proj, const float* feat, const int* offs, const int* list, float radius, float tau, int K,
                                   int C, int H, int W, int round_half, float* out) {
    REQUIRE(proj && feat && offs && list && out, "splat_composite: null operand");
    REQUIRE(H == W, "splat_composite: the image must be square (%d x %d)", H, W);
    REQUIRE(H >= 1 && H <= 4096, "splat_composite: side %d outside 1 .. 4096", H);
    REQUIRE(K >= 1 && K <= 32, "splat_composite: points per pixel K=%d out of range (1 .. 32)", K);
    REQUIRE(C >= 1 && C <= 8, "splat_composite: C=%d feature channels out of range (1 .. 8)", C);
    REQUIRE(radius > 0.f && tau > 0.f, "splat_composite: radius and tau must be positive");
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (K <= 8) LAUNCH(geo_composite_kernel<8>, dim3(tiles), dim3(256), 0, s, proj, feat, offs, list, radius, tau, K, C, W, H, round_half, out);
    else if (K <= 16) LAUNCH(geo_composite_kernel<16>, dim3(tiles), dim3(256), 0, s, proj, feat, offs, list, radius, tau, K, C, W, H, round_half, out);
    else LAUNCH(geo_composite_kernel<32>, dim3(tiles), dim3(256), 0, s, proj, feat, offs, list, radius, tau, K, C, W, H, round_half, out);
    return check_launch("splat_composite");
}
extern "C" int ffn_mesh_cover(void* stream, const float* tcoords, const uint8_t* mask, int H, int W, uint8_t* cover) {
    REQUIRE(tcoords && mask && cover, "mesh_cover: null operand");
    REQUIRE(H == W, "mesh_cover: the image must be square (%d x %d)", H, W);
    REQUIRE(H >= 2 && H <= 4096, "mesh_cover: side %d outside 2 .. 4096", H);
    LAUNCH(geo_mesh_cover_kernel, dim3(grid_for(2l * (H - 1) * (W - 1))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tcoords, mask, H, cover);
    return check_launch("mesh_cover");
}
