// C ABI of libfreefine_hip.so (see include/freefine_hip.h), the general unit: version, error state, device info, graph launch, norms, elementwise /
// scheduler / layout kernels and the two small convolution-side entries.  Host-side launch glue only: argument validation, dynamic-LDS opt-in.  No
// allocation, no synchronisation, everything on the caller's stream.  Every other unit exports the entries of its own kernels the same way
// (capi_igemm.hip, capi_attn.hip, capi_splat.hip, attn_causal.hip, dift.hip, imgprep.hip, inception.hip); capi_common.h holds what they share.
#include <stdlib.h>
#include <string.h>

#include "capi_common.h"
#include "conv_small.h"
#include "elementwise.h"
#include "norms.h"

__thread char g_err[512] = "";

extern "C" int ffn_version(void) { return 16; }      // 16: the Inception-v3 extractor of FID (ffn_conv2d, ffn_pool2d, ffn_mean_hw, ffn_fid_prep); 15: the ImageReward score's BERT (ffn_embed_tokens_ln, ffn_affine_chain); 14: automatic mask generation (ffn_upsample_bicubic_stats, ffn_box_nms); 13: the GeoDiffuser warp of GeoBench-3D (ffn_geo_project, ffn_splat_composite, ffn_mesh_cover); 12: SIFT keypoints for Mean Distance (ffn_sift_base, ffn_gauss_blur_f32, ffn_decimate2_f32, ffn_sift_extrema, ffn_sift_refine_orient, ffn_sift_describe, ffn_knn2_u8; FFN_ENOSPC); 11: click-to-mask (ffn_sam_patch_rows, ffn_sam_patch_rows_pair, ffn_hyper_masks, ffn_upsample_bicubic, FFN_ELT_GELU); 10: the correspondence map of the point-cloud warp (ffn_splat_ids, ffn_splat_correspond); 9: the case preparation of the GeoBench harness (ffn_resize_taps8_u8, ffn_resize_gather_u8, ffn_dilate_u8, ffn_mask_bbox_u8, ffn_coarse_edit_2d); 8: ffn_pool_layernorm, ffn_cosine_rows; 2: FFN_ATT_CAUSAL, FFN_IG_OUT_QGELU, ffn_embed_tokens; 3: the igemm tile query is gone (ffn_igemm_kernel_name answers); 4: ffn_dift_match; 5: ffn_resize_pil_bilinear_u8, ffn_vit_patch_rows; 6: ffn_resize_pil_u8; 7: ffn_vit_patch_rows_pair
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

// ---- operand preparation of the split-bf16 GEMMs; the 4-output-channel convolution (conv_small.h) ---------------------------------------------
extern "C" int ffn_split_pair(void* stream, const float* src, void* dst, long rows, int C, int ld_src) {
    REQUIRE(src && dst && rows > 0 && C > 0 && C % 4 == 0 && ld_src >= C && ld_src % 4 == 0, "split_pair: bad arguments (C=%d, ld_src=%d)", C, ld_src);
    REQUIRE(aligned16(src) && aligned16(dst), "split_pair: pointers must be 16-byte aligned");
    if (C % 8 == 0) LAUNCH(split_pair8_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, (bf16*)dst, rows, C, ld_src);
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
    const int cols_ = C / epc < 256 ? C / epc : 256;
    const int lds = (256 / cols_ > 0 ? 256 / cols_ : 1) * cols_ * 2 * epc * (int)sizeof(float);      // [pixel rows of threads][columns][2 x EPC]
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
        if (C % 8 == 0) {
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
