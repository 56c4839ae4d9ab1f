// Fifth translation unit of libfreefine_hip.so: the device image preparation of the DINOv2 feature metrics (imgprep.h) and the device case preparation of the
// GeoBench harness (caseprep.h) and the image preparation, mask product and upsampling of click-to-mask (sam.h).  A unit of its own, like dift.hip, so that it compiles beside capi.hip; default code generation.  capi.o validates the arguments
// (ffn_resize_pil_bilinear_u8, ffn_resize_pil_u8, ffn_vit_patch_rows, ffn_vit_patch_rows_pair; ffn_resize_taps8_u8, ffn_resize_gather_u8, ffn_dilate_u8,
// ffn_mask_bbox_u8, ffn_coarse_edit_2d; ffn_sam_patch_rows, ffn_sam_patch_rows_pair, ffn_hyper_masks, ffn_upsample_bicubic, ffn_upsample_bicubic_stats, ffn_box_nms) and calls the hidden functions below; nothing here is exported.
#include <hip/hip_runtime.h>

#include "../../include/freefine_hip.h"
#include "imgprep.h"
#include "caseprep.h"      // it turns floating-point contraction off for what follows
#include "sam.h"           // (contraction off as well)

extern "C" __attribute__((visibility("hidden"))) void fimgprep_resize(hipStream_t s, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int oh, int ow,
                                                                      const int* hb, const int* hk, int hks, const int* vb, const int* vk, int vks) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)H, (unsigned)B), dim3(IMGPREP_THREADS), 0, s, src, scratch, W, ow, hb, hk, hks);
    const int row_bytes = 3 * ow;
    hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((row_bytes + IMGPREP_THREADS - 1) / IMGPREP_THREADS), (unsigned)oh, (unsigned)B), dim3(IMGPREP_THREADS), 0, s,
                       scratch, dst, H, oh, row_bytes, vb, vk, vks);
}

extern "C" __attribute__((visibility("hidden"))) void fimgprep_resize_win(hipStream_t s, const ffn_resize_pil_desc* d) {
    (void)hipGetLastError();
    const dim3 gh((unsigned)d->H, (unsigned)d->B), blk(IMGPREP_THREADS);
    if (d->C == 1)
        hipLaunchKernelGGL(resize_win_h_kernel<1>, gh, blk, 0, s, d->src, d->scratch, d->m1, d->m2, d->rule, d->W, d->x0, d->cw, d->hbounds, d->hcoef, d->hksize);
    else
        hipLaunchKernelGGL(resize_win_h_kernel<3>, gh, blk, 0, s, d->src, d->scratch, d->m1, d->m2, d->rule, d->W, d->x0, d->cw, d->hbounds, d->hcoef, d->hksize);
    const int row_bytes = d->C * d->cw;
    hipLaunchKernelGGL(resize_win_v_kernel, dim3((unsigned)((row_bytes + IMGPREP_THREADS - 1) / IMGPREP_THREADS), (unsigned)d->ch, (unsigned)d->B), blk, 0, s, d->scratch,
                       d->dst, d->H, d->y0, d->ch, row_bytes, d->vbounds, d->vcoef, d->vksize);
}

extern "C" __attribute__((visibility("hidden"))) void fimgprep_patch_rows(hipStream_t s, int dtype, const uint8_t* src, const float* lut, void* out, int B, int H, int W,
                                                                          int ps, int ldo) {
    (void)hipGetLastError();
    const long total = (long)B * (H / ps) * (W / ps) * ldo;
    long g = (total + IMGPREP_THREADS - 1) / IMGPREP_THREADS;
    const unsigned grid = (unsigned)(g > 8192 ? 8192 : g);
    if (dtype == FFN_BF16) hipLaunchKernelGGL(patch_rows_kernel<bf16>, dim3(grid), dim3(IMGPREP_THREADS), 0, s, src, lut, static_cast<bf16*>(out), total, H, W, ps, ldo);
    else hipLaunchKernelGGL(patch_rows_kernel<float>, dim3(grid), dim3(IMGPREP_THREADS), 0, s, src, lut, static_cast<float*>(out), total, H, W, ps, ldo);
}

extern "C" __attribute__((visibility("hidden"))) void fimgprep_patch_rows_pair(hipStream_t s, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int ps,
                                                                               int K) {
    (void)hipGetLastError();
    const long total = (long)B * (H / ps) * (W / ps) * (K / 8);      // one thread per 8 columns
    long g = (total + IMGPREP_THREADS - 1) / IMGPREP_THREADS;
    const unsigned grid = (unsigned)(g > 8192 ? 8192 : g);
    hipLaunchKernelGGL(patch_rows_pair_kernel, dim3(grid), dim3(IMGPREP_THREADS), 0, s, src, lut, static_cast<bf16*>(out), total, H, W, ps, K);
}

// ---- case preparation of the GeoBench harness (caseprep.h) -----------------------------------------------------------------------------------------
static inline unsigned caseprep_blocks(long n) { return (unsigned)((n + CASEPREP_THREADS - 1) / CASEPREP_THREADS); }

extern "C" __attribute__((visibility("hidden"))) void fcaseprep_taps8(hipStream_t s, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow,
                                                                      const int* iy, const double* wy, const int* ix, const double* wx) {
    (void)hipGetLastError();
    const dim3 grid(caseprep_blocks(ow), (unsigned)oh, (unsigned)B), blk(CASEPREP_THREADS);
    if (C == 1) hipLaunchKernelGGL(lanczos8_kernel<1>, grid, blk, 0, s, src, dst, H, W, oh, ow, iy, wy, ix, wx);
    else hipLaunchKernelGGL(lanczos8_kernel<3>, grid, blk, 0, s, src, dst, H, W, oh, ow, iy, wy, ix, wx);
}

extern "C" __attribute__((visibility("hidden"))) void fcaseprep_gather(hipStream_t s, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow,
                                                                       const int* iy, const int* ix, int binarise) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(gather_kernel, dim3(caseprep_blocks((long)ow * C), (unsigned)oh, (unsigned)B), dim3(CASEPREP_THREADS), 0, s, src, dst, H, W, C, oh, ow, iy, ix, binarise);
}

extern "C" __attribute__((visibility("hidden"))) void fcaseprep_dilate(hipStream_t s, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int C, int k) {
    (void)hipGetLastError();
    const dim3 grid(caseprep_blocks((long)W * C), (unsigned)H, (unsigned)B), blk(CASEPREP_THREADS);
    hipLaunchKernelGGL(dilate_h_kernel, grid, blk, 0, s, src, scratch, W, C, k);
    hipLaunchKernelGGL(dilate_v_kernel, grid, blk, 0, s, scratch, dst, H, W * C, k);
}

extern "C" __attribute__((visibility("hidden"))) hipError_t fcaseprep_bbox(hipStream_t s, const uint8_t* mask, int* box, int B, int H, int W, int C) {
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(box, 0x80, (size_t)B * 4 * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mask_bbox_kernel, dim3((unsigned)(H < 64 ? H : 64), (unsigned)B), dim3(CASEPREP_THREADS), 0, s, mask, box, H, W, C);
    return hipSuccess;
}

extern "C" __attribute__((visibility("hidden"))) void fcaseprep_edit(hipStream_t s, const ffn_coarse_edit_desc* d) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(coarse_edit_kernel, dim3(caseprep_blocks(d->W), (unsigned)d->H, (unsigned)d->B), dim3(CASEPREP_THREADS), 0, s, *d);
}

// ---- click-to-mask (sam.h) -----------------------------------------------------------------------------------------------------------------------
static inline unsigned sam_grid(long n) {
    const long g = (n + SAM_THREADS - 1) / SAM_THREADS;
    return (unsigned)(g > 8192 ? 8192 : g);
}
static inline sam_norm sam_norm_of(const float* mean, const float* std) { return sam_norm{{mean[0], mean[1], mean[2]}, {std[0], std[1], std[2]}}; }

extern "C" __attribute__((visibility("hidden"))) void fsam_patch_rows(hipStream_t s, int dtype, const uint8_t* src, void* out, int B, int H, int W, int side, int ps, int ldo,
                                                                      const float* mean, const float* std) {
    (void)hipGetLastError();
    const long total = (long)B * (side / ps) * (side / ps) * ldo;
    if (dtype == FFN_BF16)
        hipLaunchKernelGGL(sam_patch_rows_kernel<bf16>, dim3(sam_grid(total)), dim3(SAM_THREADS), 0, s, src, static_cast<bf16*>(out), total, H, W, side, ps, ldo, sam_norm_of(mean, std));
    else
        hipLaunchKernelGGL(sam_patch_rows_kernel<float>, dim3(sam_grid(total)), dim3(SAM_THREADS), 0, s, src, static_cast<float*>(out), total, H, W, side, ps, ldo, sam_norm_of(mean, std));
}

extern "C" __attribute__((visibility("hidden"))) void fsam_patch_rows_pair(hipStream_t s, const uint8_t* src, void* out, int B, int H, int W, int side, int ps, int K,
                                                                           const float* mean, const float* std) {
    (void)hipGetLastError();
    const long total = (long)B * (side / ps) * (side / ps) * (K / 8);      // one thread per 8 columns
    hipLaunchKernelGGL(sam_patch_rows_pair_kernel, dim3(sam_grid(total)), dim3(SAM_THREADS), 0, s, src, static_cast<bf16*>(out), total, H, W, side, ps, K, sam_norm_of(mean, std));
}

extern "C" __attribute__((visibility("hidden"))) void fsam_hyper_masks(hipStream_t s, const float* up, const float* hyper, float* out, int N, int hw, int C, int M) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(hyper_masks_kernel, dim3((unsigned)((hw + SAM_THREADS - 1) / SAM_THREADS), (unsigned)N), dim3(SAM_THREADS), 0, s, up, hyper, out, hw, C, M);
}

extern "C" __attribute__((visibility("hidden"))) void fsam_bicubic(hipStream_t s, const float* src, float* dst, uint8_t* mask, int N, int h, int w, int H, int W) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(upsample_bicubic_kernel, dim3((unsigned)((W + SAM_THREADS - 1) / SAM_THREADS), (unsigned)H, (unsigned)N), dim3(SAM_THREADS), 0, s, src, dst, mask, h, w, H, W);
}

extern "C" __attribute__((visibility("hidden"))) void fsam_bicubic_stats(hipStream_t s, const float* src, int* stats, uint8_t* mask, int N, int h, int w, int H, int W,
                                                                         float offset) {
    (void)hipGetLastError();
    const dim3 maps((unsigned)((N + SAM_THREADS - 1) / SAM_THREADS)), blk(SAM_THREADS);
    hipLaunchKernelGGL(bicubic_stats_init_kernel, maps, blk, 0, s, stats, N);
    hipLaunchKernelGGL(upsample_bicubic_stats_kernel, dim3((unsigned)(H < SAM_STATS_ROW_BLOCKS ? H : SAM_STATS_ROW_BLOCKS), (unsigned)N), blk, 0, s, src, stats, mask, h, w, H,
                       W, offset);
    hipLaunchKernelGGL(bicubic_stats_finish_kernel, maps, blk, 0, s, stats, N);
}

extern "C" __attribute__((visibility("hidden"))) void fsam_box_nms(hipStream_t s, const float* boxes, unsigned long long* suppress, int M, float thresh) {
    (void)hipGetLastError();
    const unsigned nb = (unsigned)((M + SAM_WAVE - 1) / SAM_WAVE);
    hipLaunchKernelGGL(box_nms_kernel, dim3(nb, nb), dim3(SAM_WAVE), 0, s, boxes, suppress, M, thresh);
}
