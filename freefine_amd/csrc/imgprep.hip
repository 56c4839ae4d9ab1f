// The image-side preparation unit of libfreefine_hip.so: the device image preparation of the DINOv2 feature metrics (imgprep.h), the device case
// preparation of the GeoBench harness (caseprep.h), and the image preparation, mask product, upsampling, candidate statistics and box NMS of click-to-mask
// and automatic mask generation (sam.h).  Default code generation.  The unit exports the entries of its own kernels.
#include "capi_common.h"
#include "imgprep.h"
#include "caseprep.h"      // it turns floating-point contraction off for what follows
#include "sam.h"           // (contraction off as well)

// ---- image preparation of the DINOv2 feature metrics (imgprep.h) -----------------------------------------------------------------------------------
static inline int pil_ksize(int in, int out) { return 2 * (in > out ? (in + out - 1) / out : 1) + 1; }      // 2 ceil(max(in / out, 1)) + 1
static inline unsigned imgprep_grid(long n) {
    const long g = (n + IMGPREP_THREADS - 1) / IMGPREP_THREADS;
    return (unsigned)(g > 8192 ? 8192 : g);
}

extern "C" int ffn_resize_pil_bilinear_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int oh, int ow,
                                          const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef, int vksize) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && dst && scratch && hbounds && hcoef && vbounds && vcoef, "resize_pil_bilinear_u8: null pointer");
    REQUIRE(B >= 1 && B <= 65535, "resize_pil_bilinear_u8: B=%d outside 1 .. 65535", B);
    REQUIRE(H >= 1 && W >= 1 && H <= lim && W <= lim, "resize_pil_bilinear_u8: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", H, W, lim);
    REQUIRE(oh >= 1 && ow >= 1 && oh <= lim && ow <= lim, "resize_pil_bilinear_u8: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", oh, ow, lim);
    REQUIRE(hksize == pil_ksize(W, ow) && vksize == pil_ksize(H, oh), "resize_pil_bilinear_u8: table widths %d, %d; %d -> %d and %d -> %d need %d, %d", hksize, vksize, W, ow,
            H, oh, pil_ksize(W, ow), pil_ksize(H, oh));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)H, (unsigned)B), dim3(IMGPREP_THREADS), 0, s, src, scratch, W, ow, hbounds, hcoef, hksize);
    const int row_bytes = 3 * ow;
    hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((row_bytes + IMGPREP_THREADS - 1) / IMGPREP_THREADS), (unsigned)oh, (unsigned)B), dim3(IMGPREP_THREADS), 0, s,
                       scratch, dst, H, oh, row_bytes, vbounds, vcoef, vksize);
    return check_launch("resize_pil_bilinear_u8");
}

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
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    const dim3 gh((unsigned)d->H, (unsigned)d->B), blk(IMGPREP_THREADS);
    if (d->C == 1)
        hipLaunchKernelGGL(resize_win_h_kernel<1>, gh, blk, 0, s, d->src, d->scratch, d->m1, d->m2, d->rule, d->W, d->x0, d->cw, d->hbounds, d->hcoef, d->hksize);
    else
        hipLaunchKernelGGL(resize_win_h_kernel<3>, gh, blk, 0, s, d->src, d->scratch, d->m1, d->m2, d->rule, d->W, d->x0, d->cw, d->hbounds, d->hcoef, d->hksize);
    const int row_bytes = d->C * d->cw;
    hipLaunchKernelGGL(resize_win_v_kernel, dim3((unsigned)((row_bytes + IMGPREP_THREADS - 1) / IMGPREP_THREADS), (unsigned)d->ch, (unsigned)d->B), blk, 0, s, d->scratch,
                       d->dst, d->H, d->y0, d->ch, row_bytes, d->vbounds, d->vcoef, d->vksize);
    return check_launch("resize_pil_u8");
}

extern "C" int ffn_vit_patch_rows(void* stream, int dtype, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int patch, int ldo) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(dtype == FFN_F32 || dtype == FFN_BF16, "vit_patch_rows: bad dtype %d", dtype);
    REQUIRE(src && lut && out, "vit_patch_rows: null pointer");
    REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= lim && W <= lim, "vit_patch_rows: bad shape B=%d, %d x %d (sides 1 .. %d, FFN_IMGPREP_MAX_SIDE)", B, H, W, lim);
    REQUIRE(patch >= 1 && patch <= 256 && H % patch == 0 && W % patch == 0, "vit_patch_rows: %d x %d is not whole patches of %d (1 .. 256)", H, W, patch);
    REQUIRE(ldo >= 3 * patch * patch, "vit_patch_rows: ldo=%d below the %d columns of a patch", ldo, 3 * patch * patch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long total = (long)B * (H / patch) * (W / patch) * ldo;
    if (dtype == FFN_BF16) LAUNCH(patch_rows_kernel<bf16>, dim3(imgprep_grid(total)), dim3(IMGPREP_THREADS), 0, s, src, lut, static_cast<bf16*>(out), total, H, W, patch, ldo);
    else LAUNCH(patch_rows_kernel<float>, dim3(imgprep_grid(total)), dim3(IMGPREP_THREADS), 0, s, src, lut, static_cast<float*>(out), total, H, W, patch, ldo);
    return check_launch("vit_patch_rows");
}

// the same rows as the pair operand of an FFN_BF16X3 GEMM (ABI version 7): 8 columns per thread, 16-byte stores
extern "C" int ffn_vit_patch_rows_pair(void* stream, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int patch, int K) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && lut && out, "vit_patch_rows_pair: null pointer");
    REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= lim && W <= lim, "vit_patch_rows_pair: bad shape B=%d, %d x %d (sides 1 .. %d, FFN_IMGPREP_MAX_SIDE)", B, H, W, lim);
    REQUIRE(patch >= 1 && patch <= 256 && H % patch == 0 && W % patch == 0, "vit_patch_rows_pair: %d x %d is not whole patches of %d (1 .. 256)", H, W, patch);
    REQUIRE(K >= 3 * patch * patch, "vit_patch_rows_pair: K=%d below the %d columns of a patch", K, 3 * patch * patch);
    REQUIRE(K % 8 == 0, "vit_patch_rows_pair: K=%d is not a multiple of 8 (16-byte stores of both halves)", K);
    REQUIRE(aligned16(out), "vit_patch_rows_pair: out must be 16-byte aligned");
    const long total = (long)B * (H / patch) * (W / patch) * (K / 8);      // one thread per 8 columns
    LAUNCH(patch_rows_pair_kernel, dim3(imgprep_grid(total)), dim3(IMGPREP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, lut, static_cast<bf16*>(out), total, H, W,
           patch, K);
    return check_launch("vit_patch_rows_pair");
}

// ---- case preparation of the GeoBench harness (caseprep.h) -----------------------------------------------------------------------------------------
static inline unsigned caseprep_blocks(long n) { return (unsigned)((n + CASEPREP_THREADS - 1) / CASEPREP_THREADS); }

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
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(caseprep_blocks(ow), (unsigned)oh, (unsigned)B), blk(CASEPREP_THREADS);
    if (C == 1) LAUNCH(lanczos8_kernel<1>, grid, blk, 0, s, src, dst, H, W, oh, ow, iy, wy, ix, wx);
    else LAUNCH(lanczos8_kernel<3>, grid, blk, 0, s, src, dst, H, W, oh, ow, iy, wy, ix, wx);
    return check_launch("resize_taps8_u8");
}

extern "C" int ffn_resize_gather_u8(void* stream, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow, const int* iy, const int* ix, int binarise) {
    REQUIRE(src && dst && iy && ix, "resize_gather_u8: null pointer");
    CASEPREP_IMAGE("resize_gather_u8", B, H, W, C);
    CASEPREP_IMAGE("resize_gather_u8", B, oh, ow, C);
    LAUNCH(gather_kernel, dim3(caseprep_blocks((long)ow * C), (unsigned)oh, (unsigned)B), dim3(CASEPREP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, dst, H, W, C, oh,
           ow, iy, ix, binarise);
    return check_launch("resize_gather_u8");
}

extern "C" int ffn_dilate_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int C, int k) {
    REQUIRE(src && dst && scratch, "dilate_u8: null pointer");
    CASEPREP_IMAGE("dilate_u8", B, H, W, C);
    REQUIRE(k >= 1 && k <= 255, "dilate_u8: k=%d outside 1 .. 255", k);
    REQUIRE(dst != src && dst != scratch && scratch != src, "dilate_u8: src, scratch and dst must be three buffers");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    const dim3 grid(caseprep_blocks((long)W * C), (unsigned)H, (unsigned)B), blk(CASEPREP_THREADS);
    hipLaunchKernelGGL(dilate_h_kernel, grid, blk, 0, s, src, scratch, W, C, k);
    hipLaunchKernelGGL(dilate_v_kernel, grid, blk, 0, s, scratch, dst, H, W * C, k);
    return check_launch("dilate_u8");
}

extern "C" int ffn_mask_bbox_u8(void* stream, const uint8_t* mask, int* box, int B, int H, int W, int C) {
    REQUIRE(mask && box, "mask_bbox_u8: null pointer");
    CASEPREP_IMAGE("mask_bbox_u8", B, H, W, C);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(box, 0x80, (size_t)B * 4 * sizeof(int), s);
    if (e != hipSuccess) return fail(FFN_EHIP, "mask_bbox_u8: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(mask_bbox_kernel, dim3((unsigned)(H < 64 ? H : 64), (unsigned)B), dim3(CASEPREP_THREADS), 0, s, mask, box, H, W, C);
    return check_launch("mask_bbox_u8");
}

extern "C" int ffn_coarse_edit_2d(void* stream, const ffn_coarse_edit_desc* d) {
    REQUIRE(d, "coarse_edit_2d: null descriptor");
    REQUIRE(d->src_img && d->src_mask && d->bg && d->inv && d->final_img && d->tmask && d->trans_hole, "coarse_edit_2d: null pointer");
    CASEPREP_IMAGE("coarse_edit_2d", d->B, d->H, d->W, d->mask_c);
    REQUIRE(!d->hole_mask || d->hole_mask_c == 1 || d->hole_mask_c == 3, "coarse_edit_2d: hole_mask_c=%d channels (1 or 3)", d->hole_mask_c);
    LAUNCH(coarse_edit_kernel, dim3(caseprep_blocks(d->W), (unsigned)d->H, (unsigned)d->B), dim3(CASEPREP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *d);
    return check_launch("coarse_edit_2d");
}

// ---- click-to-mask: image preparation, mask product, bicubic upsampling (sam.h) ------------------------------------------------------------------------
static inline unsigned sam_grid(long n) {
    const long g = (n + SAM_THREADS - 1) / SAM_THREADS;
    return (unsigned)(g > 8192 ? 8192 : g);
}
static inline sam_norm sam_norm_of(const float* mean, const float* std) { return sam_norm{{mean[0], mean[1], mean[2]}, {std[0], std[1], std[2]}}; }

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
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long total = (long)B * (side / patch) * (side / patch) * ldo;
    if (dtype == FFN_BF16)
        LAUNCH(sam_patch_rows_kernel<bf16>, dim3(sam_grid(total)), dim3(SAM_THREADS), 0, s, src, static_cast<bf16*>(out), total, H, W, side, patch, ldo, sam_norm_of(mean, std));
    else
        LAUNCH(sam_patch_rows_kernel<float>, dim3(sam_grid(total)), dim3(SAM_THREADS), 0, s, src, static_cast<float*>(out), total, H, W, side, patch, ldo, sam_norm_of(mean, std));
    return check_launch("sam_patch_rows");
}

extern "C" int ffn_sam_patch_rows_pair(void* stream, const uint8_t* src, void* out, int B, int H, int W, int side, int patch, int K, const float* mean, const float* std) {
    SAM_PATCH_ROWS("sam_patch_rows_pair", K);
    REQUIRE(K % 8 == 0, "sam_patch_rows_pair: K=%d is not a multiple of 8 (16-byte stores of both halves)", K);
    REQUIRE(aligned16(out), "sam_patch_rows_pair: out must be 16-byte aligned");
    const long total = (long)B * (side / patch) * (side / patch) * (K / 8);      // one thread per 8 columns
    LAUNCH(sam_patch_rows_pair_kernel, dim3(sam_grid(total)), dim3(SAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, static_cast<bf16*>(out), total, H, W, side, patch,
           K, sam_norm_of(mean, std));
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
    LAUNCH(hyper_masks_kernel, dim3((unsigned)((hw + SAM_THREADS - 1) / SAM_THREADS), (unsigned)N), dim3(SAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), up, hyper, out, hw,
           C, M);
    return check_launch("hyper_masks");
}

extern "C" int ffn_upsample_bicubic(void* stream, const float* src, float* dst, uint8_t* mask, int N, int h, int w, int H, int W) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && dst, "upsample_bicubic: null pointer");
    REQUIRE(N >= 1 && N <= 65535, "upsample_bicubic: N=%d outside 1 .. 65535", N);
    REQUIRE(h >= 1 && w >= 1 && h <= lim && w <= lim, "upsample_bicubic: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", h, w, lim);
    REQUIRE(H >= 1 && W >= 1 && H <= lim && W <= lim, "upsample_bicubic: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", H, W, lim);
    LAUNCH(upsample_bicubic_kernel, dim3((unsigned)((W + SAM_THREADS - 1) / SAM_THREADS), (unsigned)H, (unsigned)N), dim3(SAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src,
           dst, mask, h, w, H, W);
    return check_launch("upsample_bicubic");
}

// ---- automatic mask generation: the statistics of the upsampled candidates, box NMS (sam.h) ---------------------------------------------------------
extern "C" int ffn_upsample_bicubic_stats(void* stream, const float* src, int32_t* stats, uint8_t* mask, int N, int h, int w, int H, int W, float offset) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && stats, "upsample_bicubic_stats: null pointer");
    REQUIRE(N >= 1 && N <= 65535, "upsample_bicubic_stats: N=%d outside 1 .. 65535", N);
    REQUIRE(h >= 1 && w >= 1 && h <= lim && w <= lim, "upsample_bicubic_stats: source %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", h, w, lim);
    REQUIRE(H >= 1 && W >= 1 && H <= lim && W <= lim, "upsample_bicubic_stats: destination %d x %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", H, W, lim);
    REQUIRE(__builtin_isfinite(offset) && offset >= 0.f, "upsample_bicubic_stats: offset=%g must be finite and >= 0", (double)offset);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    const dim3 maps((unsigned)((N + SAM_THREADS - 1) / SAM_THREADS)), blk(SAM_THREADS);
    hipLaunchKernelGGL(bicubic_stats_init_kernel, maps, blk, 0, s, stats, N);
    hipLaunchKernelGGL(upsample_bicubic_stats_kernel, dim3((unsigned)(H < SAM_STATS_ROW_BLOCKS ? H : SAM_STATS_ROW_BLOCKS), (unsigned)N), blk, 0, s, src, stats, mask, h, w, H,
                       W, offset);
    hipLaunchKernelGGL(bicubic_stats_finish_kernel, maps, blk, 0, s, stats, N);
    return check_launch("upsample_bicubic_stats");
}

extern "C" int ffn_box_nms(void* stream, const float* boxes, uint64_t* suppress, int M, float thresh) {
    REQUIRE(boxes && suppress, "box_nms: null pointer");
    REQUIRE(M >= 1 && M <= FFN_BOX_NMS_MAX, "box_nms: M=%d outside 1 .. %d (FFN_BOX_NMS_MAX)", M, FFN_BOX_NMS_MAX);
    REQUIRE(__builtin_isfinite(thresh), "box_nms: thresh=%g is not finite", (double)thresh);
    const unsigned nb = (unsigned)((M + SAM_WAVE - 1) / SAM_WAVE);
    LAUNCH(box_nms_kernel, dim3(nb, nb), dim3(SAM_WAVE), 0, reinterpret_cast<hipStream_t>(stream), boxes, reinterpret_cast<unsigned long long*>(suppress), M, thresh);
    return check_launch("box_nms");
}
