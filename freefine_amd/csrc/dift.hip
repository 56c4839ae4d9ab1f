// The Mean Distance metric's unit of libfreefine_hip.so: the DIFT correspondence search (dift_match.h) and the SIFT keypoint stages (sift.h: detector,
// descriptor, ratio-test matcher).  Default code generation.  The unit exports the entries of its own kernels (ffn_dift_*, ffn_sift_*,
// ffn_gauss_blur_f32, ffn_decimate2_f32, ffn_knn2_u8).
#include "capi_common.h"
#include "dift_match.h"
#include "sift.h"

namespace {
// workspace layout in floats.  Tm and q come first: their rows are read with 16-byte loads (C % 4 == 0, the workspace is 16-byte aligned).
struct DiftWs {
    long tm, q, n, r, dn, dr, dl, qn, d, total;
    DiftWs(int C, int h, int w, int K) {
        const long hw = (long)h * w;
        tm = 0;
        q = tm + hw * C;
        n = q + (long)K * C;
        r = n + hw;
        dn = r + hw;
        dr = dn + hw;
        dl = dr + hw;
        qn = dl + hw;
        d = qn + K;
        total = d + (long)K * hw;
    }
    long bytes() const { return total * (long)sizeof(float); }
};

template <typename T>
void launch(hipStream_t s, const ffn_dift_desc& d) {
    const DiftWs o(d.C, d.h, d.w, d.K);
    float* ws = static_cast<float*>(d.ws);
    const int hw = d.h * d.w;
    const float sy = (float)d.h / (float)d.H, sx = (float)d.w / (float)d.W;      // ATen: float(input_size) / output_size
    const unsigned gpos = (unsigned)((hw + 3) / 4);                              // one wave per position, four waves per workgroup
    hipLaunchKernelGGL(dift_mean_kernel<T>, dim3(gpos), dim3(256), 0, s, static_cast<const T*>(d.tgt), d.es, d.ld, d.E, d.C, hw, ws + o.tm);
    hipLaunchKernelGGL(dift_gram_kernel, dim3(gpos), dim3(256), 0, s, ws + o.tm, d.C, d.h, d.w, ws + o.n, ws + o.r, ws + o.dn, ws + o.dr, ws + o.dl);
    for (int k0 = 0; k0 < d.K; k0 += DIFT_KP_PER_LAUNCH) {                       // keypoints travel as kernel arguments, DIFT_KP_PER_LAUNCH at a time
        const int n = d.K - k0 < DIFT_KP_PER_LAUNCH ? d.K - k0 : DIFT_KP_PER_LAUNCH;
        dift_kps kp = {};
        for (int i = 0; i < n; ++i) {
            kp.rc[i][0] = d.kps[2 * (k0 + i)];
            kp.rc[i][1] = d.kps[2 * (k0 + i) + 1];
        }
        float* q = ws + o.q + (long)k0 * d.C;
        float* D = ws + o.d + (long)k0 * hw;
        hipLaunchKernelGGL(dift_query_kernel<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, static_cast<const T*>(d.src), d.es, d.ld, d.E, d.C, d.h, d.w, sy, sx,
                           kp, n, q, ws + o.qn + k0);
        hipLaunchKernelGGL(dift_dots_kernel, dim3(gpos), dim3(256), 0, s, ws + o.tm, q, d.C, hw, n, D);
        hipLaunchKernelGGL(dift_match_kernel, dim3((unsigned)n), dim3(DIFT_MATCH_THREADS), 0, s, ws + o.n, ws + o.r, ws + o.dn, ws + o.dr, ws + o.dl, D,
                           ws + o.qn + k0, d.h, d.w, d.H, d.W, sy, sx, d.out_rc + 2 * k0, d.out_cos + k0);
    }
}
}  // namespace

extern "C" long ffn_dift_workspace_bytes(int C, int h, int w, int K) {
    REQUIRE(C > 0 && C % 4 == 0 && h >= 1 && w >= 1 && K >= 1 && (long)h * w < (1l << 31), "dift_workspace_bytes: bad shape C=%d h=%d w=%d K=%d (C %% 4 == 0)", C, h, w, K);
    return DiftWs(C, h, w, K).bytes();
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
    const long need = DiftWs(d.C, d.h, d.w, d.K).bytes();
    REQUIRE(d.ws_bytes >= need, "dift_match: workspace of %ld bytes, %ld needed (ffn_dift_workspace_bytes)", d.ws_bytes, need);
    for (int k = 0; k < d.K; ++k)
        REQUIRE(d.kps[2 * k] >= 0 && d.kps[2 * k] < d.H && d.kps[2 * k + 1] >= 0 && d.kps[2 * k + 1] < d.W, "dift_match: keypoint %d = (%d, %d) outside [0, %d) x [0, %d)", k,
                d.kps[2 * k], d.kps[2 * k + 1], d.H, d.W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (d.dtype == FFN_BF16) launch<bf16>(s, d);
    else launch<float>(s, d);
    return check_launch("dift_match");
}

// ---- SIFT keypoints, descriptors and matching (sift.h).  Grids are exact (one thread per element / one workgroup per item). ------------------------------------
static inline unsigned sift_blocks(long n) { return (unsigned)((n + 255) / 256); }
static inline bool sift_side_ok(int h, int w) { return h >= 1 && w >= 1 && h <= FFN_SIFT_MAX_SIDE && w <= FFN_SIFT_MAX_SIDE; }

extern "C" int ffn_sift_base(void* stream, const uint8_t* img, float* out, int H, int W, int C) {
    REQUIRE(img && out, "sift_base: null pointer");
    REQUIRE(H >= 1 && W >= 1 && 2 * H <= FFN_SIFT_MAX_SIDE && 2 * W <= FFN_SIFT_MAX_SIDE && (C == 1 || C == 3), "sift_base: bad shape H=%d W=%d C=%d (C in {1, 3}, sides <= %d)", H, W,
            C, FFN_SIFT_MAX_SIDE / 2);
    LAUNCH(sift_base_kernel, dim3(sift_blocks(4l * H * W)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), img, out, H, W, C);
    return check_launch("sift_base");
}

extern "C" int ffn_gauss_blur_f32(void* stream, const float* src, float* dst, float* tmp, int H, int W, const float* taps, int T) {
    REQUIRE(src && dst && tmp && taps, "gauss_blur_f32: null pointer");
    REQUIRE(tmp != src && tmp != dst, "gauss_blur_f32: tmp must be a buffer of its own");
    REQUIRE(sift_side_ok(H, W), "gauss_blur_f32: bad shape H=%d W=%d (sides 1 .. %d)", H, W, FFN_SIFT_MAX_SIDE);
    REQUIRE(T >= 1 && T <= FFN_SIFT_MAX_TAPS && (T & 1), "gauss_blur_f32: %d taps (odd, 1 .. %d)", T, FFN_SIFT_MAX_TAPS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    sift_taps t = {};
    t.T = T;
    for (int i = 0; i < T; ++i) t.t[i] = taps[i];
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_blur_kernel<false>, dim3(sift_blocks((long)H * W)), dim3(256), 0, s, src, tmp, H, W, t);
    hipLaunchKernelGGL(sift_blur_kernel<true>, dim3(sift_blocks((long)H * W)), dim3(256), 0, s, (const float*)tmp, dst, H, W, t);
    return check_launch("gauss_blur_f32");
}

extern "C" int ffn_decimate2_f32(void* stream, const float* src, float* dst, int H, int W) {
    REQUIRE(src && dst && src != dst, "decimate2_f32: null or aliased pointer");
    REQUIRE(sift_side_ok(H, W) && H >= 2 && W >= 2, "decimate2_f32: bad shape H=%d W=%d (sides 2 .. %d)", H, W, FFN_SIFT_MAX_SIDE);
    LAUNCH(sift_decimate_kernel, dim3(sift_blocks((long)(H / 2) * (W / 2))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, dst, H, W);
    return check_launch("decimate2_f32");
}

// *count = the number of extrema (possibly beyond cap: the list then holds the first cap in arrival order, and the entry answers FFN_ENOSPC)
extern "C" int ffn_sift_extrema(void* stream, const float* gauss, float* dog, int h, int w, int* cand, int cap, int* counter, int* count) {
    REQUIRE(gauss && dog && cand && counter && count, "sift_extrema: null pointer");
    REQUIRE(sift_side_ok(h, w) && cap >= 1, "sift_extrema: bad shape h=%d w=%d cap=%d (sides 1 .. %d, cap >= 1)", h, w, cap, FFN_SIFT_MAX_SIDE);
    *count = 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(int), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sift_dog_kernel, dim3(sift_blocks(5l * h * w)), dim3(256), 0, s, gauss, dog, (long)h * w);
        if (h > 2 * SIFT_BORDER && w > 2 * SIFT_BORDER)
            hipLaunchKernelGGL(sift_extrema_kernel, dim3(sift_blocks(3l * (h - 2 * SIFT_BORDER) * (w - 2 * SIFT_BORDER))), dim3(256), 0, s, (const float*)dog, h, w, cand, cap, counter);
        e = hipMemcpyAsync(count, counter, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return fail(FFN_EHIP, "sift_extrema: %s", hipGetErrorString(e));
    if (*count > cap) return fail(FFN_ENOSPC, "sift_extrema: %d extrema but room for %d: call again with a longer list", *count, cap);
    return check_launch("sift_extrema");
}

extern "C" int ffn_sift_refine_orient(void* stream, const float* dog, const float* gauss, int h, int w, int octave, const int* cand, int n, float* out) {
    REQUIRE(n >= 0, "sift_refine_orient: n=%d", n);
    if (n == 0) return FFN_OK;
    REQUIRE(dog && gauss && cand && out, "sift_refine_orient: null pointer");
    REQUIRE(sift_side_ok(h, w) && octave >= 0 && octave < 24, "sift_refine_orient: bad shape h=%d w=%d octave=%d", h, w, octave);
    LAUNCH(sift_refine_kernel, dim3((unsigned)n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), dog, gauss, h, w, octave, cand, n, out);
    return check_launch("sift_refine_orient");
}

extern "C" int ffn_sift_describe(void* stream, const float* gauss, int h, int w, int octave, const float* kp, int n, uint8_t* desc, float* raw) {
    REQUIRE(n >= 0, "sift_describe: n=%d", n);
    if (n == 0) return FFN_OK;
    REQUIRE(gauss && kp && desc, "sift_describe: null pointer");
    REQUIRE(sift_side_ok(h, w) && octave >= 0 && octave < 24, "sift_describe: bad shape h=%d w=%d octave=%d", h, w, octave);
    LAUNCH(sift_describe_kernel, dim3((unsigned)n), dim3(SIFT_DESC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), gauss, h, w, octave, kp, n, desc, raw);
    return check_launch("sift_describe");
}

extern "C" int ffn_knn2_u8(void* stream, const uint8_t* des1, int n1, const uint8_t* des2, int n2, int* idx, int* dist) {
    REQUIRE(n1 >= 0 && n2 >= 0, "knn2_u8: n1=%d n2=%d", n1, n2);
    if (n1 == 0) return FFN_OK;
    REQUIRE(des1 && idx && dist && (des2 || n2 == 0), "knn2_u8: null pointer");
    REQUIRE((reinterpret_cast<uintptr_t>(des1) & 3) == 0 && (reinterpret_cast<uintptr_t>(des2) & 3) == 0, "knn2_u8: descriptor rows are read as 32-bit words: 4-byte alignment");
    LAUNCH(knn2_u8_kernel, dim3((unsigned)n1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), des1, des2, n2, idx, dist);
    return check_launch("knn2_u8");
}
