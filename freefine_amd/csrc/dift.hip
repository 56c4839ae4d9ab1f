// Fourth translation unit of libfreefine_hip.so: the DIFT correspondence search of the Mean Distance metric (dift_match.h).  A unit of its own, like
// attn_causal.hip, so that it compiles beside capi.hip; default code generation.  capi.o validates the descriptor (ffn_dift_match) and calls the two hidden
// functions below; nothing here is exported.  The SIFT keypoint stages of the same metric (sift.h: detector, descriptor, ratio-test matcher) compile here too,
// behind the fsift_* launchers at the end.
#include <hip/hip_runtime.h>

#include "../../include/freefine_hip.h"
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

extern "C" __attribute__((visibility("hidden"))) long fdift_ws_bytes(int C, int h, int w, int K) { return DiftWs(C, h, w, K).total * (long)sizeof(float); }

extern "C" __attribute__((visibility("hidden"))) void fdift_launch(hipStream_t s, const ffn_dift_desc* d) {
    (void)hipGetLastError();
    if (d->dtype == FFN_BF16) launch<bf16>(s, *d);
    else launch<float>(s, *d);
}

// ---- SIFT (sift.h).  capi.o validates; these only launch.  Grids are exact (one thread per element / one workgroup per item). ------------------------------------
static inline unsigned sift_blocks(long n) { return (unsigned)((n + 255) / 256); }

extern "C" __attribute__((visibility("hidden"))) void fsift_base(hipStream_t s, const uint8_t* img, float* out, int H, int W, int C) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_base_kernel, dim3(sift_blocks(4l * H * W)), dim3(256), 0, s, img, out, H, W, C);
}

extern "C" __attribute__((visibility("hidden"))) void fsift_blur(hipStream_t s, const float* src, float* dst, float* tmp, int H, int W, const float* taps, int T) {
    sift_taps t = {};
    t.T = T;
    for (int i = 0; i < T; ++i) t.t[i] = taps[i];
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_blur_kernel<false>, dim3(sift_blocks((long)H * W)), dim3(256), 0, s, src, tmp, H, W, t);
    hipLaunchKernelGGL(sift_blur_kernel<true>, dim3(sift_blocks((long)H * W)), dim3(256), 0, s, (const float*)tmp, dst, H, W, t);
}

extern "C" __attribute__((visibility("hidden"))) void fsift_decimate(hipStream_t s, const float* src, float* dst, int H, int W) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_decimate_kernel, dim3(sift_blocks((long)(H / 2) * (W / 2))), dim3(256), 0, s, src, dst, H, W);
}

// -> hipSuccess and *found = the number of extrema (possibly beyond cap: the list then holds the first cap in arrival order), or the HIP error
extern "C" __attribute__((visibility("hidden"))) int fsift_extrema(hipStream_t s, const float* G, float* D, int h, int w, int* cand, int cap, int* counter, int* found) {
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sift_dog_kernel, dim3(sift_blocks(5l * h * w)), dim3(256), 0, s, G, D, (long)h * w);
    if (h > 2 * SIFT_BORDER && w > 2 * SIFT_BORDER)
        hipLaunchKernelGGL(sift_extrema_kernel, dim3(sift_blocks(3l * (h - 2 * SIFT_BORDER) * (w - 2 * SIFT_BORDER))), dim3(256), 0, s, (const float*)D, h, w, cand, cap, counter);
    e = hipMemcpyAsync(found, counter, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
}

extern "C" __attribute__((visibility("hidden"))) void fsift_refine(hipStream_t s, const float* D, const float* G, int h, int w, int o, const int* cand, int n, float* out) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_refine_kernel, dim3((unsigned)n), dim3(64), 0, s, D, G, h, w, o, cand, n, out);
}

extern "C" __attribute__((visibility("hidden"))) void fsift_describe(hipStream_t s, const float* G, int h, int w, int o, const float* kp, int n, uint8_t* desc, float* raw) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(sift_describe_kernel, dim3((unsigned)n), dim3(SIFT_DESC_THREADS), 0, s, G, h, w, o, kp, n, desc, raw);
}

extern "C" __attribute__((visibility("hidden"))) void fknn2_u8(hipStream_t s, const uint8_t* des1, int n1, const uint8_t* des2, int n2, int* idx, int* dist) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(knn2_u8_kernel, dim3((unsigned)n1), dim3(256), 0, s, des1, des2, n2, idx, dist);
}
