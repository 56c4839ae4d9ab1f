// Fourth translation unit of libfreefine_hip.so: the DIFT correspondence search of the Mean Distance metric (dift_match.h).  A unit of its own, like
// attn_causal.hip, so that it compiles beside capi.hip; default code generation.  capi.o validates the descriptor (ffn_dift_match) and calls the two hidden
// functions below; nothing here is exported.
#include <hip/hip_runtime.h>

#include "../../include/freefine_hip.h"
#include "dift_match.h"

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
