// Third translation unit of libfreefine_hip.so: the kernels only the CLIP text tower needs (attention_causal.h: attn_causal_kernel in its three
// arithmetic modes, embed_tokens_kernel).  A unit of its own so that they compile beside capi.hip (which takes minutes) instead of lengthening it; default
// code generation.  capi.o validates the descriptor, plans the launch and launches the kernel like every other.  No exported symbol: the getters have
// hidden visibility.
#include <hip/hip_runtime.h>

#include "attention_causal.h"

// dtype: FFN_F32 / FFN_BF16 / FFN_BF16X3
extern "C" __attribute__((visibility("hidden"))) void (*fcausal_kernel(int dtype))(ffn_attn_desc) {
    return dtype == FFN_BF16 ? attn_causal_kernel<bf16, false> : (dtype == FFN_BF16X3 ? attn_causal_kernel<float, true> : attn_causal_kernel<float, false>);
}

extern "C" __attribute__((visibility("hidden"))) void fembed_launch(hipStream_t s, int bf16_out, const int* ids, const float* table, const float* pos, void* out,
                                                                    long M, int S, int C, int V) {
    const long n4 = M * (C / 4);
    long grid = (n4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    (void)hipGetLastError();
    if (bf16_out) hipLaunchKernelGGL(embed_tokens_kernel<bf16>, dim3((unsigned)grid), dim3(256), 0, s, ids, table, pos, (bf16*)out, n4, S, C, V);
    else hipLaunchKernelGGL(embed_tokens_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, ids, table, pos, (float*)out, n4, S, C, V);
}
