// The attention kernels that are compiled outside capi_attn.hip, as ffn_attn (capi_attn.hip) reaches them: the defining unit and the calling unit both
// include this header, so the signatures cannot drift apart.  Internal to the library: hidden visibility.
#pragma once
#include "../../include/freefine_hip.h"

typedef void (*attn_kernel_t)(ffn_attn_desc);
// attn_x3w.hip (its own code generation flags): attn_x3w_kernel<masks>, for descriptors whose k / vt are the pre-split images (kv_pair), and its LDS bytes
extern "C" __attribute__((visibility("hidden"))) attn_kernel_t fx3w_kernel(int masks);
extern "C" __attribute__((visibility("hidden"))) int fx3w_lds_bytes(void);
// attn_causal.hip: attn_causal_kernel in the arithmetic of dtype (FFN_F32 / FFN_BF16 / FFN_BF16X3)
extern "C" __attribute__((visibility("hidden"))) attn_kernel_t fcausal_kernel(int dtype);
