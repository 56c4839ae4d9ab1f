// A translation unit of libfreefine_hip.so for one kernel: attn_x3w_kernel (attention_x3w.h) runs ONE wave per SIMD on the whole 512-register file, and at that
// occupancy hipcc's default code generation works against it:
//   -mllvm -amdgpu-mfma-vgpr-form   MFMA results in the architectural VGPRs.  By default a kernel that may use more than 256 registers gets the
//                                   AGPR-destination MFMA forms, and every softmax instruction on the scores then goes through v_accvgpr_read / _write
//                                   copies (measured on the first version: 190 copies per 64 keys, and spills);
//   -fno-slp-vectorize              no v_pk_add_f32 / v_pk_mul_f32 in the gaps between MFMAs (a packed f32 instruction costs more issue time there
//                                   than the two scalar ones it replaces: MI355X_MICROARCH.md, price of one filler beside MFMAs).
// Built by __graft_entry__.build() into its own object; ffn_attn (capi_attn.hip) opts in to the LDS size and launches the kernel like every other.
// No exported symbol: fx3w_kernel and fx3w_lds_bytes (attn_units.h) have hidden visibility.
#include <hip/hip_runtime.h>

#include "attention_x3w.h"
#include "attn_units.h"

int fx3w_lds_bytes(void) { return attn_x3w_lds_bytes(); }

attn_kernel_t fx3w_kernel(int masks) { return masks ? attn_x3w_kernel<true> : attn_x3w_kernel<false>; }
