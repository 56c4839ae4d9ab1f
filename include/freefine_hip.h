/* freefine_hip.h -- C ABI of libfreefine_hip.so: the MI355X (gfx950) kernels behind the FreeFine
 * DDIM-inversion + guided-denoising hot path.
 *
 * The reference (CIawevy/FreeFine) has no FFI of its own: its "operator API" for this path is Python that
 * monkey-patches diffusers (src/utils/attention.py:226-564) and calls torch ops.  Each entry point below names
 * the reference code it replaces (paths relative to /root/reference).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. the torch caching allocator); the library never
 *     allocates, frees or retains memory; scratch is passed in explicitly;
 *   - every call enqueues on the hipStream_t given as `stream` (void* so the header needs no HIP include), is
 *     asynchronous with respect to the host and performs no synchronisation -> capturable in a hipGraph.  ONE exception:
 *     ffn_igemm in bf16, the FIRST time it sees a problem shape outside stream capture, times its candidate configurations on the
 *     stream (it synchronises the stream, rewrites `out` several times and holds a process-wide lock while it does); call
 *     ffn_igemm_tune() for every shape during warm-up -- or set FFN_IGEMM_TUNE=0 -- where that must not happen later (worker threads,
 *     latency-sensitive replays, runs that need identical tile choices on every rank);
 *   - return value 0 = success, negative = error (FFN_E*); ffn_last_error() returns a thread-local message;
 *   - dtype selects the element type of activations / weights: FFN_F32 (exact fp32 MFMA, "parity mode") or
 *     FFN_BF16 (bf16 MFMA operands, fp32 accumulation, "fast mode").  Norm parameters, biases, masks-as-weights,
 *     latents and scheduler tensors are always fp32;
 *   - activations are channel-contiguous: [batch, H*W, C].
 */
#ifndef FREEFINE_HIP_H
#define FREEFINE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { FFN_F32 = 0, FFN_BF16 = 1, FFN_BF16X3 = 2 /* ffn_igemm / ffn_attn: split-bf16 arithmetic, fp32 results (see ffn_igemm) */,
       FFN_FP8 = 3 /* ffn_igemm, 3x3 convolutions only: OCP e4m3 operands, bf16 results (see ffn_igemm) */ };
enum { FFN_OK = 0, FFN_EINVAL = -22, FFN_ENOSYS = -38, FFN_EHIP = -5, FFN_ENOSPC = -28 };      /* FFN_ENOSPC (ABI version 12): a caller-sized output list is too short */

int ffn_version(void);
const char* ffn_last_error(void);
/* fills name (<=64 bytes) with the gcnArchName of `device`, returns CU count or negative error. */
int ffn_device_info(int device, char* name, int name_len);
/* hipGraphLaunch(graph_exec, stream) through this library's HIP runtime.  Why it is in the ABI: a foreign-function call releases the host
 * language's interpreter lock, torch.cuda.CUDAGraph.replay() does not -- and on ROCm 7.2 a launch of a ~380-node UNet-forward graph holds the
 * calling thread for milliseconds, so the one-image-per-call layout (several host threads, one HIP stream each: the reference's
 * src/demo/model.py:577-617 loop run as it stands) serialised on that lock.  graph_exec = the hipGraphExec_t of a captured forward
 * (torch: CUDAGraph.raw_cuda_graph_exec()). */
int ffn_graph_launch(void* stream, void* graph_exec);

/* ---- implicit GEMM: Linear / 1x1 conv (dense A) and 3x3 conv (im2col gather) ------------------------------
 * out[m,n] = epi( alpha * sum_k A(m,k) W[n,k] ), W is [N][Kpad]: K contiguous, Kpad = row stride of W (>= K, multiple of
 * the 16-byte chunk: 4 f32 / 8 bf16); columns >= K are never read, so an activation can serve as W (attention-as-GEMM).
 * Replaces: diffusers ResnetBlock2D/Downsample2D/Upsample2D/Linear modules reached from override_forward
 * (src/utils/attention.py:105-214) and to_q/to_k/to_v/to_out in the hooked Attention.forward (attention.py:372-407). */
enum {
    FFN_IG_OUT_SILU = 1 << 0,
    FFN_IG_OUT_F32 = 1 << 1,
    FFN_IG_GEGLU = 1 << 2,         /* N = 2*Nout; 16-column blocks alternate hidden/gate; out = hidden * gelu(gate) */
    FFN_IG_OUT_TRANSPOSED = 1 << 3, /* out[b][n][s], row stride ldo, m = b*rows_per_batch + s (V^T for ffn_attn) */
    FFN_IG_OUT_PAIR = 1 << 4,       /* FFN_BF16X3 only: out is the bf16 PAIR form [M][ldo] of rows of C = ldo/2 columns (layout: FFN_BF16X3 below) -- the A
                                       operand of the next FFN_BF16X3 GEMM (the GEGLU projection feeding ff.net.2; round 6: ff.net.2 + residual feeding proj_out -- bias, row
                                       bias and the fp32 residual are added before the split; out must not alias the residual) */
    FFN_IG_OUT_GELU = 1 << 5,       /* out = gelu_erf(acc + bias) (+ residual): the MLP of the DINOv2 blocks (dinov2/layers/mlp.py:31-38) */
    FFN_IG_OUT_KV64 = 1 << 7,       /* FFN_BF16X3 only (round 6): the projection writes the attention kernels' PRE-SPLIT K / V^T images itself (what ffn_attn_presplit
                                       produces from an fp32 K / V^T: one fp32 round trip and one HBM-bound pass less per self-attention block).  Row-major output:
                                       columns c >= kv64_from of a row are stored, per 64 columns (one head), as [hi(64) | lo(64)] bf16 in the bytes their fp32 values
                                       would occupy (columns below kv64_from stay fp32: the q half of the fused q | k projection; kv64_from and N %% 64 == 0).
                                       FFN_IG_OUT_TRANSPOSED: every run of 64 consecutive positions s of a row out[b][n][.] is stored as [hi(64) | lo(64)]
                                       (rows_per_batch %% 64 == 0).  Plain epilogue only (bias allowed), no split-K.  ffn_attn reads them with kv_pair = 1. */
    FFN_IG_OUT_RELU = 1 << 6,       /* out = max(acc + bias, 0) (+ residual): the DPT head's ResidualConvUnit / output convs (depth_anything/blocks.py:68-78,
                                       dpt.py:93-98).  SILU / GELU / QGELU / RELU are mutually exclusive and exclude GEGLU and the transposed output */
    FFN_IG_OUT_QGELU = 1 << 8       /* out = y * sigmoid(1.702 y), y = acc + bias (+ residual after it): the "quick_gelu" of CLIP ViT-L's MLP (SD-1.x text tower; transformers
                                       activations.py QuickGELUActivation).  Same rules as FFN_IG_OUT_GELU, all three dtypes; runs on the generic tiles (the ping-pong
                                       tiles' epilogue does not carry it) */
};
/* Strides and alignment of ffn_igemm_desc: what each kernel family relies on, and what ffn_igemm therefore checks before any launch (FFN_EINVAL).
 * Every operand may be a column view of a wider buffer: only the row strides below and the base pointers enter the addressing.
 *   A, W    every family stages 16-byte chunks (4 fp32 / 8 bf16 / 16 e4m3) straight into LDS: A, W 16-byte aligned, lda, Kpad (split-bf16: a_lo too)
 *           multiples of the chunk, lda >= K (dense; pair forms: lda >= 2K blocked, a_lo >= K and a_lo + K <= lda planes), Kpad >= K (2K / 3K).
 *           Chunks are whole inside K or whole outside it (K a multiple of the chunk): columns [K, lda) of A and [K, Kpad) of W are never read.
 *           3x3 / 2x2 convolutions gather pixels of Cin (split-bf16: lda) elements from a dense NHWC tensor: there is no pixel stride outside split-bf16.
 *   out     four columns per lane.  igemm_glds_kernel, igemm_halo_kernel and igemm_splitk_reduce_kernel (igemm.h) store them as ONE naturally aligned
 *           access: 8 bytes of bf16, 16 bytes of fp32 (also FFN_IG_OUT_F32, the pair form: two 8-byte halves, the transposed form with
 *           rows_per_batch % 4 == 0; other transposed outputs go element by element) -- out 16-byte aligned, N % 4 == 0, ldo % 4 == 0 suffice.
 *           igemm_pp_kernel (igemm_p8.h) stores through a buffer resource over [out, out + M * ldo): bf16 rows leave as 16-byte pieces of two
 *           neighbouring fragments (and one 8-byte piece where the fragment count is odd), fp32 rows as 16-byte pieces, at byte offsets that are
 *           multiples of 8 (bf16) / 16 (fp32) from a row start.  With ldo % 8 == 4 in bf16 the row starts, and so the 16-byte pieces, are only 8-byte
 *           aligned: global (buffer) stores of gfx950 need 4-byte alignment, so this is slower, not wrong -- no family is kept off such descriptors.
 *           Rows >= M fall outside the resource and are dropped; N is whole tiles, so no column >= N is ever addressed.
 *           ldo >= the columns written: N (GEGLU: N / 2; pair form: ldo / 2 >= them; transposed: min(rows_per_batch, M)).
 *   residual  read like out is written: 8 bytes of bf16 (FFN_BF16, FFN_FP8) or 16 bytes of fp32 (FFN_F32, FFN_BF16X3) per lane, by plain loads (igemm.h)
 *           or through a buffer resource over [residual, residual + M * ldr) (igemm_p8.h): residual 8- resp. 16-byte aligned, ldr % 4 == 0, ldr >= N.
 *   split-K slabs (ws): dense fp32 [splitk][M][N], 16-byte accesses: ws 16-byte aligned. */
typedef struct ffn_igemm_desc {
    const void* A;        /* dense: [M][lda];  conv: NHWC input [B][Hin][Win][Cin] */
    const void* W;        /* [N][Kpad] */
    void* out;            /* [M][ldo] (or transposed) */
    const float* bias;    /* [N] or NULL (GEGLU: packed like W rows) */
    const float* rowbias; /* [batch][ldrb] or NULL; batch = m / rows_per_batch (time-embedding projection) */
    const void* residual; /* [M][ldr] or NULL */
    int M, N, K, Kpad;
    int lda, ldo, ldr, ldrb;
    int rows_per_batch;
    int Hin, Win, Cin, Hout, Wout, stride, pad, upsample; /* conv only; upsample=1 fuses nearest-2x of the input */
    int flags;
    float alpha;
    int conv; /* 0 = dense, 1 = 3x3 conv, 2 = 2x2 conv: taps (dy, dx) in {0,1}^2 read input pixel (yo - (pad >> 1) + dy, xo - (pad & 1) + dx),
                 K = 4 Cin, stride 1 -- one sub-pixel class of a 3x3 conv behind a nearest-2x upsample (output pixel (2y+a, 2x+b) sees a 2x2
                 window of the low-resolution input, pad = 2 (1 - a) + (1 - b), with the 3x3 taps that coincide summed: 4/9 of the FLOPs);
                 bf16 ping-pong tiles only (Cin % 64 == 0, N % 256 or % 320 == 0, M >= 192) */
    int splitk;       /* 0 = let the library choose (needs ws), 1 = never split, k = force k K-slices */
    void* ws;         /* optional fp32 scratch for split-K partial slabs (>= splitk*M*N*4 bytes) or NULL */
    long ws_bytes;
    int a_lo;         /* FFN_BF16X3: x3 = 0 / 1: column (conv: channel) offset of the lo plane inside a row (pixel) of A; x3 = 2: 32 (the block); else ignored */
    int x3;           /* FFN_BF16X3: operand layout -- 0 / 1 = planes (A [hi(K) | lo(K)], W [W_hi | W_lo | W_hi] over the whole K, conv: per tap);
                         2 = blocked: A and W as 128-byte blocks [hi(32) | lo(32)] per 32 elements of K (needs K, conv: Cin, % 32 == 0; what the
                         ping-pong tile's split-bf16 core streams) */
    int f8;           /* set by the library from `dtype` (callers leave it 0) */
    int kv64_from;    /* FFN_IG_OUT_KV64, row-major output: first column written in the pre-split form (0 = the whole row) */
} ffn_igemm_desc;
int ffn_igemm(void* stream, int dtype, const ffn_igemm_desc* d);
/* FFN_BF16X3 ("split-bf16", the fast mode that keeps fp32-level results): every fp32 operand value v is carried as hi = bf16(v) and
 * lo = bf16(v - hi) (16-17 significant bits together) and a product a*w is evaluated as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on the bf16
 * MFMA with fp32 accumulation -- 3 MFMAs per product term (ceiling 2.5 PFLOP/s / 3 = 833 TFLOP/s against 157 TFLOP/s of the fp32
 * MFMA), dropped term a_lo*w_lo ~ 2^-18.  Operand formats:
 *   the PAIR form of a row (pixel) of C fp32 values = 2C bf16.  C % 32 == 0: BLOCKED -- every 32 columns are one 128-byte block
 *        [hi(32) | lo(32)] (column c: hi at element 64 (c / 32) + c % 32, lo 32 elements behind it), so that a 32-deep K stage of a GEMM is
 *        ONE whole line carrying both planes (round 5; rounds 3-4 kept two planes and streamed the hi plane twice).  Otherwise one block of C
 *        columns, i.e. the planes [hi(C) | lo(C)].  ffn_split_pair, the *_pair norms, FFN_IG_OUT_PAIR and ffn_attn's out_pair all write it;
 *   A    pair rows of K columns (conv: pixels of Cin channels), lda = row (pixel) stride in bf16 elements.  desc.x3 = 2 (blocked, K resp.
 *        Cin % 32 == 0): a_lo = 32.  desc.x3 = 0 / 1 (planes): lo plane at columns [a_lo, a_lo + K);
 *   W    bf16 [N][Kpad].  x3 = 2: the pair form of each fp32 weight row, conv: of each tap's Cin columns (Kpad >= 2K; column
 *        k' = (tap*Cin/32 + block)*64 + {0, 32} + e).  x3 = 0 / 1: Kpad >= 3K, [W_hi | W_lo | W_hi] (conv: per tap, k' = (tap*3 + seg)*Cin + ci);
 *   out, residual   fp32 (FFN_IG_OUT_F32 is implied); bias / rowbias fp32 as always; GEGLU, SILU, transposed output, split-K as in bf16.
 * K in the descriptor is the REAL contraction length (dense K, conv 9*Cin). */
int ffn_split_pair(void* stream, const float* src, void* dst, long rows, int C, int ld_src);
/* 3x3 / stride 1 / pad 1 convolution with FOUR output channels (the UNet's conv_out): x NHWC [B][H*W][Cin] (FFN_F32 or FFN_BF16 elements), w fp32
 * [4][9][Cin] ((ky, kx, ci) order), bias fp32 [4] or NULL, out fp32 [B][H*W][4].  Direct fp32 convolution on the vector ALU (exact fp32 products in
 * every mode) instead of 1/32 of an MFMA tile; Cin % 16 == 0, Cin <= 448 (weights in LDS). */
int ffn_conv3x3_n4(void* stream, int dtype, const void* x, const float* w, const float* bias, float* out, int B, int H, int W, int Cin);
/* FFN_FP8 (3x3 convolutions of the bf16 fast mode, reported beside it -- not a parity mode): A = e4m3 bytes NHWC [B][Hin][Win][Cin] with
 * Cin a multiple of 16 (the ping-pong tile: of 128; ffn_groupnorm_f8 writes such a tensor, channels zero-padded), W = e4m3 [N][Kpad]
 * in the usual (ky, kx, ci) order, K = 9 * Cin; out / residual bf16, bias / rowbias fp32.  Both operands carry power-of-two scales (the
 * activation's is ffn_groupnorm_f8's `qscale`, the weight's is chosen at pack time); `alpha` = 1 / (their product) un-scales the result.
 * The kernels are the bf16 ones: e4m3 rides the same 16-byte chunk geometry (16 values per chunk, 128 per K row), each fragment pair
 * takes two v_mfma_f32_16x16x32_fp8_fp8 -- twice the contraction per staged byte at the bf16 MFMA rate. */
int ffn_groupnorm_f8(void* stream, const void* x_bf16, void* y_e4m3, const float* gamma, const float* beta, int B, int HW, int C, int Cp,
                     int G, float eps, int silu, float qscale, float* partial_ws, float* scale, float* shift);
/* Kernel families behind ffn_igemm (freefine_amd/csrc): igemm_pp_kernel (igemm_p8.h; bf16 -- 256- or 192-row "ping-pong" tiles with
 * LDS-DMA operands in flight across barriers, the default wherever N is a multiple of 256 or 320 and K a multiple of 64),
 * igemm_glds_kernel / igemm_halo_kernel (igemm.h; every other bf16 shape and all of f32).
 * bf16 problems: the first time a problem shape is seen outside stream capture, ffn_igemm times its few plausible (tile, K-split)
 * configurations on the caller's stream (this one call synchronises the stream and launches the kernel several times: `out` must
 * not alias `residual`) and caches the winner; FFN_IGEMM_TUNE=0 in the environment keeps the deterministic rule-based choice
 * (f32 and transposed outputs always use it); no other environment variable changes which kernel runs.  Testing hooks: the number of bf16
 * configurations, and forcing one wherever it is a candidate for the problem (-1 = off; returns the previous value). */
/* explicit warm-up entry point: tunes (or looks up) the configuration for `d` now, exactly as the first ffn_igemm call would --
 * it IS a full ffn_igemm call: `out` is written (several times while candidates are timed) and holds the winner's result */
int ffn_igemm_tune(void* stream, int dtype, const ffn_igemm_desc* d);
/* the tuned table as data: entries of ffn_igemm_tune_entry_ints() ints (problem key, configuration, K split).  export returns the
 * number of entries in the table (copies at most max_entries); import merges entries (unknown configurations are skipped) and returns
 * how many it took.  Use: persist the table across processes, or broadcast rank 0's table in a multi-GPU run so that every rank
 * launches identical configurations. */
int ffn_igemm_tune_entry_ints(void);
int ffn_igemm_tune_export(int* buf, int max_entries);
int ffn_igemm_tune_import(const int* buf, int n_entries);
/* Entries carry a stamp of the build that wrote them (table layout, configuration list, gfx950): import ignores foreign ones, and
 * an imported entry is launched only after its (configuration, K split) was found among the candidates THIS build offers for the
 * actual problem (workspace capacity, split legality, tile applicability); otherwise it is dropped and the problem re-tuned.
 * ffn_igemm_tune_clear empties the table (returns the number of entries dropped); ffn_igemm_tune_enable(0) stops timing-based
 * tuning in this process -- problems not in the table then take the deterministic rule (returns the previous setting).  A sharded
 * run wanting bit-identical bf16 results on every rank: clear + import rank 0's table, then ffn_igemm_tune_enable(0). */
int ffn_igemm_tune_clear(void);
int ffn_igemm_tune_enable(int on);
int ffn_igemm_tune_stamp(void);   /* first int of every entry this build exports */
int ffn_igemm_num_configs(void);
int ffn_igemm_force_config(int cfg);
/* the kernel instantiation ffn_igemm launches for this problem, spelled like rocprofv3's kernel trace: the same choice as ffn_igemm's, without
 * timing (a forced configuration, else the table's entry, else the rule-based one).  Nothing is launched and no buffer is looked at; a descriptor
 * whose shape or flags ffn_igemm refuses gets the same error code and message. */
int ffn_igemm_kernel_name(int dtype, const ffn_igemm_desc* d, char* buf, int len);

/* ---- multi-pass masked attention (the FreeFine attention modulation) -----------------------------------------
 * out[b,q,h,:] = sum_p w_p(b) * wq_p[q] * softmax_k(scale*<Q[qrow_p(b),q,h],K[kvrow_p(b),k,h]> + mask_p(q,k)) V[kvrow_p(b),k,h]
 * Replaces: Attention_Modulator.Temporal_contextal_attention{,_bg,_compose}, modulate_local_cross_attn{,_bg,_compose},
 * style_align_share_attention, mask_attention, get_attention_scores, get_cross_hidden_state and the prepare_*_mask
 * builders (src/utils/attention.py:774-1432) plus the plain branch of ca_forward (attention.py:394-404). */
#define FFN_ATT_MAXP 4
#define FFN_ATT_MAXB 16
enum { FFN_ATT_HEAD_RULE = 1, FFN_ATT_UNIFORM_SEL1 = 2, FFN_ATT_UNIFORM_SEL0 = 4,
       FFN_ATT_CAUSAL = 8 /* key k is allowed for query q iff k <= q (the CLIP text tower's self attention).  Accepted when S == Sk <= 96, D == 64, npass == 1,
                             kv_pair == 0, scale > 0 and every active entry carries the flag and has no kmask / qsel / wq / w_slope; any other descriptor with the
                             flag set returns FFN_EINVAL and launches nothing.  Runs attn_causal_kernel (attention_causal.h) in all three dtypes; out_pair as usual */ };
typedef struct ffn_attn_entry {
    int q_row, kv_row;      /* batch rows supplying Q and K/V for this (pass, output row) */
    float w_const, w_slope; /* weight = w_const + w_slope * (*w_dev); both 0 -> entry skipped */
    const float* wq;        /* per-query weight [S] or NULL */
    const uint8_t* kmask;   /* per-key byte mask [Sk] or NULL */
    const uint8_t* qsel;    /* per-query selector [S] or NULL (=1): allowed(q,k) = (kmask[k]!=0) == (qsel[q]!=0) */
    int flags;              /* FFN_ATT_HEAD_RULE: mask applies only where (b*heads+head) is even (attention.py:859 vs 761);
                               FFN_ATT_UNIFORM_SEL1/0: the allowed set for sel=1/0 is empty -> uniform over all keys;
                               FFN_ATT_CAUSAL: see above */
    int hr_row;             /* 0: the tiled-head rule uses the OUTPUT row index; k>0: it uses row k-1 (row-deduplicated batches) */
} ffn_attn_entry;
typedef struct ffn_attn_desc {
    const void* q;      /* [Bq][S][ldq], head h at column h*D */
    const void* k;      /* [Bk][Sk][ldk] */
    const void* vt;     /* [Bk][heads*D][ldvt]  V transposed (ldvt >= Sk, multiple of 8, padding finite) */
    void* out;          /* [Bo][S][ldo] */
    const float* w_dev; /* device scalar (context_guidance) or NULL */
    int Bo, S, Sk, heads, D;
    int ldq, ldk, ldvt, ldo;
    float scale;
    int npass;
    int out_pair;       /* FFN_BF16X3 with D <= 64 only: out is the bf16 PAIR form [Bo][S][ldo] of rows of ldo/2 columns (layout: FFN_BF16X3 above), the A operand of
                           the to_out projection's FFN_BF16X3 GEMM; 0 = fp32 rows */
    int kv_pair;        /* 1: k / vt are the PRE-SPLIT bf16 images ffn_attn_presplit (or a projection with FFN_IG_OUT_KV64) wrote: k[row][key] = heads blocks
                           of [hi(64) | lo(64)], ldk * 4 bytes from key to key; vt[row][head * 64 + d] = Sk / 64 blocks of [hi(64 keys) | lo(64 keys)], ldvt * 4
                           bytes from row to row (i.e. ldk / ldvt are what they would be for the fp32 tensors the images replace: heads * 64 / Sk when compact).
                           Only for launches whose kernel reads the images: attn_x3w_kernel (attention_x3w.h: one wave per SIMD on 32x32x16 MFMAs), i.e.
                           FFN_BF16X3 launches that run attn_x3p_kernel with kv_pair = 0.  ffn_attn and ffn_attn_kernel_name return FFN_EINVAL for any other
                           (ask ffn_attn_kernel_name with kv_pair = 1 whether a descriptor qualifies); 0 = fp32 k / vt */
    ffn_attn_entry e[FFN_ATT_MAXP * FFN_ATT_MAXB]; /* entry (p,b) at p*FFN_ATT_MAXB + b */
} ffn_attn_desc;
int ffn_attn(void* stream, int dtype, const ffn_attn_desc* d);
/* The kernel follows from the descriptor alone (ffn_attn_kernel_name names it):
 * dtype FFN_BF16X3: q / k / vt / out are fp32 exactly as with FFN_F32; head sizes D <= 64 run attn_x3_kernel (attention_x3.h: both
 * products in split-bf16 arithmetic, three bf16 MFMAs per term, fp32 softmax) -- or, under attn_pp_kernel's preconditions (D = 64,
 * Sk % 64 == 0, S >= 128, no uniform-softmax entry), attn_x3p_kernel (attention_x3p.h: the same arithmetic in the ping-pong schedule)
 * and, on pre-split K / V^T (kv_pair), attn_x3w_kernel; short unmasked key sequences (D = 64, Sk <= 96, fragment images of all passes
 * within the LDS) run xattn_x3_kernel (attention_xx3.h); larger heads fall back to the exact fp32 kernel. */
/* bf16 launches with D = 64, Sk % 64 == 0, S >= 128 and no degenerate (uniform-softmax) entry run attn_pp_kernel (attention_pp.h:
 * software-pipelined, 8 waves in two alternating groups); everything else attn_kernel (attention.h).  Same results up to fp32
 * summation order.
 * bf16 launches with D = 64, Sk <= 96 and active entries that carry no key mask / selector (the text cross-attention) run xattn_kernel
 * (attention_x.h: K and V^T of a (row, head) in a wave's registers) for ONE pass of plain entries, else xattn_mp_kernel. */
/* fp32 K [rows][Sk][ldk] (heads * 64 columns) and V^T [rows][heads * 64][ldvt] -> the bf16 images attn_x3w_kernel stages by LDS-DMA when
 * desc.kv_pair = 1: k_pair [rows][Sk][heads][hi(64) | lo(64)], vt_pair [rows][heads * 64][Sk / 64][hi(64 keys) | lo(64 keys)] (each as many bytes
 * as its fp32 source; Sk % 64 == 0, head dim 64).  Once per attention call: the kernel's 16 query-block workgroups per (row, head) otherwise each
 * split the whole K / V^T in their key loops (16-25 % of the launch).  Reference call sites: the self-attention of the hooked Attention.forward,
 * src/utils/attention.py:394-404, 1043-1091. */
int ffn_attn_presplit(void* stream, const float* k, const float* vt, void* k_pair, void* vt_pair, int rows, int Sk, int heads, int ldk, int ldvt);
/* Descriptors whose entries carry FFN_ATT_CAUSAL run attn_causal_kernel (attention_causal.h: one workgroup per (row, head), one wave per 16 queries, key
 * fragments above the diagonal skipped) whatever the dtype; a descriptor without the flag is planned exactly as before the flag existed. */
/* padded head dim / query fragments per wave of the instantiation ffn_attn dispatches for head dim D */
int ffn_attn_variant(int dtype, int D, int* dp, int* qf);
/* the kernel instantiation ffn_attn launches for this problem, spelled like rocprofv3's kernel trace */
int ffn_attn_kernel_name(int dtype, const ffn_attn_desc* d, char* buf, int len);

/* ---- elementwise / resampling helpers of the depth front end ------------------------------------------ */
/* y = max(a, 0) (FFN_ELT_RELU, b ignored) or y = a + b (FFN_ELT_ADD) over n elements (n % 4 == 0; fp32 or bf16).  Replaces the
 * activation in front of ResidualConvUnit.conv1 and FeatureFusionBlock's skip_add (depth_anything/blocks.py:68, 137-139). */
/* FFN_ELT_GELU (ABI version 11, b ignored): y = a (1 + erf(a / sqrt 2)) / 2, erff in fp32; in bf16 the fast erf of the GEMM epilogues.  The activation behind
 * GroupNorm(1, 64) in EfficientSAM's mask upscaling (evaluation/DesignEdit/sam/efficient_sam/efficient_sam_decoder.py:186-197). */
enum { FFN_ELT_RELU = 0, FFN_ELT_ADD = 1, FFN_ELT_GELU = 2 };
int ffn_eltwise(void* stream, int dtype, int op, const void* a, const void* b, void* y, long n);
/* bilinear resampling of an NHWC tensor [B][Hin][Win][C] -> [B][Hout][Wout][C] with align_corners = True (source coordinate
 * y * (Hin - 1) / (Hout - 1), fp32 weights; Hout == 1 reads row 0): torch.nn.functional.interpolate(mode="bilinear",
 * align_corners=True) as called by depth_anything/blocks.py:147-149 and dpt.py:132, 165.  relu != 0 applies max(., 0) (dpt.py:166). */
int ffn_resize_bilinear(void* stream, int dtype, const void* x, void* y, int B, int Hin, int Win, int Hout, int Wout, int C, int relu);

/* ---- point-cloud warp of the 3-D coarse edit ------------------------------------------------------------
 * The arithmetic of IntegratedP3DTransRasterBlendingFull (src/utils/geo_utils.py:427-528): depth-lifted object pixels -> rigid transform about
 * the cloud's centre -> FoV-perspective projection -> pytorch3d-style disc splat (PointsRasterizer: the K nearest covering points per pixel,
 * AlphaCompositor with weights 1 - d^2 / r^2).  pytorch3d is absent from the build image: the restatement is PARITY UNPINNED (property-tested
 * and checked against oracle/warp3d.py).  All buffers fp32 / int32, device memory.
 *   ffn_splat_lift     pts[n][4] = (-(i - W/2) z / fx, -(j - H/2) z / fy, z, 0) for the masked pixels idx[n] = j * W + i (geo_utils.py:436-457)
 *   ffn_splat_project  proj[n][4] = (x_ndc, y_ndc, z_view, 0): view = ((p - center + translate) . rotate) * scale + center, row vectors,
 *                      ndc = view.xy / (view.z * tan_half_fov)  (geo_utils.py:343-378, 399-425, 478-481)
 *   ffn_splat_bin      tile binning (16 x 16 pixel tiles, tiles = ceil(W/16) * ceil(H/16)): fill = 0 adds to counts[tile] the number of discs
 *                      whose bounding box touches the tile; fill = 1 writes the point ids to list[offs[tile] + k] (counts = zeroed cursor,
 *                      offs = exclusive scan of the counting pass with the total at offs[tiles])
 *   ffn_splat_render   image[H][W][3] (fp32, composited colours), idx_sum[H][W] (sum of the K point ids, -1 per empty slot: what the
 *                      reference's mask test reads, geo_utils.py:517) and covered[H][W] (any point)  (geo_utils.py:482-517)
 *   ffn_splat_ids      (ABI version 10, with ffn_splat_correspond)  ids[H][W][K] (int32): the ids of the points ffn_splat_render composites at each pixel, in compositing order (depth, ties
 *                      by id), -1 per empty slot -- pytorch3d's `fragments.idx` (geo_utils.py:491), from the same selection routine as the render
 *   ffn_splat_correspond  the correspondence map of the warp (evaluation/FreeFine/get_3d_transform_correspondence.py:21-54 writes one per
 *                      case; Mean Distance reads it, evaluation/metrics/mean_distance.py:108,122): map[H][W][2] (fp32) receives, for source pixel
 *                      idx[p], the continuous target pixel (x, y) the renderer draws point p at (a point drawn on a pixel centre: that pixel's
 *                      integer coordinates); NaN in both for a point with !(z >= 0) or non-finite NDC.  Pixels idx does not name are not
 *                      touched (the host pre-fills them).  visible[H][W] (uint8; may be NULL, and then ids may be NULL too): source pixel
 *                      idx[p] gets 1 iff the point's nearest pixel (floor(y + 0.5), floor(x + 0.5)) lies inside the image and p is among
 *                      that pixel's K ids, else 0.  n = 0 is a no-op.  Both: no allocation, no sync, the caller's stream; FFN_EINVAL before
 *                      any launch on a null required pointer, n < 0, W / H <= 0 or K outside 1 .. 32 */
typedef struct ffn_splat_xform {
    float center[3], translate[3], rotate[9] /* row-major, applied as p . R */, scale[3];
    float tan_half_fov;
} ffn_splat_xform;
int ffn_splat_lift(void* stream, const float* depth, const int* idx, float* pts, int n, int W, int H, float fx, float fy);
int ffn_splat_project(void* stream, const float* pts, float* proj, int n, const ffn_splat_xform* x);
int ffn_splat_bin(void* stream, int fill, const float* proj, int n, float radius, int W, int H, int* counts, const int* offs, int* list);
int ffn_splat_render(void* stream, const float* proj, const float* rgb, const int* offs, const int* list, float radius, int K, int W, int H,
                     float* image, int* idx_sum, uint8_t* covered);
int ffn_splat_ids(void* stream, const float* proj, const int* offs, const int* list, float radius, int K, int W, int H, int* ids);
int ffn_splat_correspond(void* stream, const float* proj, const int* idx, int n, int W, int H, const int* ids, int K, float* map, uint8_t* visible);

/* ---- the GeoDiffuser warp (ABI version 13): step 2 of the reference's GeoBench-3D preparation -----------------------------------
 * evaluation/FreeFine/get_3d_transform_correspondence.py:207-289 through evaluation/GeoDiffuser/GeoDiffuser/utils (ui_utils2.py:504-593, 685-743;
 * vis_utils.py:404-479; warp_utils.py:28-176, 235-298, 304-399, 407-492, 599-645).  Square images only (the reference takes sqrt(N) for the side).
 * PINNED to the reference's code: the coordinates of ffn_geo_project and the triangle topology of ffn_mesh_cover.  NOT pinned: the two rasterisers
 * (pytorch3d's rasterize_points and rasterize_meshes, absent from the build image), which restate pytorch3d's published kernels.
 *   ffn_geo_project    every pixel (i, j) of the S x S image: cam = K^-1 (j, i, 1) depth[i][j] with K = (f, f, S/2, S/2); p = pose[:, :3] cam + pose[:, 3]
 *                      (pose: 12 floats in HOST memory, 3 x 4 row-major); (X, Y, Z') = K p; Z = max(Z', 1e-3); tcoords[S][S][3] = (2 (X / Z) / (S - 1) - 1,
 *                      2 (Y / Z) / (S - 1) - 1, Z), the reference's t_coords, whose first two channels are the correspondence map; proj[S*S][4] =
 *                      (-X_norm, -Y_norm, Z, 0), the same point as ffn_splat_bin / ffn_splat_ids read it (warp_utils.py:90-91).  depth is already
 *                      normalised (vis_utils.py:410-423) by the caller.
 *   ffn_splat_composite  out[S][S][C] (fp32) from feat[n][C] over the tile lists of ffn_splat_bin (n = S*S points, radius in NDC units = radius_px / S * 2):
 *                      the selection of ffn_splat_render (the K nearest by z among the points with d^2 < r^2, ties by point id, points with z < 0
 *                      dropped -- pytorch3d leaves the order of equal z unpinned), alpha = (1 - sqrt(clamp(d^2 / r^2, 1e-3, 1)))^tau, front-to-back
 *                      alpha_composite; round_half != 0 rounds the result once through fp16 (the reference returns `.to(torch.half)`).
 *   ffn_mesh_cover     cover[S][S] (uint8; the caller zeroes it, the kernel only ever stores 1): the pixel centre lies strictly inside (all three
 *                      barycentric coordinates > 0) a projected triangle of the mask's mesh: per 2 x 2 pixel quad the triangles (tl, tr, bl) and
 *                      (bl, tr, br) of create_triangles, each present when its own three vertices have mask != 0; vertices = tcoords.  Faces of
 *                      |area| <= 1e-8 or entirely behind z = 0 are skipped; no back-face culling (rasterize_meshes at blur radius ~ 0).
 * All three: no allocation, no sync, the caller's stream; FFN_EINVAL before any launch on a null pointer, H != W, a side beyond 4096, C outside 1 .. 8,
 * K outside 1 .. 32, radius, tau or focal <= 0. */
int ffn_geo_project(void* stream, const float* depth, const float* pose, float focal, int H, int W, float* tcoords, float* proj);
int ffn_splat_composite(void* stream, const float* proj, const float* feat, const int* offs, const int* list, float radius, float tau, int K,
                        int C, int H, int W, int round_half, float* out);
int ffn_mesh_cover(void* stream, const float* tcoords, const uint8_t* mask, int H, int W, uint8_t* cover);

/* ---- normalisation ------------------------------------------------------------------------------------------- */
/* `silu` of ffn_groupnorm / ffn_gn_apply is a flag word: FFN_NORM_SILU applies SiLU; FFN_NORM_OUT_PAIR (fp32 input only) writes y as the
 * bf16 PAIR rows [B*HW][2C] an FFN_BF16X3 GEMM reads (layout: FFN_BF16X3 above; no separate ffn_split_pair pass).  ffn_layernorm_pair: the same for LayerNorm. */
enum { FFN_NORM_SILU = 1, FFN_NORM_OUT_PAIR = 2 };
/* GroupNorm statistics -> per-(batch,channel) scale/shift (fp32).  partial_ws: >= B*nchunk*2*C floats where
 * nchunk = ffn_gn_nchunk(HW).  Replaces torch GroupNorm inside diffusers blocks (attention.py:105-214). */
int ffn_gn_nchunk(int HW);
/* 1 if ffn_groupnorm handles this problem in one fused launch (no workspace needed), 0 if it needs the partial / scale / shift workspace */
int ffn_gn_fused(int B, int HW, int C, int G);
int ffn_gn_stats(void* stream, int dtype, const void* x, const float* gamma, const float* beta, int B, int HW, int C, int G,
                 float eps, float* partial_ws, float* scale, float* shift);
int ffn_gn_apply(void* stream, int dtype, const void* x, void* y, const float* scale, const float* shift, int B, int HW,
                 int C, int silu);
/* GroupNorm (+ optional SiLU) in one call: a single fused launch when a (batch, group) slice has <= 131072 elements (every UNet
 * GroupNorm at 64x64 latents), else ffn_gn_stats + ffn_gn_apply (workspace pointers may be NULL in the fused case). */
int ffn_groupnorm(void* stream, int dtype, const void* x, void* y, const float* gamma, const float* beta, int B, int HW, int C, int G,
                  float eps, int silu, float* partial_ws, float* scale, float* shift);
/* round 6: GroupNorm (three-launch form, fp32 x) whose apply pass writes BOTH pair tensors a ResBlock with a 1x1 shortcut reads: y = pair(act(GN(x))) for conv1
 * and yraw = pair(x) for the shortcut GEMM (what ffn_split_pair(x) would produce, bit for bit) -- x is read once less.  C % 8 == 0; the workspace is required
 * (also for shapes ffn_gn_fused() would take in one launch); `silu`: FFN_NORM_SILU or 0.  Reference: the norm1 / conv_shortcut inputs of diffusers' ResnetBlock2D
 * (in-tree copy /root/reference/evaluation/DragonDiffusion/src/unet/resnet_2d.py:110). */
int ffn_groupnorm_pair_raw(void* stream, const void* x, void* y_pair, void* yraw_pair, const float* gamma, const float* beta, int B, int HW, int C, int G,
                           float eps, int silu, float* partial_ws, float* scale, float* shift);
int ffn_layernorm(void* stream, int dtype, const void* x, void* y, const float* gamma, const float* beta, int M, int C,
                  float eps);
int ffn_layernorm_pair(void* stream, const float* x, void* y, const float* gamma, const float* beta, int M, int C, float eps);
int ffn_softmax_rows(void* stream, int dtype, const void* x, void* y, long M, int N, float scale);
/* ABI version 8.  LayerNorm of ONE row per sequence of x [N][S][C] (activation type of `dtype`: FFN_F32 / FFN_BF16) -> y [N][C] in the same type, or
 * (pair = 1, FFN_F32 only) the pair rows [N][2C] of ffn_layernorm_pair.  ids == NULL: row 0 of every sequence (the class token of a ViT); otherwise ids int32
 * [N][S] in device memory, S <= 96, and the row is the FIRST position holding the sequence's largest id (open_clip's text pooling: end-of-text has the largest
 * id).  The statistics and the affine step are ffn_layernorm's routine: bit-identical to ffn_layernorm on the gathered rows.  C as ffn_layernorm (a multiple of
 * 4 fp32 / 8 bf16 values, at most 384 16-byte chunks); x, y 16-byte aligned.  Anything else: FFN_EINVAL before any launch. */
int ffn_pool_layernorm(void* stream, int dtype, const void* x, const int* ids, void* y, const float* gamma, const float* beta, int N, int S, int C, float eps,
                       int pair);
/* ABI version 8.  out[i] = <a_i, b_j> / (max(|a_i|, 1e-12) max(|b_j|, 1e-12)), a fp32 [B][P], b fp32 [b_rows][P] with b_rows = B (j = i) or 1 (j = 0): the
 * cosine of torch.nn.functional.normalize'd rows (the Human Preference Score: evaluation/metrics/human_preference_score.py).  Three fp32 sums per row, summed
 * in a fixed order: deterministic.  P % 4 == 0; a, b 16-byte aligned. */
int ffn_cosine_rows(void* stream, const float* a, const float* b, float* out, int B, int P, int b_rows);

/* ---- scheduler / guidance elementwise (fp32, NCHW like the reference) ------------------------------------------ */
/* eps = eu + cfg*(ec-eu)*mask   (src/demo/model.py:605-611; mask NULL -> :608) */
int ffn_cfg_masked(void* stream, const float* eps_u, const float* eps_c, const float* mask, float cfg, float* eps, long n,
                   int HW);
/* inv_step (src/demo/model.py:109-132); coefficients are the fp32 values torch computes: c_bt=sqrt(1-a_t),
 * c_at=sqrt(a_t), c_an=sqrt(a_next), c_bn=sqrt(1-a_next) */
int ffn_ddim_inv_step(void* stream, const float* eps, const float* x, float c_bt, float c_at, float c_an, float c_bn,
                      float* x_next, float* pred_x0, long n);
/* ctrl_step (src/demo/model.py:134-198) */
typedef struct ffn_ctrl_step_desc {
    const float* eps;
    const float* x;
    const float* noise; /* NULL when eta == 0 */
    const float* m;     /* float(mask) [HW] */
    const float* om;    /* float(1 - mask) evaluated in the mask's own dtype (uint8 wrap kept) [HW] */
    float* x_prev;
    float* pred_x0; /* may be NULL */
    float c_bt, c_at, c_ap, c_dir;
    float c_dirm[8], stdv[8];
    int row_masked[8];
    int rows, CHW, HW;
} ffn_ctrl_step_desc;
int ffn_ddim_ctrl_step(void* stream, const ffn_ctrl_step_desc* d);

/* ---- layout / misc ----------------------------------------------------------------------------------------------- */
typedef struct ffn_pack_desc {
    const float* src; /* fp32 NCHW [Bsrc][Cl][HW] */
    void* dst;        /* T NHWC [B][HW][CP], channels >= Cl zero */
    int src_row[16];
    int B, Cl, CP, HW;
} ffn_pack_desc;
int ffn_pack_nchw(void* stream, int dtype, const ffn_pack_desc* d);
int ffn_nhwc_to_nchw_f32(void* stream, const float* src, float* dst, int B, int HW, int C, int ld);
/* out[r][0:C1] = a[r], out[r][C1:C1+C2] = b[r].  a == NULL: the left block is already in place (its producer wrote it with
 * ldo = C1 + C2), only b is copied */
int ffn_concat(void* stream, int dtype, const void* a, const void* b, void* out, long rows, int C1, int C2);
int ffn_timestep_embed(void* stream, int dtype, const float* t_dev, const float* freq, void* out, int B, int half, int flip);
int ffn_transpose(void* stream, int dtype, const void* src, void* dst, int B, int R, int C, int ld_src, int ld_dst);
int ffn_cast(void* stream, int src_dtype, int dst_dtype, const void* src, void* dst, long n);
/* Token + position embedding lookup of the CLIP text tower (transformers CLIPTextEmbeddings, reached from the reference's self.text_encoder(ids)[0],
 * src/demo/model.py:536-567): out[m][:] = table[ids[m]][:] + pos[m % S][:], m < M, added in fp32 and stored in the activation type of `dtype` (FFN_F32 and
 * FFN_BF16X3: fp32 rows -- a LayerNorm follows, no pair rows; FFN_BF16: bf16 rows).  ids int32 [M] in device memory, 0 <= id < V (the CALLER checks that on
 * the host before upload; the kernel reads no table row outside [0, V)); table fp32 [V][C], pos fp32 [S][C], C % 4 == 0. */
int ffn_embed_tokens(void* stream, int dtype, const int* ids, const float* table, const float* pos, void* out, long M, int S, int C, int V);
/* ABI version 15.  BERT's embedding (transformers BlipTextEmbeddings, the text encoder of the ImageReward score): out[m][:] = LayerNorm(table[ids[m]][:] +
 * pos[m % S][:]; gamma, beta, eps).  Arguments and checks as ffn_embed_tokens.  The sum is taken in fp32 and normalised by the routine of ffn_layernorm
 * (csrc/layernorm_row.h); out is fp32 (FFN_F32: bit-identical to ffn_layernorm(ffn_embed_tokens(..., FFN_F32))) or bf16 (FFN_BF16: the same fp32 values rounded
 * once).  C as ffn_layernorm: a multiple of 4 (fp32) / 8 (bf16), at most 1536.  A row whose sum is constant has variance 0 and gives beta, finite at any
 * eps > 0.  Anything else: FFN_EINVAL before any launch. */
int ffn_embed_tokens_ln(void* stream, int dtype, const int* ids, const float* table, const float* pos, void* out, const float* gamma, const float* beta, long M,
                        int S, int C, int V, float eps);
/* ABI version 15.  A chain of L affine layers with nothing between them, then a shift and a scale (ImageReward's reward head):
 *   a_0 = x[b][0 : dims[0]] (row b starts at x + b * ldx: ldx = S * C reads row 0 of every [S][C] sequence without a gather);  a_l = W_l a_{l-1} + b_l;
 *   out[b][0 : dims[L]] = (a_L - shift) / scale.
 * x, out and params fp32; params holds W_1 [dims[1]][dims[0]], b_1 [dims[1]], W_2 [dims[2]][dims[1]], b_2 ... back to back; dims: HOST int32 [L + 1], read
 * before the call returns.  1 <= L <= FFN_CHAIN_MAXL, 1 <= dims[l] <= FFN_CHAIN_MAXW, no width needs to be a multiple of anything; ldx >= dims[0]; scale != 0.
 * One workgroup per row; every output value is one sum over k in an order that depends on neither B nor the row: deterministic, equal rows give equal bits.
 * Anything else: FFN_EINVAL before any launch. */
#define FFN_CHAIN_MAXL 8
#define FFN_CHAIN_MAXW 1024
int ffn_affine_chain(void* stream, const float* x, const float* params, float* out, int B, int ldx, const int* dims, int L, float shift, float scale);
int ffn_image_to_nhwc(void* stream, int dtype, const uint8_t* img, void* dst, long npix, int CP);
int ffn_nhwc_to_image(void* stream, int dtype, const void* src, float* dst, int B, int HW, int ld);

/* ---- DIFT correspondence search of the Mean Distance metric --------------------------------------------------------------------------
 * Reference: evaluation/metrics/MD/mean_distance.py:139-165 -- both DIFT feature maps upsampled bilinearly to the image size (F.interpolate), then per keypoint
 * the argmax over all pixels of CosineSimilarity(dim=1) between the source feature at the keypoint and the edited image's features.  Here the upsampled maps are
 * never formed (csrc/dift_match.h: bilinear interpolation is linear, so every cosine is a few FMAs over low-resolution dot products).
 * src / tgt: the activation rows [E][h*w][ld] (first C columns used, ld >= C; `es` elements between ensemble members) of the source and the edited image, fp32
 * (FFN_F32) or bf16 (FFN_BF16); the ensemble mean over E is taken in fp32.  kps: HOST int32 [K][2] = (row, col) in [0, H) x [0, W), read before the call returns
 * (they travel as kernel arguments).  out_rc: device int32 [K][2] = (row, col) of the match, numpy's argmax rule (lowest flat index row * W + col among equal
 * cosines; NaN never wins); out_cos: device float [K], the cosine there, cos = dot / (max(|q|, 1e-8) * max(|f|, 1e-8)).  Deterministic: no atomics.
 * ws: ffn_dift_workspace_bytes(C, h, w, K) bytes of 16-byte aligned device scratch.  C % 4 == 0; ld, es multiples of the 16-byte chunk (4 fp32 / 8 bf16);
 * H * W < 2^31.  Any K (the library loops over groups of keypoints). */
typedef struct ffn_dift_desc {
    const void* src;
    const void* tgt;
    const int* kps;
    void* ws;
    int* out_rc;
    float* out_cos;
    long ws_bytes;
    long es;
    int dtype, E, C, ld, h, w, H, W, K;
} ffn_dift_desc;
int ffn_dift_match(void* stream, const ffn_dift_desc* d);
long ffn_dift_workspace_bytes(int C, int h, int w, int K);

/* ---- SIFT keypoints, descriptors and ratio-test matching of the Mean Distance metric (ABI version 12; csrc/sift.h) ----------------------------
 * Reference: evaluation/metrics/MD/mean_distance.py:49-79 takes MD's keypoints from cv2.SIFT_create().detectAndCompute and cv2.BFMatcher().knnMatch.  These
 * entries restate Lowe's SIFT with OpenCV's default parameters, one entry per stage; they are held to the fp64 restatement tests/sift_ref.py, NOT to cv2's output
 * (cv2 exists nowhere this is built: parity with its bytes is unmeasured).  freefine_amd/sift.py strings them together.  Images are contiguous; every octave side
 * is at most FFN_SIFT_MAX_SIDE.  Anything outside the stated limits is refused with FFN_EINVAL before any launch.  All on the caller's stream, no allocation;
 * only ffn_sift_extrema synchronises (it returns a count).
 *
 *   ffn_sift_base         img uint8 [H][W][C], C = 3 or 1 -> out fp32 [2H][2W].  gray = (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14 (OpenCV's 8-bit BGR2GRAY
 *                         applied to the array as given: the reference passes RGB, so channel 0 gets B's weight; C = 1 is taken as gray), then 2x bilinear upsampling
 *                         (source coordinate (d + 0.5) / 2 - 0.5, clamped).  Exact in fp32.
 *   ffn_gauss_blur_f32    separable blur of src [H][W] into dst (dst may be src; tmp [H][W] is a third buffer).  taps: HOST float [T], T odd <= FFN_SIFT_MAX_TAPS,
 *                         read before the call returns.  Per pass out(p) = sum over k ascending of taps[k] * in(reflect101(p + k - T / 2)), each product rounded,
 *                         then added (no FMA); horizontal pass first.
 *   ffn_decimate2_f32     dst [H / 2][W / 2] = src(2 y, 2 x): the first image of the next octave.
 *   ffn_sift_extrema      gauss [6][h][w] -> dog [5][h][w] = gauss[i + 1] - gauss[i], and the list cand int32 [cap][3] = (layer, row, col) of the 26-neighbour extrema
 *                         of dog layers 1..3 (ties allowed: >= / <=), |value| > 1, 5-pixel border, in no particular order.  counter: one device int (scratch);
 *                         *count (host): how many were found.  More than cap: FFN_ENOSPC, the list holds cap of them -- never a silently short list.  An octave
 *                         with a side below 11 pixels has no candidates.
 *   ffn_sift_refine_orient  per candidate: up to 5 steps of the 3-D quadratic fit (image scale 1 / 255, central differences, Cramer's rule), contrast test
 *                         |D + grad . x / 2| * 3 >= 0.04, edge test det > 0 and tr^2 * 10 < 121 det, 36-bin orientation histogram on the Gaussian layer (radius
 *                         round(4.5 s), weight sigma 1.5 s), [1 4 6 4 1] / 16 smoothing, one angle per local peak >= 0.8 max (parabola).  octave: 0 = the
 *                         upsampled base.  out fp32 [n][27] = (keep, layer, row, col, x, y, size, response, npeaks, 18 angles in degrees), x / y / size in INPUT-image
 *                         pixels; a rejected candidate's record is all zero.
 *   ffn_sift_describe     kp fp32 [n][7] = (x, y, size, angle, response, octave - 1, layer), all of octave `octave` -> desc uint8 [n][128] (4 x 4 x 8, trilinear
 *                         binning, histogram width 3 s, Gaussian weight exp(-(r^2 + c^2) / 8) in bin units, L2-normalise, clip at 0.2, renormalise to 512, saturate);
 *                         raw (may be null) fp32 [n][128]: the values before the conversion to uint8.
 *   ffn_knn2_u8           for every row of des1 [n1][128] the two nearest rows of des2 [n2][128] by squared L2 distance in int32, ties to the lower index:
 *                         idx int32 [n1][2], dist int32 [n1][2]; a missing neighbour (n2 < 2) is index -1 at distance INT_MAX.  Rows 4-byte aligned.  Lowe's ratio
 *                         test 0.75 is 16 * dist[0] < 9 * dist[1] (the caller's). */
#define FFN_SIFT_MAX_SIDE 16384
#define FFN_SIFT_MAX_TAPS 63
int ffn_sift_base(void* stream, const uint8_t* img, float* out, int H, int W, int C);
int ffn_gauss_blur_f32(void* stream, const float* src, float* dst, float* tmp, int H, int W, const float* taps, int T);
int ffn_decimate2_f32(void* stream, const float* src, float* dst, int H, int W);
int ffn_sift_extrema(void* stream, const float* gauss, float* dog, int h, int w, int* cand, int cap, int* counter, int* count);
int ffn_sift_refine_orient(void* stream, const float* dog, const float* gauss, int h, int w, int octave, const int* cand, int n, float* out);
int ffn_sift_describe(void* stream, const float* gauss, int h, int w, int octave, const float* kp, int n, uint8_t* desc, float* raw);
int ffn_knn2_u8(void* stream, const uint8_t* des1, int n1, const uint8_t* des2, int n2, int* idx, int* dist);

/* ---- device image preparation of the DINOv2 feature metrics (FID-DINO, Kernel Distance) ---------------------------------------------------
 * Reference: evaluation/metrics/FID/fid_score.py:122-124 -- TF.Resize((224, 224)) of a PIL image (antialiased bilinear), TF.ToTensor, TF.Normalize, on the
 * host; here from the decoded uint8 image to the operand rows of the patch-embedding GEMM on the device (csrc/imgprep.h).  Images are [B][H][W][3] uint8,
 * contiguous, any byte alignment.  No side of a source or destination image may exceed FFN_IMGPREP_MAX_SIDE (the horizontal pass stages one source row
 * in LDS); larger images are refused with FFN_EINVAL.
 *
 * ffn_resize_pil_bilinear_u8: PIL's Image.resize((ow, oh), BILINEAR) in PIL's own integer arithmetic (libImaging/Resample.c, 8 bits per channel): a
 * horizontal pass src -> scratch [B][H][ow][3], a vertical pass scratch -> dst [B][oh][ow][3], each clamp((2^21 + sum pixel * k) >> 22, 0, 255) in int32.
 * The tables are device int32 arrays the caller builds on the host in float64 (freefine_amd.ops.pil_bilinear_coeffs): bounds [out][2] = (first source index,
 * number of taps), coef [out][ksize] with ksize = 2 ceil(max(in / out, 1)) + 1 (checked).  Bounds are clamped into the image by the kernels.  B <= 65535.
 *
 * ffn_vit_patch_rows: out [B (H / patch)(W / patch)][ldo] in fp32 (FFN_F32) or bf16 (FFN_BF16, round to nearest even): row = patch (row-major over the patch
 * grid), column (c, ky, kx) = lut[c][src[b][py patch + ky][px patch + kx][c]], columns 3 patch^2 .. ldo - 1 zero -- the im2col rows of
 * Conv2d(3, C, kernel = stride = patch) over the normalised image.  lut: device fp32 [3][256], ToTensor + Normalize per channel and byte value, evaluated by the
 * caller.  H, W multiples of patch; ldo >= 3 patch^2.  FFN_BF16X3 is refused: the pair form has an entry of its own.
 *
 * ffn_vit_patch_rows_pair (ABI version 7): the same rows as the A operand of an FFN_BF16X3 GEMM -- out bf16 [B (H / patch)(W / patch)][2K], the PAIR form (FFN_BF16X3
 * above) of rows of K fp32 columns: K % 32 == 0: 128-byte blocks [hi(32) | lo(32)], otherwise the planes [hi(K) | lo(K)]; hi = bf16(v) (round to nearest even),
 * lo = bf16(v - hi), v = lut[c][byte]; columns 3 patch^2 .. K - 1 zero in both halves.  By definition the bytes ffn_vit_patch_rows(FFN_F32, ldo = K) followed by
 * ffn_split_pair(rows, K, K) writes, without the fp32 rows going through memory.  Refused with FFN_EINVAL before any launch: what ffn_vit_patch_rows refuses,
 * K < 3 patch^2, K % 8 != 0 (a thread writes 8 columns of each half as one 16-byte store), out not 16-byte aligned. */
#define FFN_IMGPREP_MAX_SIDE 4096
int ffn_resize_pil_bilinear_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int oh, int ow, const int* hbounds,
                               const int* hcoef, int hksize, const int* vbounds, const int* vcoef, int vksize);
int ffn_vit_patch_rows(void* stream, int dtype, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int patch, int ldo);
int ffn_vit_patch_rows_pair(void* stream, const uint8_t* src, const float* lut, void* out, int B, int H, int W, int patch, int K);

/* ---- the general PIL resize of the consistency metrics (Background / Subject Consistency; ABI version 6) -----------------------------------------
 * Reference: evaluation/metrics/VBench/background_consistency.py:18-28 (image * keep mask, then CLIP's transform: PIL BICUBIC resize, centre crop),
 * VBench/subject_consistency.py:10-22 (image * keep mask, torchvision Resize(224): PIL BILINEAR).  What ffn_resize_pil_bilinear_u8 does, plus:
 *   any PIL filter   the caller gives the table widths (1 <= hksize, vksize <= FFN_IMGPREP_MAX_TAPS: what PIL's widest filter, Lanczos of support 3, needs at
 *                    FFN_IMGPREP_MAX_SIDE); coefficients are signed (bicubic has negative taps); (first index, taps) are clamped into the row by the kernels
 *   C = 1 or 3       src [B][H][W][C] (a mask is a one-channel image)
 *   a crop window    rows y0 .. y0 + ch - 1 and columns x0 .. x0 + cw - 1 of the oh x ow destination the tables describe: dst [B][ch][cw][C],
 *                    scratch [B][H][cw][C]; only the window is computed
 *   a keep mask      rule FFN_KEEP_SUM_LT128: a pixel is kept iff (uint8)(m1 + m2) < 128 (numpy's uint8 wrap: 200 + 100 = 44 keeps, 128 + 128 = 0 keeps;
 *                    m2 may be null = 0); FFN_KEEP_GT128: iff m1 > 128 (m2 ignored); a dropped pixel reads as 0 in all channels.  m1 / m2: uint8 [B][H][W].
 *                    FFN_KEEP_NONE: no mask (m1, m2 ignored).  Masks need C = 3.  The masked image is never written to memory.
 * Refused with FFN_EINVAL before any launch: null pointers, sides beyond FFN_IMGPREP_MAX_SIDE, C outside {1, 3}, a window outside the destination, an unknown
 * rule, a mask with C = 1, a rule without m1, a table width outside 1 .. FFN_IMGPREP_MAX_TAPS.  B <= 65535. */
#define FFN_IMGPREP_MAX_TAPS (2 * 3 * FFN_IMGPREP_MAX_SIDE + 1)
enum { FFN_KEEP_NONE = 0, FFN_KEEP_SUM_LT128 = 1, FFN_KEEP_GT128 = 2 };
typedef struct {
    const uint8_t* src;
    uint8_t* dst;
    uint8_t* scratch;
    const uint8_t* m1;
    const uint8_t* m2;
    const int* hbounds;
    const int* hcoef;
    const int* vbounds;
    const int* vcoef;
    int B, H, W, C, oh, ow, hksize, vksize;
    int y0, x0, ch, cw;
    int rule;
} ffn_resize_pil_desc;
int ffn_resize_pil_u8(void* stream, const ffn_resize_pil_desc* d);

/* ---- device case preparation of the GeoBench harness (ABI version 9; csrc/caseprep.h) ------------------------------------------------------------
 * Reference: the cv2 restatements of src/utils/vis_utils.py (_resize_lanczos4, _resize_nearest, dilate_mask, re_edit_2d / re_edit_3d), which stay the
 * reference: every entry gives the bytes the numpy function gives.  Like the numpy functions, the interpolating paths are pinned to that restatement, NOT to
 * OpenCV (whose 8-bit paths use fixed-point coefficient tables).  Images are [B][H][W][C] uint8, contiguous, any byte alignment, C in {1, 3}, 1 <= B <= 65535,
 * sides 1 .. FFN_IMGPREP_MAX_SIDE; null pointers and anything outside these limits are refused with FFN_EINVAL before any launch.  All floating point is fp64
 * with contraction off: every product and every sum below is rounded on its own.
 *
 * ffn_resize_taps8_u8: an 8-tap separable resize (cv2.INTER_LANCZOS4 as _lanczos4_matrix states it).  Tables built by the caller on the host in float64
 * (freefine_amd.ops.lanczos4_taps): iy [oh][8] / ix [ow][8] int32 source indices, already clamped to the border (the kernel clamps again), wy [oh][8] /
 * wx [ow][8] fp64 weights, already normalised.  v[y][X][c] = sum_j wy[y][j] * src[iy[y][j]][X][c]; out[y][x][c] = sum_j wx[x][j] * v[y][ix[x][j]][c]; each
 * sum starts at 0 and adds its taps in ascending j; then rint (round half to even) and clamp to 0 .. 255.  v is recomputed per output pixel: no scratch.
 * Equal source and destination size is the caller's plain copy (the tables of that case are not the identity).
 *
 * ffn_resize_gather_u8: dst[y][x][c] = src[iy[y]][ix[x]][c] through two int32 tables (cv2.INTER_NEAREST: min(int(d * src / dst), src - 1) in float64, built
 * by the caller; clamped again by the kernel).  binarise != 0: every nonzero byte is written as 1 (the m[m > 0] = 1 of read_and_resize_mask).
 *
 * ffn_dilate_u8: the k x k maximum with anchor k / 2 (cv2.dilate(ones(k, k)) = scipy.ndimage.maximum_filter(size = (k, k), mode = "constant", cval = 0)):
 * 1 <= k <= 255, separable, scratch is a uint8 image of the source's size; the window of output x covers inputs x - k / 2 .. x + k - k / 2 - 1 (for even k one
 * more to the left than to the right); pixels outside the image read as 0.  dst may not alias src or scratch.
 *
 * ffn_mask_bbox_u8: box [B][4] int32 = (-top, bottom, -left, right): the first / last row and column of mask [B][H][W][C] whose CHANNEL 0 is nonzero -- the
 * bounding box _affine_for_edit takes from np.where.  An empty mask leaves bottom < 0.  The launch presets box (hipMemsetAsync), then reduces with integer
 * atomics.  The caller reads 16 bytes per case back.
 *
 * ffn_coarse_edit_2d: re_edit_2d / re_edit_3d in one kernel.  inv [B][6] fp64 on the device: rows 0 and 1 (a00 a01 a02 / a10 a11 a12) of the INVERSE affine,
 * computed by the caller as _warp_affine does (np.linalg.inv of the matrix of _affine_for_edit).  Per destination pixel (x, y):
 *   sx = (a00 x + a01 y) + a02, sy = (a10 x + a11 y) + a12        in this bracketing
 *   target mask = 255 iff src_mask[floor(sy + 0.5)][floor(sx + 0.5)] channel 0 is nonzero (0 outside the source), else 0
 *   q = floor(s * 32 + 0.5) / 32 per axis, (x0, y0) = floor(q), (fx, fy) = q - floor(q); four taps, a tap outside the source is 0;
 *   warped = rint((t00 (1 - fx) + t01 fx)(1 - fy) + (t10 (1 - fx) + t11 fx) fy), round half to even (the blend is exact: 8 x 5 x 5 bits)
 *   final = target ? warped : bg;   trans_hole = target ? warped : (hole_mask ? 0 : hole_img)
 * src_img, bg, hole_img, final_img, trans_hole: [B][H][W][3]; src_mask [B][H][W][mask_c], channel 0 read; tmask [B][H][W].  hole_img null: src_img;
 * hole_mask null: src_mask's channel 0; else hole_mask [B][H][W][hole_mask_c], with 3 channels applied per channel (numpy's broadcast in re_edit_3d).
 * The warped image and the warped mask are never written to memory.  Outputs may not alias inputs. */
typedef struct {
    const uint8_t* src_img;
    const uint8_t* src_mask;
    const uint8_t* bg;
    const uint8_t* hole_img;
    const uint8_t* hole_mask;
    const double* inv;
    uint8_t* final_img;
    uint8_t* tmask;
    uint8_t* trans_hole;
    int B, H, W, mask_c, hole_mask_c;
} ffn_coarse_edit_desc;
int ffn_resize_taps8_u8(void* stream, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow, const int* iy, const double* wy, const int* ix,
                        const double* wx);
int ffn_resize_gather_u8(void* stream, const uint8_t* src, uint8_t* dst, int B, int H, int W, int C, int oh, int ow, const int* iy, const int* ix, int binarise);
int ffn_dilate_u8(void* stream, const uint8_t* src, uint8_t* dst, uint8_t* scratch, int B, int H, int W, int C, int k);
int ffn_mask_bbox_u8(void* stream, const uint8_t* mask, int* box, int B, int H, int W, int C);
int ffn_coarse_edit_2d(void* stream, const ffn_coarse_edit_desc* d);

/* ---- click-to-mask: what surrounds the EfficientSAM network (ABI version 11; csrc/sam.h, freefine_amd/sam.py) -----------------------------------------
 * Reference: evaluation/DesignEdit/sam/efficient_sam/efficient_sam.py (preprocess :223-234, predict_masks :126-129) and efficient_sam_decoder.py:312, reached
 * from src/demo/utils.py:40-100.  Floating-point contraction is off in these kernels: every product and every sum is rounded on its own, in fp32.  All four
 * entries validate before any launch and refuse with FFN_EINVAL: null pointers, non-positive sizes, a side beyond FFN_IMGPREP_MAX_SIDE, N beyond 65535.
 *
 * The patch-row entries: src uint8 [B][H][W][3] of any size -> the operand rows [B (side / patch)^2][ldo] of the patch-embedding GEMM for a side x side
 * network input, columns (c, ky, kx), zero from 3 patch^2 on, in fp32 / bf16 (FFN_F32 / FFN_BF16) -- or, the _pair entry, the PAIR form bf16 [..][2K] of rows of
 * K fp32 columns (K % 8 == 0, out 16-byte aligned; layout and hi / lo as in the ViT patch-row pair entry above).  v = byte / 255; if (H, W) != (side, side), ATen's
 * upsample_bilinear2d with align_corners = False and no antialiasing: scale = in / out in fp32, source = scale (dst + 0.5) - 0.5 clamped at 0, i0 = min(int(source),
 * in - 1), i1 = i0 + (i0 < in - 1), weight of i1 = source - i0 in [0, 1], blended as h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11); then (v - mean[c]) / std[c].
 * mean, std: HOST float [3], read before the call returns (they travel as kernel arguments); std > 0.  The fp32 image is never written to memory.
 *
 * The hyper-mask entry: out [N][M][hw] fp32 = sum_c hyper[n][m][c] up[n][pixel][c], ascending c: up fp32 [N][hw][C] (NHWC rows of the upscaled embedding, 16-byte aligned),
 * hyper fp32 [N][M][C]; C % 4 == 0, C <= 64, M <= 8, hw <= FFN_IMGPREP_MAX_SIDE squared.
 *
 * The bicubic entry: src fp32 [N][h][w] -> dst fp32 [N][H][W] by ATen's upsample_bicubic2d with align_corners = False, A = -0.75: scale = in / out in fp32, source =
 * scale (dst + 0.5) - 0.5 NOT clamped, t = source - floor(source), taps floor(source) - 1 .. + 2 each clamped to the border, coefficients cubic_convolution2(t + 1),
 * cubic_convolution1(t), cubic_convolution1(1 - t), cubic_convolution2(2 - t); the four column taps of each row are summed first, then the four rows.  mask (may be
 * NULL): uint8 [N][H][W] = 255 where the value STORED in dst is >= 0, else 0 (torch.ge(logits, 0) of src/demo/utils.py:94). */
int ffn_sam_patch_rows(void* stream, int dtype, const uint8_t* src, void* out, int B, int H, int W, int side, int patch, int ldo, const float* mean, const float* std);
int ffn_sam_patch_rows_pair(void* stream, const uint8_t* src, void* out, int B, int H, int W, int side, int patch, int K, const float* mean, const float* std);
int ffn_hyper_masks(void* stream, const float* up, const float* hyper, float* out, int N, int hw, int C, int M);
int ffn_upsample_bicubic(void* stream, const float* src, float* dst, uint8_t* mask, int N, int h, int w, int H, int W);

/* ---- automatic mask generation: what a point-grid pass wants from its candidate maps (ABI version 14; csrc/sam.h, HipEfficientSam.generate) ----------
 * Reference: evaluation/GeoDiffuser/GeoDiffuser/segment_anything/automatic_mask_generator.py (_process_batch :266-321) and utils/amg.py (calculate_stability_score
 * :156, batched_mask_to_box :303).  Both entries validate before any launch and refuse with FFN_EINVAL.
 *
 * The statistics entry: src fp32 [N][h][w] -> stats int32 [N][8] over the H x W values v that ffn_upsample_bicubic would store for the same arguments (the two
 * kernels call one device function: v is the same bit pattern), WITHOUT storing them:
 *     stats[n] = { area = #(v >= 0), n_hi = #(v > +offset), n_lo = #(v > -offset), x_min, y_min, x_max, y_max, 0 }
 * area counts the bits of ffn_upsample_bicubic's byte mask; n_hi, n_lo compare strictly, as calculate_stability_score does (stability = n_hi / n_lo); the extents are
 * those of the pixels with v >= 0, maxima inclusive as in batched_mask_to_box, and 0, 0, 0, 0 for an empty map.  stats is initialised by the entry itself (its
 * previous content does not matter).  mask (may be NULL): uint8 [N][H][W] = 255 (v >= 0), else 0 -- the byte mask without the fp32 image.  All accumulation is in
 * integers: the result does not depend on the order of execution.  Refused: null src / stats, N outside 1 .. 65535, a side outside 1 .. FFN_IMGPREP_MAX_SIDE,
 * offset negative or not finite.
 *
 * The NMS entry: boxes fp32 [M][4] (x1, y1, x2, y2), ordered best first -> suppress uint64 [M][ceil(M / 64)], every word written: bit (j % 64) of word (j / 64) of
 * row i is set iff j > i and iou(i, j) > thresh, with torchvision's box arithmetic in fp32, each operation rounded on its own:
 *     area = (x2 - x1)(y2 - y1); inter = max(min(x2) - max(x1), 0) max(min(y2) - max(y1), 0); iou = inter / (area_i + area_j - inter)
 * (no "+ 1"; two zero-area boxes give 0 / 0 = NaN, which is not > thresh: they do not suppress each other).  The greedy sweep -- keep row i unless an earlier KEPT
 * row has bit i set -- is the caller's (freefine_amd/ops.py box_nms runs it on the host from the copied matrix).  Refused: null pointers, M outside
 * 1 .. FFN_BOX_NMS_MAX, a thresh that is not finite. */
#define FFN_BOX_NMS_MAX 16384
int ffn_upsample_bicubic_stats(void* stream, const float* src, int32_t* stats, uint8_t* mask, int N, int h, int w, int H, int W, float offset);
int ffn_box_nms(void* stream, const float* boxes, uint64_t* suppress, int M, float thresh);

/* ---- the Inception-v3 feature extractor of FID (ABI version 16; csrc/convkk.h, csrc/inception.hip, freefine_amd/inception.py) ----------------------------
 * Reference: evaluation/metrics/FID/fid.py, fid_score.py and inception.py (pytorch-fid's InceptionV3).  Everything is fp32 and NHWC as a COLUMN VIEW: a pixel's
 * channels are contiguous, consecutive pixels are `ld` floats apart (ld >= channels), so an entry reads or writes a slice of a wider tensor -- every branch of a
 * Mixed block writes straight into its columns of the concatenated output.  Bytes outside the view are never written.  All entries: no allocation, no sync, the
 * caller's stream; pointers 16-byte aligned and strides multiples of 4 floats; anything outside the stated limits is refused with FFN_EINVAL before any launch.
 *
 * ffn_conv2d: out[b][oy][ox][n] = act(bias[n] + sum over (ky, kx, ci) of x[b][oy stride - pad_h + ky][ox stride - pad_w + kx][ci] w[n][(ky KW + kx) Cin + ci]),
 * taps outside the image contributing zero; Hout = (Hin + 2 pad_h - KH) / stride + 1 (floor), Wout likewise.  An implicit GEMM on the exact-fp32 MFMA
 * (v_mfma_f32_16x16x4_f32): dtype FFN_F32 only, any other dtype returns FFN_ENOSYS.  x [B][Hin][Win] pixels of Cin channels, stride ldx; w [N][Kpad] with
 * K = KH KW Cin <= Kpad, Kpad % 4 == 0 (columns K .. Kpad - 1 are not read); bias [N] or NULL; out [B][Hout][Wout] pixels of N channels, stride ldo.
 * KH, KW in {1, 3, 5, 7} independently; stride 1 or 2 (both axes); pad_h, pad_w >= 0 independently; Cin % 4 == 0, N % 4 == 0.  flags: FFN_CONV_RELU
 * (act = max(., 0); otherwise the identity).  The summation order is fixed: two runs give the same bits.
 *
 * ffn_pool2d: k x k windows, stride and pad on both axes, floor output sizes; FFN_POOL_MAX (max_pool2d: padding never wins) or FFN_POOL_AVG_VALID (the mean over
 * the window's in-image taps, summed in (ky, kx) order: avg_pool2d(count_include_pad=False)).  k 1 .. 7, stride 1 .. k, 2 pad <= k, C % 4 == 0.
 * ffn_mean_hw: y [B][C] (contiguous) = the mean over the HW pixels of x [B][HW] (stride ldx), summed in ascending order: AdaptiveAvgPool2d(1).
 * ffn_fid_prep: src uint8 [B][side_in][side_in][3] -> out fp32 [B][side_out][side_out][4]: v = lut[c][byte] (lut fp32 [3][256]: ToTensor + Normalize, as
 * ffn_vit_patch_rows takes it), ATen's upsample_bilinear2d with align_corners = False (scale = in / out in fp32, source = max(0, scale (dst + 0.5) - 0.5),
 * blended as h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11)), then 2 v - 1; the fourth channel is zero (the stem is a Cin = 4 convolution). */
typedef struct ffn_conv2d_desc {
    const float* x;
    const float* w;
    const float* bias;
    float* out;
    int B, Hin, Win, Cin, N;
    int KH, KW, stride, pad_h, pad_w;
    int ldx, ldo, Kpad, flags;
} ffn_conv2d_desc;
enum { FFN_CONV_RELU = 1 };
enum { FFN_POOL_MAX = 0, FFN_POOL_AVG_VALID = 1 };
int ffn_conv2d(void* stream, int dtype, const ffn_conv2d_desc* d);
int ffn_pool2d(void* stream, int op, const float* x, float* y, int B, int Hin, int Win, int C, int ldx, int ldy, int k, int stride, int pad);
int ffn_mean_hw(void* stream, const float* x, float* y, int B, int HW, int C, int ldx);
int ffn_fid_prep(void* stream, const uint8_t* src, const float* lut, float* out, int B, int side_in, int side_out);

#ifdef __cplusplus
}
#endif
#endif
