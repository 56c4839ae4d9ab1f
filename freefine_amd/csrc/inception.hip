// The Inception-v3 unit of libfreefine_hip.so (FID: freefine_amd/inception.py): the general KH x KW convolution on the exact-fp32 MFMA, window pooling, the
// global mean and the image preparation (convkk.h).  Default code generation.  The unit exports the entries of its own kernels.
#include "capi_common.h"
#include "convkk.h"

// the tiles of ffn_conv2d: (BM, BN) and what one 256-thread workgroup of each costs relative to its BM x BN outputs (narrower tiles re-read more of A per output)
struct convkk_tile {
    int bm, bn;
    float cost;
};
static const convkk_tile kConvTiles[] = {{128, 128, 1.00f}, {128, 64, 1.10f}, {128, 32, 1.30f}, {64, 64, 1.25f}};

// the tile that finishes first: rounds of resident workgroups (two per CU) x the work of one, padding included
static int convkk_choose(int M, int N) {
    const long resident = 2L * device_cus();
    int best = 0;
    double best_t = 0.0;
    for (int i = 0; i < (int)(sizeof(kConvTiles) / sizeof(kConvTiles[0])); ++i) {
        const convkk_tile& t = kConvTiles[i];
        const long blocks = (long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
        const double time = (double)((blocks + resident - 1) / resident) * t.bm * t.bn * t.cost;
        if (i == 0 || time < best_t) best = i, best_t = time;
    }
    return best;
}

static inline bool odd_1_to_7(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

extern "C" int ffn_conv2d(void* stream, int dtype, const ffn_conv2d_desc* d) {
    if (dtype != FFN_F32) return fail(FFN_ENOSYS, "conv2d: dtype %d (FFN_F32 only)", dtype);
    REQUIRE(d, "conv2d: null descriptor");
    REQUIRE(d->x && d->w && d->out, "conv2d: null pointer");
    REQUIRE(d->B >= 1 && d->Hin >= 1 && d->Win >= 1, "conv2d: bad shape B=%d, %d x %d", d->B, d->Hin, d->Win);
    REQUIRE(odd_1_to_7(d->KH) && odd_1_to_7(d->KW), "conv2d: kernel %d x %d (each side one of 1, 3, 5, 7)", d->KH, d->KW);
    REQUIRE(d->stride == 1 || d->stride == 2, "conv2d: stride=%d (1 or 2)", d->stride);
    REQUIRE(d->pad_h >= 0 && d->pad_w >= 0 && d->pad_h <= 1024 && d->pad_w <= 1024, "conv2d: padding (%d, %d) outside 0 .. 1024", d->pad_h, d->pad_w);
    REQUIRE(d->Cin >= 4 && d->Cin % 4 == 0, "conv2d: Cin=%d is not a positive multiple of 4", d->Cin);
    REQUIRE(d->N >= 4 && d->N % 4 == 0, "conv2d: N=%d is not a positive multiple of 4", d->N);
    REQUIRE(d->Hin + 2 * d->pad_h >= d->KH && d->Win + 2 * d->pad_w >= d->KW, "conv2d: a %d x %d kernel does not fit the padded %d x %d image", d->KH, d->KW,
            d->Hin + 2 * d->pad_h, d->Win + 2 * d->pad_w);
    REQUIRE((long)d->KH * d->KW * d->Cin <= (1L << 24), "conv2d: K=%ld beyond 2^24", (long)d->KH * d->KW * d->Cin);
    const int K = d->KH * d->KW * d->Cin;
    REQUIRE(d->Kpad >= K && d->Kpad % 4 == 0, "conv2d: Kpad=%d must be a multiple of 4 and at least K=%d", d->Kpad, K);
    REQUIRE(d->ldx >= d->Cin && d->ldx % 4 == 0, "conv2d: ldx=%d must be a multiple of 4 and at least Cin=%d", d->ldx, d->Cin);
    REQUIRE(d->ldo >= d->N && d->ldo % 4 == 0, "conv2d: ldo=%d must be a multiple of 4 and at least N=%d", d->ldo, d->N);
    REQUIRE((d->flags & ~FFN_CONV_RELU) == 0, "conv2d: unknown flags 0x%x", d->flags);
    REQUIRE(aligned16(d->x) && aligned16(d->w) && aligned16(d->out) && aligned16(d->bias), "conv2d: x, w, bias and out must be 16-byte aligned");
    const int Hout = (d->Hin + 2 * d->pad_h - d->KH) / d->stride + 1, Wout = (d->Win + 2 * d->pad_w - d->KW) / d->stride + 1;
    const long M = (long)d->B * Hout * Wout;
    REQUIRE(M < (1L << 31) - 256 && (long)d->B * d->Hin * d->Win < (1L << 31), "conv2d: B=%d images of %d x %d: more than 2^31 pixels", d->B, d->Hin, d->Win);
    convkk_args a;
    a.x = d->x, a.w = d->w, a.bias = d->bias, a.out = d->out;
    a.M = (int)M, a.N = d->N, a.K = K, a.Kpad = d->Kpad;
    a.Hin = d->Hin, a.Win = d->Win, a.Cin = d->Cin, a.Hout = Hout, a.Wout = Wout, a.KH = d->KH, a.KW = d->KW, a.stride = d->stride;
    a.pad_h = d->pad_h, a.pad_w = d->pad_w, a.ldx = d->ldx, a.ldo = d->ldo, a.relu = (d->flags & FFN_CONV_RELU) != 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const convkk_tile& t = kConvTiles[convkk_choose(a.M, a.N)];
    const dim3 grid((unsigned)((a.M + t.bm - 1) / t.bm), (unsigned)((a.N + t.bn - 1) / t.bn)), blk(CONVKK_THREADS);
    REQUIRE(grid.y <= 65535, "conv2d: N=%d beyond 65535 column tiles", d->N);
    if (t.bm == 128 && t.bn == 128) LAUNCH((convkk_kernel<128, 128, 64, 64>), grid, blk, 0, s, a);
    else if (t.bm == 128 && t.bn == 64) LAUNCH((convkk_kernel<128, 64, 64, 32>), grid, blk, 0, s, a);
    else if (t.bm == 128) LAUNCH((convkk_kernel<128, 32, 32, 32>), grid, blk, 0, s, a);
    else LAUNCH((convkk_kernel<64, 64, 32, 32>), grid, blk, 0, s, a);
    return check_launch("conv2d");
}

extern "C" int ffn_pool2d(void* stream, int op, const float* x, float* y, int B, int Hin, int Win, int C, int ldx, int ldy, int k, int stride, int pad) {
    REQUIRE(op == FFN_POOL_MAX || op == FFN_POOL_AVG_VALID, "pool2d: unknown op %d", op);
    REQUIRE(x && y, "pool2d: null pointer");
    REQUIRE(B >= 1 && Hin >= 1 && Win >= 1, "pool2d: bad shape B=%d, %d x %d", B, Hin, Win);
    REQUIRE(C >= 4 && C % 4 == 0, "pool2d: C=%d is not a positive multiple of 4", C);
    REQUIRE(k >= 1 && k <= 7 && stride >= 1 && stride <= k, "pool2d: window %d, stride %d (window 1 .. 7, stride 1 .. window)", k, stride);
    REQUIRE(pad >= 0 && 2 * pad <= k, "pool2d: pad=%d outside 0 .. half the window %d", pad, k);
    REQUIRE(Hin + 2 * pad >= k && Win + 2 * pad >= k, "pool2d: a window of %d does not fit the padded %d x %d image", k, Hin + 2 * pad, Win + 2 * pad);
    REQUIRE(ldx >= C && ldx % 4 == 0 && ldy >= C && ldy % 4 == 0, "pool2d: ldx=%d, ldy=%d must be multiples of 4 and at least C=%d", ldx, ldy, C);
    REQUIRE(aligned16(x) && aligned16(y), "pool2d: x and y must be 16-byte aligned");
    const int Hout = (Hin + 2 * pad - k) / stride + 1, Wout = (Win + 2 * pad - k) / stride + 1;
    REQUIRE((long)B * Hin * Win < (1L << 31), "pool2d: B=%d images of %d x %d: more than 2^31 pixels", B, Hin, Win);
    const long total = (long)B * Hout * Wout * (C / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)grid_for(total, CONVKK_THREADS, 65536)), blk(CONVKK_THREADS);
    if (op == FFN_POOL_MAX) LAUNCH(pool2d_kernel<FFN_POOL_MAX>, grid, blk, 0, s, x, y, total, Hin, Win, Hout, Wout, C / 4, ldx, ldy, k, stride, pad);
    else LAUNCH(pool2d_kernel<FFN_POOL_AVG_VALID>, grid, blk, 0, s, x, y, total, Hin, Win, Hout, Wout, C / 4, ldx, ldy, k, stride, pad);
    return check_launch("pool2d");
}

extern "C" int ffn_mean_hw(void* stream, const float* x, float* y, int B, int HW, int C, int ldx) {
    REQUIRE(x && y, "mean_hw: null pointer");
    REQUIRE(B >= 1 && HW >= 1 && (long)B * HW < (1L << 31), "mean_hw: bad shape B=%d, HW=%d", B, HW);
    REQUIRE(C >= 4 && C % 4 == 0, "mean_hw: C=%d is not a positive multiple of 4", C);
    REQUIRE(ldx >= C && ldx % 4 == 0, "mean_hw: ldx=%d must be a multiple of 4 and at least C=%d", ldx, C);
    REQUIRE(aligned16(x) && aligned16(y), "mean_hw: x and y must be 16-byte aligned");
    const long total = (long)B * (C / 4);
    LAUNCH(mean_hw_kernel, dim3((unsigned)((total + CONVKK_THREADS - 1) / CONVKK_THREADS)), dim3(CONVKK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), x, y, total, HW, C / 4,
           ldx);
    return check_launch("mean_hw");
}

extern "C" int ffn_fid_prep(void* stream, const uint8_t* src, const float* lut, float* out, int B, int side_in, int side_out) {
    const int lim = FFN_IMGPREP_MAX_SIDE;
    REQUIRE(src && lut && out, "fid_prep: null pointer");
    REQUIRE(B >= 1 && B <= 65535, "fid_prep: B=%d outside 1 .. 65535", B);
    REQUIRE(side_in >= 1 && side_in <= lim && side_out >= 1 && side_out <= lim, "fid_prep: sides %d -> %d outside 1 .. %d (FFN_IMGPREP_MAX_SIDE)", side_in, side_out, lim);
    REQUIRE(aligned16(out), "fid_prep: out must be 16-byte aligned");
    const long total = (long)B * side_out * side_out;
    REQUIRE(total < (1L << 31), "fid_prep: B=%d images of side %d: more than 2^31 pixels", B, side_out);
    LAUNCH(fid_prep_kernel, dim3((unsigned)((total + CONVKK_THREADS - 1) / CONVKK_THREADS)), dim3(CONVKK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, lut, out, total,
           side_in, side_out);
    return check_launch("fid_prep");
}
