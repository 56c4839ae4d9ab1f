// SIFT keypoints, descriptors and ratio-test matching for the Mean Distance metric (reference: evaluation/metrics/MD/mean_distance.py:49-79 takes its keypoints from
// cv2.SIFT_create().detectAndCompute and cv2.BFMatcher().knnMatch).  cv2 exists nowhere this is built, so nothing here is pinned to cv2's bytes: the kernels restate
// Lowe's algorithm with OpenCV's DEFAULT PARAMETERS (3 layers per octave, sigma 1.6, contrast threshold 0.04, edge threshold 10, first octave -1) and are held,
// stage by stage, to the fp64 restatement tests/sift_ref.py.  Deliberately not restated: cv2's fastAtan2 and its exp approximations (atan2f / expf here).
//
// Compiled with floating-point contraction OFF (the pragma below): every product is rounded before it is added, so the fp32 run of the restatement, which numpy
// evaluates one operation at a time, describes this arithmetic.
//
// Stages (one entry point each, so that each is testable on the device's own upstream output):
//   sift_base_kernel      uint8 HWC -> fp32 base image: gray = (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14 (OpenCV's 8-bit BGR2GRAY; the reference hands PIL's
//                         RGB array to cv2, so channel 0 -- red -- gets B's weight: kept), then 2x bilinear upsampling, source coordinate (d + 0.5) / 2 - 0.5,
//                         clamped at the edge.  The weights are 1/4 and 3/4: every output is a multiple of 1/16 below 256, exact in fp32.
//   sift_blur_kernel<V>   one pass of the separable Gaussian: out(p) = sum_k taps[k] * in(reflect101(p + k - T / 2)), k ASCENDING from an accumulator of 0, every
//                         product rounded, then added.  The horizontal pass runs first, the vertical pass on its result.  Taps come from the host.
//   sift_decimate_kernel  every second pixel: the first image of the next octave
//   sift_dog_kernel       D[i] = G[i + 1] - G[i], one fp32 subtraction
//   sift_extrema_kernel   26-neighbour extrema of D[1..3] with ties allowed, |v| > 1, 5-pixel border; wave-aggregated compaction (one ballot, one atomic per wave)
//   sift_refine_kernel    one wave per candidate: quadratic fit (Cramer's rule), contrast and edge tests, 36-bin orientation histogram, peaks
//   sift_describe_kernel  one workgroup per keypoint: 4 x 4 x 8 trilinear histogram, normalisation, uint8
//   knn2_u8_kernel        one workgroup per query row: the two nearest rows by squared L2 distance in int32, ties to the lower index
// Everything is deterministic: no floating-point atomics; the only atomic is the candidate counter, and the candidate ORDER it produces is removed again by the
// host's sort (freefine_amd/sift.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

#define SIFT_MAX_TAPS 63
#define SIFT_BORDER 5
#define SIFT_REFINE_FLOATS 27       // keep, layer, r, c, x, y, size, response, npeaks, 18 angles
#define SIFT_ORI_MAX_RADIUS 16
#define SIFT_DESC_CHUNK 1024
#define SIFT_DESC_THREADS 256

struct sift_taps {
    float t[SIFT_MAX_TAPS];
    int T;
};

// OpenCV's borderInterpolate(BORDER_REFLECT_101): ... c b | a b c d | c b ..., repeated until the index is inside (the last octaves are narrower than the kernel)
__device__ __forceinline__ int sift_reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__global__ __launch_bounds__(256) void sift_base_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int H, int W, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int OW = 2 * W;
    if (idx >= (long)2 * H * OW) return;
    const int oy = (int)(idx / OW), ox = (int)(idx - (long)oy * OW);
    const float sy = ((float)oy + 0.5f) * 0.5f - 0.5f, sx = ((float)ox + 0.5f) * 0.5f - 0.5f;
    const int fy0 = (int)floorf(sy), fx0 = (int)floorf(sx);
    const float ly = sy - (float)fy0, lx = sx - (float)fx0;
    const int y0 = min(max(fy0, 0), H - 1), y1 = min(max(fy0 + 1, 0), H - 1), x0 = min(max(fx0, 0), W - 1), x1 = min(max(fx0 + 1, 0), W - 1);
    auto gray = [&](int y, int x) -> float {
        const uint8_t* p = img + ((long)y * W + x) * C;
        if (C == 1) return (float)p[0];
        return (float)(((int)p[0] * 1868 + (int)p[1] * 9617 + (int)p[2] * 4899 + 8192) >> 14);
    };
    const float top = gray(y0, x0) * (1.f - lx) + gray(y0, x1) * lx, bot = gray(y1, x0) * (1.f - lx) + gray(y1, x1) * lx;
    out[idx] = top * (1.f - ly) + bot * ly;
}

template <bool VERTICAL>
__global__ __launch_bounds__(256) void sift_blur_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, sift_taps taps) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W), R = taps.T / 2;
    float acc = 0.f;
    for (int k = 0; k < taps.T; ++k) {
        const float v = VERTICAL ? in[(long)sift_reflect101(y + k - R, H) * W + x] : in[(long)y * W + sift_reflect101(x + k - R, W)];
        acc = acc + taps.t[k] * v;
    }
    out[idx] = acc;
}

// dst [H / 2][W / 2] = src [H][W] at (2 y, 2 x)
__global__ __launch_bounds__(256) void sift_decimate_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W) {
    const int h = H / 2, w = W / 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)h * w) return;
    const int y = (int)(idx / w), x = (int)(idx - (long)y * w);
    dst[idx] = src[(long)(2 * y) * W + 2 * x];
}

// G [6][hw] -> D [5][hw]
__global__ __launch_bounds__(256) void sift_dog_kernel(const float* __restrict__ G, float* __restrict__ D, long hw) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 5 * hw) return;
    D[idx] = G[idx + hw] - G[idx];
}

// grid covers 3 * (h - 10) * (w - 10) interior cells of layers 1..3 (the host launches it only when h, w >= 11).  cand [cap][3] = (layer, r, c); *count grows past
// cap on overflow (nothing is written past cap; the host reports it).
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ D, int h, int w, int* __restrict__ cand, int cap, int* __restrict__ count) {
    const int ih = h - 2 * SIFT_BORDER, iw = w - 2 * SIFT_BORDER;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, total = 3l * ih * iw;
    bool is = false;
    int layer = 0, r = 0, c = 0;
    if (idx < total) {
        layer = (int)(idx / ((long)ih * iw)) + 1;
        const long rem = idx - (long)(layer - 1) * ih * iw;
        r = (int)(rem / iw) + SIFT_BORDER;
        c = (int)(rem - (long)(r - SIFT_BORDER) * iw) + SIFT_BORDER;
        const long hw = (long)h * w;
        const float* p = D + layer * hw + (long)r * w + c;
        const float v = *p;
        if (fabsf(v) > 1.0f) {
            bool mx = v > 0.f, mn = v < 0.f;
#pragma unroll
            for (int dl = -1; dl <= 1; ++dl)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const float q = p[dl * hw + dy * w + dx];
                        mx = mx && v >= q;
                        mn = mn && v <= q;
                    }
            is = mx || mn;
        }
    }
    const unsigned long long m = __ballot(is);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(count, (int)__popcll(m));
    base = __shfl(base, 0, 64);
    if (is) {
        const int pos = base + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (pos < cap) {
            cand[3 * pos] = layer;
            cand[3 * pos + 1] = r;
            cand[3 * pos + 2] = c;
        }
    }
}

// atan2 in degrees, [0, 360)
__device__ __forceinline__ float sift_angle(float dy, float dx) {
    float a = atan2f(dy, dx) * 57.29577951308232f;
    if (a < 0.f) a = a + 360.f;
    return a;
}

// One wave (= one 64-thread workgroup) per candidate.  D [5][h][w], G [6][h][w] of octave o (0 = the upsampled base).  The refinement is a short serial
// computation that every lane repeats on the same values; the orientation samples (bin, weight * magnitude) are evaluated by all lanes into LDS, and lane j < 36
// then sums the samples of bin j in the window's raster order: no atomics, one fixed order.
__global__ __launch_bounds__(64) void sift_refine_kernel(const float* __restrict__ D, const float* __restrict__ G, int h, int w, int o, const int* __restrict__ cand,
                                                         int n, float* __restrict__ out) {
    __shared__ int s_bin[(2 * SIFT_ORI_MAX_RADIUS + 1) * (2 * SIFT_ORI_MAX_RADIUS + 1)];
    __shared__ float s_val[(2 * SIFT_ORI_MAX_RADIUS + 1) * (2 * SIFT_ORI_MAX_RADIUS + 1)];
    __shared__ float s_raw[36], s_sm[36];
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= n) return;
    float* rec = out + (long)k * SIFT_REFINE_FLOATS;
    int layer = cand[3 * k], r = cand[3 * k + 1], c = cand[3 * k + 2];
    const long hw = (long)h * w;
    const float img_scale = 1.f / 255.f, d1 = img_scale * 0.5f, d2 = img_scale, dc = img_scale * 0.25f;
    float xi = 0.f, xr = 0.f, xc = 0.f;
    bool keep = layer >= 1 && layer <= 3 && r >= SIFT_BORDER && r < h - SIFT_BORDER && c >= SIFT_BORDER && c < w - SIFT_BORDER;      // (a list from elsewhere: no read outside)
    int step = 0;
    for (; keep && step < 5; ++step) {
        const float* im = D + layer * hw + (long)r * w + c;
        const float* pv = im - hw;
        const float* nx = im + hw;
        const float gx = (im[1] - im[-1]) * d1, gy = (im[w] - im[-w]) * d1, gs = (nx[0] - pv[0]) * d1;
        const float v2 = im[0] * 2.f;
        const float dxx = (im[1] + im[-1] - v2) * d2, dyy = (im[w] + im[-w] - v2) * d2, dss = (nx[0] + pv[0] - v2) * d2;
        const float dxy = (im[w + 1] - im[w - 1] - im[-w + 1] + im[-w - 1]) * dc;
        const float dxs = (nx[1] - nx[-1] - pv[1] + pv[-1]) * dc, dys = (nx[w] - nx[-w] - pv[w] + pv[-w]) * dc;
        // H X = dD by Cramer's rule (a singular H gives X = 0), H = [[dxx dxy dxs] [dxy dyy dys] [dxs dys dss]]
        const float m00 = dyy * dss - dys * dys, m01 = dxy * dss - dys * dxs, m02 = dxy * dys - dyy * dxs;
        const float det = dxx * m00 - dxy * m01 + dxs * m02;
        float X0 = 0.f, X1 = 0.f, X2 = 0.f;
        if (det != 0.f) {
            const float id = 1.f / det;
            X0 = id * (gx * m00 - dxy * (gy * dss - dys * gs) + dxs * (gy * dys - dyy * gs));
            X1 = id * (dxx * (gy * dss - dys * gs) - gx * m01 + dxs * (dxy * gs - gy * dxs));
            X2 = id * (dxx * (dyy * gs - gy * dys) - dxy * (dxy * gs - gy * dxs) + gx * m02);
        }
        xc = -X0;
        xr = -X1;
        xi = -X2;
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        if (!(fabsf(xi) <= 715827882.f && fabsf(xr) <= 715827882.f && fabsf(xc) <= 715827882.f)) {      // INT_MAX / 3; NaN fails too
            keep = false;
            break;
        }
        c += (int)rintf(xc);
        r += (int)rintf(xr);
        layer += (int)rintf(xi);
        if (layer < 1 || layer > 3 || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER) keep = false;
    }
    if (step >= 5) keep = false;
    float contr = 0.f;
    if (keep) {
        const float* im = D + layer * hw + (long)r * w + c;
        const float gx = (im[1] - im[-1]) * d1, gy = (im[w] - im[-w]) * d1, gs = (im[hw] - im[-hw]) * d1;
        const float t = gx * xc + gy * xr + gs * xi;
        contr = im[0] * img_scale + t * 0.5f;
        if (fabsf(contr) * 3.f < 0.04f) keep = false;
        const float v2 = im[0] * 2.f;
        const float dxx = (im[1] + im[-1] - v2) * d2, dyy = (im[w] + im[-w] - v2) * d2;
        const float dxy = (im[w + 1] - im[w - 1] - im[-w + 1] + im[-w - 1]) * dc;
        const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
        if (det <= 0.f || tr * tr * 10.f >= 121.f * det) keep = false;
    }
    if (!keep) {
        if (lane < SIFT_REFINE_FLOATS) rec[lane] = 0.f;
        return;
    }
    const float scl = 1.6f * exp2f(((float)layer + xi) / 3.f);              // the keypoint's scale in its octave
    const float oct = (float)(1 << o) * 0.5f;                               // octave pixels -> input-image pixels (the base is the input upsampled 2x)
    const int radius = min((int)rintf(4.5f * scl), SIFT_ORI_MAX_RADIUS);    // layer + xi < 3.5, so 4.5 s < 16.2: the bound is never the smaller one
    const float sig = 1.5f * scl, escale = -1.f / (2.f * sig * sig);
    const float* g = G + layer * hw;
    const int side = 2 * radius + 1, len = side * side;
    for (int s = lane; s < len; s += 64) {
        const int i = s / side - radius, j = s - (s / side) * side - radius;
        const int y = r + i, x = c + j;
        int bin = -1;
        float v = 0.f;
        if (y > 0 && y < h - 1 && x > 0 && x < w - 1) {
            const float dx = g[(long)y * w + x + 1] - g[(long)y * w + x - 1], dy = g[(long)(y - 1) * w + x] - g[(long)(y + 1) * w + x];
            const float wgt = expf((float)(i * i + j * j) * escale), mag = sqrtf(dx * dx + dy * dy);
            bin = (int)rintf(0.1f * sift_angle(dy, dx));
            if (bin >= 36) bin -= 36;
            if (bin < 0) bin += 36;
            v = wgt * mag;
        }
        s_bin[s] = bin;
        s_val[s] = v;
    }
    __syncthreads();
    if (lane < 36) {                                                        // bin `lane`: its samples in the window's raster order
        float a = 0.f;
        for (int s = 0; s < len; ++s)
            if (s_bin[s] == lane) a = a + s_val[s];
        s_raw[lane] = a;
    }
    __syncthreads();
    if (lane < 36) {
        const int j = lane;
        s_sm[j] = (s_raw[(j + 34) % 36] + s_raw[(j + 2) % 36]) * (1.f / 16.f) + (s_raw[(j + 35) % 36] + s_raw[(j + 1) % 36]) * (4.f / 16.f) + s_raw[j] * (6.f / 16.f);
    }
    __syncthreads();
    if (lane == 0) {
        float omax = s_sm[0];
        for (int j = 1; j < 36; ++j) omax = fmaxf(omax, s_sm[j]);
        const float thr = omax * 0.8f;
        int np = 0;
        for (int j = 0; j < 36; ++j) {
            const float hl = s_sm[j > 0 ? j - 1 : 35], hr = s_sm[j < 35 ? j + 1 : 0], hj = s_sm[j];
            if (hj > hl && hj > hr && hj >= thr) {
                float bin = (float)j + 0.5f * (hl - hr) / (hl - 2.f * hj + hr);
                bin = bin < 0.f ? 36.f + bin : (bin >= 36.f ? bin - 36.f : bin);
                float ang = 360.f - 10.f * bin;
                if (fabsf(ang - 360.f) < 1.1920929e-7f) ang = 0.f;
                rec[9 + np] = ang;
                ++np;
            }
        }
        for (int q = np; q < 18; ++q) rec[9 + q] = 0.f;
        rec[0] = 1.f;
        rec[1] = (float)layer;
        rec[2] = (float)r;
        rec[3] = (float)c;
        rec[4] = ((float)c + xc) * oct;
        rec[5] = ((float)r + xr) * oct;
        rec[6] = scl * oct * 2.f;
        rec[7] = fabsf(contr);
        rec[8] = (float)np;
    }
}

// One workgroup per keypoint.  kp [n][7] = (x, y, size, angle, response, octave, layer) as sift_refine_kernel's records give them, all of octave o.  The samples
// of the (2 radius + 1)^2 window are evaluated SIFT_DESC_CHUNK at a time into LDS; then thread (i, j, k) of the 4 x 4 x 9 bins walks the chunk in sample order and
// adds the samples that touch its bin: every bin is summed in the window's raster order, without atomics.  Orientation bin 8 is folded into bin 0 at the end.
// raw (may be null): the 128 values before the conversion to uint8.
__global__ __launch_bounds__(SIFT_DESC_THREADS) void sift_describe_kernel(const float* __restrict__ G, int h, int w, int o, const float* __restrict__ kp, int n,
                                                                          uint8_t* __restrict__ desc, float* __restrict__ raw) {
    __shared__ float s_r[SIFT_DESC_CHUNK], s_c[SIFT_DESC_CHUNK], s_o[SIFT_DESC_CHUNK], s_m[SIFT_DESC_CHUNK];
    __shared__ float s_fold[16], s_d[128], s_scale[2];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= n) return;
    const float* q = kp + (long)k * 7;
    const float toct = 2.f / (float)(1 << o);                               // input-image pixels -> octave pixels
    const float px = q[0] * toct, py = q[1] * toct, scl = q[2] * toct * 0.5f;
    float ori = 360.f - q[3];
    if (fabsf(ori - 360.f) < 1.1920929e-7f) ori = 0.f;
    int layer = (int)q[6];
    layer = min(max(layer, 0), 5);
    const float* g = G + (long)layer * h * w;
    const int cx = (int)rintf(px), cy = (int)rintf(py);
    const float hist_width = 3.f * scl;
    const int diag = (int)sqrt((double)w * w + (double)h * h);
    const float fr = rintf(hist_width * 1.4142135623730951f * 5.f * 0.5f);
    const int radius = fr >= 0.f && fr < (float)diag ? (int)fr : (fr >= (float)diag ? diag : 0);
    const float ang = ori * 0.017453292519943295f;
    const float cos_t = cosf(ang) / hist_width, sin_t = sinf(ang) / hist_width;
    const int side = 2 * radius + 1;
    const long len = (long)side * side;
    const int bi = tid / 36, bj = (tid / 9) % 4, bk = tid % 9;              // the bin of threads 0..143
    float acc = 0.f;
    for (long base = 0; base < len; base += SIFT_DESC_CHUNK) {
        const int cnt = (int)min((long)SIFT_DESC_CHUNK, len - base);
        for (int s = tid; s < cnt; s += SIFT_DESC_THREADS) {
            const long t = base + s;
            const int i = (int)(t / side) - radius, j = (int)(t - (t / side) * side) - radius;
            const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
            const float rbin = r_rot + 2.f - 0.5f, cbin = c_rot + 2.f - 0.5f;
            const int y = cy + i, x = cx + j;
            float m = 0.f, ob = 0.f, rb = -100.f;
            if (rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && y > 0 && y < h - 1 && x > 0 && x < w - 1) {
                const float dx = g[(long)y * w + x + 1] - g[(long)y * w + x - 1], dy = g[(long)(y - 1) * w + x] - g[(long)(y + 1) * w + x];
                const float wgt = expf((c_rot * c_rot + r_rot * r_rot) * -0.125f);
                ob = (sift_angle(dy, dx) - ori) * (8.f / 360.f);
                m = sqrtf(dx * dx + dy * dy) * wgt;
                rb = rbin;
            }
            s_r[s] = rb;
            s_c[s] = cbin;
            s_o[s] = ob;
            s_m[s] = m;
        }
        __syncthreads();
        if (tid < 144) {
            for (int s = 0; s < cnt; ++s) {
                float rbin = s_r[s];
                if (rbin < -50.f) continue;                                 // outside the window or the image: not a sample
                float cbin = s_c[s], obin = s_o[s];
                const float mag = s_m[s];
                const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
                rbin = rbin - r0f;
                cbin = cbin - c0f;
                obin = obin - o0f;
                int o0 = (int)o0f;
                if (o0 < 0) o0 += 8;
                if (o0 >= 8) o0 -= 8;
                const int dr = bi - (int)r0f, dcc = bj - (int)c0f, dob = bk - o0;
                if ((dr | dcc | dob) & ~1) continue;                        // each of the three in {0, 1}
                const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
                const float vr = dr ? v_r1 : v_r0;
                const float v_c1 = vr * cbin, v_c0 = vr - v_c1;
                const float vc = dcc ? v_c1 : v_c0;
                const float v_o1 = vc * obin, v_o0 = vc - v_o1;
                acc = acc + (dob ? v_o1 : v_o0);
            }
        }
        __syncthreads();
    }
    if (tid < 144 && bk == 8) s_fold[bi * 4 + bj] = acc;
    __syncthreads();
    if (tid < 144 && bk < 8) s_d[(bi * 4 + bj) * 8 + bk] = bk == 0 ? acc + s_fold[bi * 4 + bj] : acc;
    __syncthreads();
    if (tid == 0) {
        float n2 = 0.f;
        for (int i = 0; i < 128; ++i) n2 = n2 + s_d[i] * s_d[i];
        const float thr = sqrtf(n2) * 0.2f;
        n2 = 0.f;
        for (int i = 0; i < 128; ++i) {
            const float v = fminf(s_d[i], thr);
            n2 = n2 + v * v;
        }
        s_scale[0] = thr;
        s_scale[1] = 512.f / fmaxf(sqrtf(n2), 1.1920929e-7f);
    }
    __syncthreads();
    if (tid < 128) {
        const float v = fminf(s_d[tid], s_scale[0]) * s_scale[1];
        if (raw) raw[(long)k * 128 + tid] = v;
        desc[(long)k * 128 + tid] = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
    }
}

// (distance, index) pairs as one 64-bit key: smaller distance first, then the lower index
__device__ __forceinline__ void knn2_merge(unsigned long long& a1, unsigned long long& a2, unsigned long long b1, unsigned long long b2) {
    const unsigned long long lo = a1 < b1 ? a1 : b1, hi = a1 < b1 ? b1 : a1, nx = a1 < b1 ? a2 : b2;
    a1 = lo;
    a2 = hi < nx ? hi : nx;
}
__device__ __forceinline__ unsigned long long knn2_shfl_xor(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

#define KNN2_EMPTY 0x7fffffff7fffffffull

// one workgroup per row of des1 [n1][128]: idx [n1][2], dist [n1][2]; a missing neighbour (n2 < 2) is index -1 at distance INT_MAX
__global__ __launch_bounds__(256) void knn2_u8_kernel(const uint8_t* __restrict__ des1, const uint8_t* __restrict__ des2, int n2, int* __restrict__ idx,
                                                      int* __restrict__ dist) {
    __shared__ unsigned long long s_k[8];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t a[32];
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(des1 + (long)row * 128);
#pragma unroll
    for (int i = 0; i < 32; ++i) a[i] = pa[i];
    unsigned long long k1 = KNN2_EMPTY, k2 = KNN2_EMPTY;
    for (int j = tid; j < n2; j += 256) {
        const uint32_t* pb = reinterpret_cast<const uint32_t*>(des2 + (long)j * 128);
        int d = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const uint32_t b = pb[i];
#pragma unroll
            for (int s = 0; s < 32; s += 8) {
                const int t = (int)((a[i] >> s) & 255u) - (int)((b >> s) & 255u);
                d += t * t;
            }
        }
        const unsigned long long key = ((unsigned long long)(unsigned)d << 32) | (unsigned)j;
        if (key < k1) {
            k2 = k1;
            k1 = key;
        } else if (key < k2) {
            k2 = key;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long b1 = knn2_shfl_xor(k1, m), b2 = knn2_shfl_xor(k2, m);
        knn2_merge(k1, k2, b1, b2);
    }
    if (lane == 0) {
        s_k[2 * wave] = k1;
        s_k[2 * wave + 1] = k2;
    }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 4; ++v) knn2_merge(k1, k2, s_k[2 * v], s_k[2 * v + 1]);
        idx[2 * row] = k1 == KNN2_EMPTY ? -1 : (int)(unsigned)k1;
        idx[2 * row + 1] = k2 == KNN2_EMPTY ? -1 : (int)(unsigned)k2;
        dist[2 * row] = (int)(k1 >> 32);
        dist[2 * row + 1] = (int)(k2 >> 32);
    }
}
