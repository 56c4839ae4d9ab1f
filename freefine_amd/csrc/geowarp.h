// The GeoDiffuser warp: step 2 of the reference's GeoBench-3D data preparation (evaluation/FreeFine/get_3d_transform_correspondence.py:207-289),
// which renders coarse3d_depth_anything_blended/, mesh_mask/, md_mask/ and correspondence/ through
// evaluation/GeoDiffuser/GeoDiffuser/utils/{ui_utils2.py:504-593, 685-743; vis_utils.py:404-479; warp_utils.py:28-176, 235-298, 304-399, 407-492, 599-645}.
//
//   project    (warp_utils.py:738-747, 599-645): EVERY pixel (i, j) of the S x S image is lifted with pixel2cam, K^-1 (j, i, 1) depth with
//              K = (f, f, S/2, S/2), moved by a 3 x 4 pose, put through K again; Z is clamped at 1e-3 and X_norm = 2 (X / Z) / (S - 1) - 1
//              (likewise Y).  tcoords = (X_norm, Y_norm, Z) is the reference's t_coords; proj = (-X_norm, -Y_norm, Z, 0) is the same point in
//              pytorch3d's frame (warp_utils.py:90-91), the convention splat_bin_kernel / splat_select_topk read.
//   composite  (warp_utils.py:72-176, SynSin's z-buffer splat): the K nearest points by z among those with d2 < r2 at every pixel (splat.h's
//              binning and selection, unchanged), alpha = (1 - sqrt(clamp(d2 / r2, 1e-3, 1)))^tau, front-to-back alpha_composite of C feature
//              channels, optionally rounded once through fp16 (`.to(torch.half)`, :176).
//   mesh cover (warp_utils.py:235-298, 304-399): the mask's pixels are the vertices of a mesh with two triangles per 2 x 2 quad
//              (create_triangles: (tl, tr, bl) and (bl, tr, br), each kept when its own three vertices are in the mask); cover = 1 where a
//              pixel centre lies strictly inside a projected triangle.
//
// PARITY: project and the triangle topology are pinned to the reference's code (tests/golden/g18_geodiffuser_coords.npz).  The two rasterisers
// restate pytorch3d's published rasterize_points / rasterize_meshes (pytorch3d is not in the build image): unpinned, held to tests/geowarp_ref.py.
#pragma once
#include "splat.h"

struct GeoPose {
    float m[12];              // 3 x 4, row-major: p' = m[:, :3] p + m[:, 3]
};

__global__ __launch_bounds__(256) void geo_project_kernel(const float* __restrict__ depth, const GeoPose P, float focal, int S,
                                                          float* __restrict__ tcoords, float* __restrict__ proj) {
    const int n = S * S;
    const float c = (float)S * 0.5f, inv_f = 1.f / focal, off = -c / focal;        // K^-1 = [1/f 0 -c/f; 0 1/f -c/f; 0 0 1]
    const float s1 = (float)(S - 1);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int i = p / S, j = p - i * S;
        const float d = depth[p];
        const float x = ((float)j * inv_f + off) * d, y = ((float)i * inv_f + off) * d, z = d;
        const float q0 = P.m[0] * x + P.m[1] * y + P.m[2] * z + P.m[3];
        const float q1 = P.m[4] * x + P.m[5] * y + P.m[6] * z + P.m[7];
        const float q2 = P.m[8] * x + P.m[9] * y + P.m[10] * z + P.m[11];
        const float X = focal * q0 + c * q2, Y = focal * q1 + c * q2;
        const float Z = fmaxf(q2, 1e-3f);
        const float xn = 2.f * (X / Z) / s1 - 1.f, yn = 2.f * (Y / Z) / s1 - 1.f;
        tcoords[3l * p] = xn;
        tcoords[3l * p + 1] = yn;
        tcoords[3l * p + 2] = Z;
        *reinterpret_cast<f32x4*>(proj + 4l * p) = f32x4{-xn, -yn, Z, 0.f};
    }
}

// one workgroup per tile, one lane per pixel: splat_render_kernel's frame with SynSin's weights and C feature channels
template <int KMAX>
__global__ __launch_bounds__(256) void geo_composite_kernel(const float* __restrict__ proj, const float* __restrict__ feat, const int* __restrict__ offs,
                                                            const int* __restrict__ list, float radius, float tau, int K, int C, int W, int H,
                                                            int round_half, float* __restrict__ out) {
    __shared__ f32x4 s_pt[256];
    const int TW = (W + 15) >> 4;
    const int tile = blockIdx.x, ty = tile / TW, tx = tile - ty * TW;
    const int row = ty * 16 + (threadIdx.x >> 4), col = tx * 16 + (threadIdx.x & 15);
    const bool live = row < H && col < W;
    const float xf = splat_pix_to_ndc(W - 1 - col, W, H), yf = splat_pix_to_ndc(H - 1 - row, H, W);
    const float r2 = radius * radius;
    float qz[KMAX], qd[KMAX];
    int qi[KMAX];
    splat_select_topk<KMAX>(proj, list, offs[tile], offs[tile + 1], K, live, xf, yf, r2, s_pt, qz, qd, qi);
    if (!live) return;
    float cum = 1.f, o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K && qi[k] != 0x7fffffff) {
            const float q = fminf(fmaxf(qd[k] / r2, 1e-3f), 1.f);
            float a = 1.f - sqrtf(q);
            if (tau != 1.f) a = powf(a, tau);
            const float w = cum * a;
            const float* f = feat + (long)qi[k] * C;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < C) o[c] += w * f[c];
            cum *= 1.f - a;
        }
    }
    float* dst = out + ((long)row * W + col) * C;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < C) dst[c] = round_half ? (float)(_Float16)o[c] : o[c];
}

// pytorch3d's EdgeFunctionForward(p, a, b)
__device__ __forceinline__ float geo_edge(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// one lane per triangle (2 per 2 x 2 quad), over its bounding box clipped to the image.  Vertices in pytorch3d's frame (x, y negated), pixel
// centres as the splat kernels place them.  The only write is the constant 1 (a vector byte store): order does not matter.
__global__ __launch_bounds__(256) void geo_mesh_cover_kernel(const float* __restrict__ tcoords, const uint8_t* __restrict__ mask, int S,
                                                             uint8_t* __restrict__ cover) {
    const int Q = S - 1, n = 2 * Q * Q;
    const float Sf = (float)S;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
        const int second = t >= Q * Q, q = second ? t - Q * Q : t;
        const int i = q / Q, j = q - i * Q;
        const int tl = i * S + j, tr = tl + 1, bl = tl + S, br = bl + 1;
        const int a = second ? bl : tl, b = tr, c = second ? br : bl;
        if (!mask[a] || !mask[b] || !mask[c]) continue;
        const float ax = -tcoords[3l * a], ay = -tcoords[3l * a + 1], az = tcoords[3l * a + 2];
        const float bx = -tcoords[3l * b], by = -tcoords[3l * b + 1], bz = tcoords[3l * b + 2];
        const float cx = -tcoords[3l * c], cy = -tcoords[3l * c + 1], cz = tcoords[3l * c + 2];
        if (fmaxf(az, fmaxf(bz, cz)) < 0.f) continue;                              // entirely behind the camera
        const float face = geo_edge(ax, ay, bx, by, cx, cy);
        if (!(face > 1e-8f || face < -1e-8f)) continue;                           // zero area (or NaN)
        const float xmin = fminf(ax, fminf(bx, cx)), xmax = fmaxf(ax, fmaxf(bx, cx));
        const float ymin = fminf(ay, fminf(by, cy)), ymax = fmaxf(ay, fmaxf(by, cy));
        if (!(fabsf(xmin) < 1e30f) || !(fabsf(xmax) < 1e30f) || !(fabsf(ymin) < 1e30f) || !(fabsf(ymax) < 1e30f)) continue;
        // xf(col) = 1 - (2 col + 1) / S  ->  col = ((1 - xf) S - 1) / 2, decreasing in xf; one pixel of margin, clipped to the image
        const float c_lo = fminf(fmaxf(((1.f - xmax) * Sf - 1.f) * 0.5f - 1.f, 0.f), Sf - 1.f);
        const float c_hi = fminf(fmaxf(((1.f - xmin) * Sf - 1.f) * 0.5f + 1.f, -1.f), Sf - 1.f);
        const float r_lo = fminf(fmaxf(((1.f - ymax) * Sf - 1.f) * 0.5f - 1.f, 0.f), Sf - 1.f);
        const float r_hi = fminf(fmaxf(((1.f - ymin) * Sf - 1.f) * 0.5f + 1.f, -1.f), Sf - 1.f);
        const int col0 = (int)floorf(c_lo), col1 = (int)ceilf(c_hi), row0 = (int)floorf(r_lo), row1 = (int)ceilf(r_hi);
        const float area = geo_edge(cx, cy, ax, ay, bx, by) + 1e-8f;
        for (int row = row0; row <= row1 && row < S; ++row) {
            const float py = splat_pix_to_ndc(S - 1 - row, S, S);
            for (int col = col0; col <= col1 && col < S; ++col) {
                const float px = splat_pix_to_ndc(S - 1 - col, S, S);
                const float w0 = geo_edge(px, py, bx, by, cx, cy) / area;
                const float w1 = geo_edge(px, py, cx, cy, ax, ay) / area;
                const float w2 = geo_edge(px, py, ax, ay, bx, by) / area;
                if (w0 > 0.f && w1 > 0.f && w2 > 0.f) cover[(long)row * S + col] = 1;
            }
        }
    }
}
