// The 3-D front end's entries of libfreefine_hip.so: the point-cloud warp (ffn_splat_*; kernels: splat.h) and the GeoDiffuser warp (ffn_geo_project,
// ffn_splat_composite, ffn_mesh_cover; kernels: geowarp.h).  Host-side launch glue only, on the caller's stream.
#include "capi_common.h"
#include "splat.h"
#include "geowarp.h"

// ---- point-cloud warp of the 3-D front end (splat.h) ----------------------------------------------------------------
extern "C" int ffn_splat_lift(void* stream, const float* depth, const int* idx, float* pts, int n, int W, int H, float fx, float fy) {
    REQUIRE(depth && idx && pts, "splat_lift: null operand");
    REQUIRE(n > 0 && W > 0 && H > 0 && (long)W * H < (1l << 31) && fx != 0.f && fy != 0.f, "splat_lift: bad shape / focal length");
    LAUNCH(splat_lift_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth, idx, pts, n, W, H, fx, fy);
    return check_launch("splat_lift");
}
extern "C" int ffn_splat_project(void* stream, const float* pts, float* proj, int n, const ffn_splat_xform* x) {
    REQUIRE(pts && proj && x, "splat_project: null operand");
    REQUIRE(n > 0, "splat_project: empty cloud");
    SplatXform X;
    for (int i = 0; i < 3; ++i) { X.c[i] = x->center[i]; X.t[i] = x->translate[i]; X.s[i] = x->scale[i]; }
    for (int i = 0; i < 9; ++i) X.R[i] = x->rotate[i];
    REQUIRE(x->tan_half_fov > 0.f, "splat_project: tan_half_fov must be positive");
    X.inv_tan = 1.f / x->tan_half_fov;
    LAUNCH(splat_project_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pts, proj, n, X);
    return check_launch("splat_project");
}
extern "C" int ffn_splat_bin(void* stream, int fill, const float* proj, int n, float radius, int W, int H, int* counts, const int* offs, int* list) {
    REQUIRE(proj && counts, "splat_bin: null operand");
    REQUIRE(!fill || (offs && list), "splat_bin: the filling pass needs the tile offsets and the list");
    REQUIRE(n > 0 && W > 0 && H > 0 && radius > 0.f, "splat_bin: bad shape / radius");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (fill) LAUNCH(splat_bin_kernel<true>, dim3(grid_for(n)), dim3(256), 0, s, proj, n, radius, W, H, counts, offs, list);
    else LAUNCH(splat_bin_kernel<false>, dim3(grid_for(n)), dim3(256), 0, s, proj, n, radius, W, H, counts, offs, list);
    return check_launch("splat_bin");
}
extern "C" int ffn_splat_render(void* stream, const float* proj, const float* rgb, const int* offs, const int* list, float radius, int K, int W, int H,
                                float* image, int* idx_sum, uint8_t* covered) {
    REQUIRE(proj && rgb && offs && list && image && idx_sum && covered, "splat_render: null operand");
    REQUIRE(K >= 1 && K <= 32, "splat_render: points per pixel K=%d out of range (1 .. 32)", K);
    REQUIRE(W > 0 && H > 0 && radius > 0.f, "splat_render: bad shape / radius");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    if (K <= 8) LAUNCH(splat_render_kernel<8>, dim3(tiles), dim3(256), 0, s, proj, rgb, offs, list, radius, K, W, H, image, idx_sum, covered);
    else if (K <= 16) LAUNCH(splat_render_kernel<16>, dim3(tiles), dim3(256), 0, s, proj, rgb, offs, list, radius, K, W, H, image, idx_sum, covered);
    else LAUNCH(splat_render_kernel<32>, dim3(tiles), dim3(256), 0, s, proj, rgb, offs, list, radius, K, W, H, image, idx_sum, covered);
    return check_launch("splat_render");
}
extern "C" int ffn_splat_ids(void* stream, const float* proj, const int* offs, const int* list, float radius, int K, int W, int H, int* ids) {
    REQUIRE(proj && offs && list && ids, "splat_ids: null operand");
    REQUIRE(K >= 1 && K <= 32, "splat_ids: points per pixel K=%d out of range (1 .. 32)", K);
    REQUIRE(W > 0 && H > 0 && radius > 0.f, "splat_ids: bad shape / radius");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    if (K <= 8) LAUNCH(splat_ids_kernel<8>, dim3(tiles), dim3(256), 0, s, proj, offs, list, radius, K, W, H, ids);
    else if (K <= 16) LAUNCH(splat_ids_kernel<16>, dim3(tiles), dim3(256), 0, s, proj, offs, list, radius, K, W, H, ids);
    else LAUNCH(splat_ids_kernel<32>, dim3(tiles), dim3(256), 0, s, proj, offs, list, radius, K, W, H, ids);
    return check_launch("splat_ids");
}
extern "C" int ffn_splat_correspond(void* stream, const float* proj, const int* idx, int n, int W, int H, const int* ids, int K, float* map,
                                    uint8_t* visible) {
    REQUIRE(proj && idx && map, "splat_correspond: null operand");
    REQUIRE(!visible || ids, "splat_correspond: the visibility output needs the ids of ffn_splat_ids");
    REQUIRE(n >= 0 && W > 0 && H > 0 && (long)W * H < (1l << 31), "splat_correspond: bad shape");
    REQUIRE(K >= 1 && K <= 32, "splat_correspond: points per pixel K=%d out of range (1 .. 32)", K);
    if (n == 0) return FFN_OK;
    LAUNCH(splat_correspond_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), proj, idx, n, W, H, ids, K, map, visible);
    return check_launch("splat_correspond");
}

// ---- the GeoDiffuser warp of the reference's GeoBench-3D step 2 (geowarp.h) ---------------------------------------------
extern "C" int ffn_geo_project(void* stream, const float* depth, const float* pose, float focal, int H, int W, float* tcoords, float* proj) {
    REQUIRE(depth && pose && tcoords && proj, "geo_project: null operand");
    REQUIRE(H == W, "geo_project: the image must be square (%d x %d): the reference takes sqrt(N) for the side", H, W);
    REQUIRE(H >= 2 && H <= 4096 && focal > 0.f, "geo_project: side %d outside 2 .. 4096, or focal length <= 0", H);
    GeoPose P;
    for (int a = 0; a < 12; ++a) P.m[a] = pose[a];
    LAUNCH(geo_project_kernel, dim3(grid_for((long)H * W)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), depth, P, focal, H, tcoords, proj);
    return check_launch("geo_project");
}
extern "C" int ffn_splat_composite(void* stream, const float* proj, const float* feat, const int* offs, const int* list, float radius, float tau, int K,
                                   int C, int H, int W, int round_half, float* out) {
    REQUIRE(proj && feat && offs && list && out, "splat_composite: null operand");
    REQUIRE(H == W, "splat_composite: the image must be square (%d x %d)", H, W);
    REQUIRE(H >= 1 && H <= 4096, "splat_composite: side %d outside 1 .. 4096", H);
    REQUIRE(K >= 1 && K <= 32, "splat_composite: points per pixel K=%d out of range (1 .. 32)", K);
    REQUIRE(C >= 1 && C <= 8, "splat_composite: C=%d feature channels out of range (1 .. 8)", C);
    REQUIRE(radius > 0.f && tau > 0.f, "splat_composite: radius and tau must be positive");
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (K <= 8) LAUNCH(geo_composite_kernel<8>, dim3(tiles), dim3(256), 0, s, proj, feat, offs, list, radius, tau, K, C, W, H, round_half, out);
    else if (K <= 16) LAUNCH(geo_composite_kernel<16>, dim3(tiles), dim3(256), 0, s, proj, feat, offs, list, radius, tau, K, C, W, H, round_half, out);
    else LAUNCH(geo_composite_kernel<32>, dim3(tiles), dim3(256), 0, s, proj, feat, offs, list, radius, tau, K, C, W, H, round_half, out);
    return check_launch("splat_composite");
}
extern "C" int ffn_mesh_cover(void* stream, const float* tcoords, const uint8_t* mask, int H, int W, uint8_t* cover) {
    REQUIRE(tcoords && mask && cover, "mesh_cover: null operand");
    REQUIRE(H == W, "mesh_cover: the image must be square (%d x %d)", H, W);
    REQUIRE(H >= 2 && H <= 4096, "mesh_cover: side %d outside 2 .. 4096", H);
    LAUNCH(geo_mesh_cover_kernel, dim3(grid_for(2l * (H - 1) * (W - 1))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tcoords, mask, H, cover);
    return check_launch("mesh_cover");
}
