// The two-source, normalise-while-staging form of the 2-D 3x3 f16x3 conv (conv2d_f16x3_tile.h, CAT = true), for Eapp's ResBlock_Custom
// (reference model.py:110-123):
//     out = conv( relu(GN32(conv_ws( relu(GN32(x)) ))) ) + conv_res(x)
// With a = relu(GN32(t)), conv(a) + conv_res(x) is ONE conv over the channel concatenation [a ; x] with the weights [W_conv | W_res]
// and the bias b_conv + b_res, so a block is two launches of this kernel:
//     t   = cat_fwd(x1 = x, table(x), relu)                    weights: conv_ws's, standardised by the caller
//     out = cat_fwd(x1 = t, table(t), relu;  x2 = x as it is)  weights: [W_conv | W_res]
// and neither activated map, nor the skip branch, nor the concatenation is written to memory.  The statistics and the tables come from
// mphip_groupnorm_stats and mphip_groupnorm_affine_table (launches of their own); this unit computes no statistics.
//
// Tile, LDS layout, MFMA sequence, epilogue and the packed weights (mphip_pack_conv2d_weight with Ci = C1 + C2) are conv2d_f16x3.hip's.
// Without a table and a second source the kernel stages what conv2d_k3_f16x3_kernel stages: same bits.
#include "conv2d_f16x3_tile.h"

namespace mphip {

__device__ unsigned long long g_conv2d_gn_saturated;

__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_cat_f16x3_kernel(const float *__restrict__ x1, const float *__restrict__ x1_range, const C2CatArgs cat,
                           const _Float16 *__restrict__ wslabs, const float *__restrict__ whdr, const float *__restrict__ bias,
                           const float *__restrict__ residual, float *__restrict__ y, float *__restrict__ out_range, int C1, int Co, int H,
                           int W, int relu, int tiles_w, int tiles_h, unsigned nslots) {
    conv2d_k3_tile<true, &g_conv2d_gn_saturated>(x1, x1_range, cat, wslabs, whdr, bias, residual, y, out_range, C1, Co, H, W, relu, tiles_w,
                                                 tiles_h, nslots);
}

int conv2d_gn_f16x3_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_gn_saturated, count, reset); }

static bool c2_cat_supported(int N, int C1, int C2, int Co, int H, int W) {
    if (C1 < C2_KC || C1 % C2_KC || C2 < 0 || C2 % C2_KC || C2 > (1 << 20) || C1 > (1 << 20)) return false;
    return c2_supported(N, C1 + C2, Co, H, W);   // (each source alone then has fewer than 2^31 elements too)
}

void conv2d_cat_launch(const C2Call &c, const C2Grid &g) {
    const C2CatArgs cat{c.aff1, (const float *)c.x2, c.aff2, c.x2_range, c.C2, c.relu1 ? 1 : 0, c.relu2 ? 1 : 0};
    hipLaunchKernelGGL(conv2d_k3_cat_f16x3_kernel, g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range, cat,
                       (const _Float16 *)((const char *)c.w_packed + 16), (const float *)c.w_packed, c.bias, (const float *)c.residual,
                       (float *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.relu, g.tiles_w, g.tiles_h, g.nslots);
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_cat_supported(int N, int C1, int C2, int Co, int H, int W) { return c2_cat_supported(N, C1, C2, Co, H, W) ? 1 : 0; }

extern "C" size_t mphip_conv2d_cat_workspace_bytes(int N, int C1, int C2, int Co, int H, int W) {
    return c2_cat_supported(N, C1, C2, Co, H, W) ? c2_workspace_bytes(2) : 0;   // a descriptor per source (x1_range / x2_range == NULL)
}

extern "C" int mphip_conv2d_cat_fwd(const float *x1, const float *affine1, int relu1, const float *x1_range, int C1, const float *x2,
                                    const float *affine2, int relu2, const float *x2_range, int C2, const void *w_packed, const float *bias,
                                    const float *residual, float *y, float *out_range, int N, int Co, int H, int W, int relu,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    return mphip_conv2d_cat_fwd_typed(x1, MPHIP_DTYPE_F32, affine1, relu1, x1_range, C1, x2, affine2, relu2, x2_range, C2, w_packed, bias,
                                      residual, MPHIP_DTYPE_F32, y, MPHIP_DTYPE_F32, out_range, N, Co, H, W, relu, 3, workspace,
                                      workspace_bytes, stream);
}
