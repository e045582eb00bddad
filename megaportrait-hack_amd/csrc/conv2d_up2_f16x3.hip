// The 2-D 3x3 f16x3 conv with a bilinear x2 up-sample folded in (conv2d_f16x3_tile.h, UP = 1 and UP = 2), for G2d's three
// Sequential(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True), ResBlock2D) stages at inference:
//     y1  = relu( conv1'(up2(x)) )                        conv2d_k3_up2_f16x3_kernel     the source is up-sampled while it is staged
//     out = relu( conv2'(y1) + up2(shortcut'(x)) )        conv2d_k3_resup2_f16x3_kernel  the residual is up-sampled in the epilogue
// (a 1x1 conv and a bilinear resample commute, so the shortcut runs on the LOW-resolution map) and up2(x) is never written to memory.
//
// up2(x) for x [N,C,h,w] is [N,C,2h,2w].  For output row i:   num = i * (h - 1),  den = 2h - 1   (h == 1: num = 0, den = 1),
//     i0 = num div den,   lambda = float(num mod den) / float(den)   (one correctly rounded fp32 division),   i1 = min(i0 + 1, h - 1);
// columns get j0, j1, mu the same way from w.  The value is horizontal first,
//     top = x[i0,j0] * (1 - mu) + x[i0,j1] * mu,   bot = x[i1,j0] * (1 - mu) + x[i1,j1] * mu,   u = top * (1 - lambda) + bot * lambda,
// every product, sum and 1 - . rounded to fp32 on its own (-ffp-contract=off; up2_blend): F.interpolate(align_corners=True) restated
// with exact integer coordinates (model.up2_reference is the same expression in torch ops, and the kernels reproduce its bits).
// u is a convex blend of four inputs up to rounding, so the range descriptor of x is a bound of up2(x): no up-sampled map is scanned.
//
// Up-sampled source.  A 16 x 16 output tile's 18 x 18 halo blends from at most 10 x 10 source pixels per channel: per 16-channel chunk
// that patch is loaded (7 loads per thread), parked in LDS (6400 B) and blended into the hi / lo X planes when the chunk is written.
// Patch rows and columns are clamped at h - 1 and w - 1; zero padding and the ragged edge are zeros OF THE UP-SAMPLED MAP.
// Up-sampled residual.  Staging is the plain one; `v += residual[oi]` becomes the blend of four loads of r [N,Co,H/2,W/2].
// Tile, LDS layout of W and X, MFMA sequence, pack (mphip_pack_conv2d_weight), epilogue, out_range and saturation counting are
// conv2d_f16x3.hip's; with the same descriptor the results are, bit for bit, conv2d(up2_reference(x)) and conv2d(x, residual =
// up2_reference(r)).  fp32 maps and three products only.
#include "conv2d_f16x3_tile.h"

namespace mphip {

__device__ unsigned long long g_conv2d_up2_saturated;

// H, W: the OUTPUT map (x is [N,Ci,H/2,W/2])
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_up2_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                           const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                           float *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int relu, int tiles_w,
                           int tiles_h, unsigned nslots) {
    conv2d_k3_tile<false, &g_conv2d_up2_saturated, MPHIP_DTYPE_F32, MPHIP_DTYPE_F32, 3, 1>(x, x_range, C2CatArgs{}, wslabs, whdr, bias, residual,
                                                                                          y, out_range, Ci, Co, H, W, relu, tiles_w, tiles_h,
                                                                                          nslots);
}

// residual: r [N,Co,H/2,W/2], never NULL; H, W even
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_resup2_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                              const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                              float *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int relu, int tiles_w,
                              int tiles_h, unsigned nslots) {
    conv2d_k3_tile<false, &g_conv2d_up2_saturated, MPHIP_DTYPE_F32, MPHIP_DTYPE_F32, 3, 2>(x, x_range, C2CatArgs{}, wslabs, whdr, bias, residual,
                                                                                          y, out_range, Ci, Co, H, W, relu, tiles_w, tiles_h,
                                                                                          nslots);
}

int conv2d_up2_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_up2_saturated, count, reset); }

// h, w: the LOW-resolution map; the rule is c2_supported on the doubled one
bool c2_up2_supported(int N, int Ci, int Co, int h, int w) {
    if (h < 1 || w < 1 || h > (1 << 29) || w > (1 << 29)) return false;
    return c2_supported(N, Ci, Co, 2 * h, 2 * w);
}

void conv2d_up2_launch(const C2Call &c, const C2Grid &g) {
    const _Float16 *slabs = (const _Float16 *)((const char *)c.w_packed + 16);
    if (c.form == C2_UP2)   // c.H, c.W: the source map
        hipLaunchKernelGGL(conv2d_k3_up2_f16x3_kernel, g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range, slabs,
                           (const float *)c.w_packed, c.bias, (const float *)c.residual, (float *)c.y, c.out_range, c.C1, c.Co, 2 * c.H,
                           2 * c.W, c.relu, g.tiles_w, g.tiles_h, g.nslots);
    else
        hipLaunchKernelGGL(conv2d_k3_resup2_f16x3_kernel, g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range, slabs,
                           (const float *)c.w_packed, c.bias, (const float *)c.residual, (float *)c.y, c.out_range, c.C1, c.Co, c.H, c.W,
                           c.relu, g.tiles_w, g.tiles_h, g.nslots);
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_up2_supported(int N, int Ci, int Co, int h, int w) { return c2_up2_supported(N, Ci, Co, h, w) ? 1 : 0; }

extern "C" size_t mphip_conv2d_up2_workspace_bytes(int N, int Ci, int Co, int h, int w) {
    return c2_up2_supported(N, Ci, Co, h, w) ? c2_workspace_bytes(1) : 0;   // the library-computed descriptor of x (x_range == NULL)
}

extern "C" int mphip_conv2d_up2_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, const float *residual,
                                    float *y, float *out_range, int N, int Ci, int Co, int h, int w, int relu, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    return conv2d_run(c2_call_f32("conv2d_up2_fwd", C2_UP2, x, x_range, w_packed, bias, residual, y, out_range, N, Ci, Co, h, w, relu, workspace,
                                  workspace_bytes, stream));
}

extern "C" int mphip_conv2d_resup2_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias,
                                       const float *residual_lowres, float *y, float *out_range, int N, int Ci, int Co, int H, int W,
                                       int relu, void *workspace, size_t workspace_bytes, void *stream) {
    return conv2d_run(c2_call_f32("conv2d_resup2_fwd", C2_RESUP2, x, x_range, w_packed, bias, residual_lowres, y, out_range, N, Ci, Co, H, W,
                                  relu, workspace, workspace_bytes, stream));
}
