// The half-precision forms of the 2-D 3x3 conv: the instantiations of conv2d_f16x3_tile.h over the model dtype of the maps (XDT, YDT) and
// the product count (NP) that the fused 2-D blocks use in half and autocast runs, behind mphip_conv2d_fwd_typed / mphip_conv2d_cat_fwd_typed.
// conv2d_f16x3.hip and conv2d_gn_f16x3.hip keep the fp32, three-product kernels: the fp32 entries are the typed ones with fp32 maps and three
// products, and conv2d_run (conv2d_run.hip), which knows the dtype rules, hands such a call to the launchers of those two units.
//
// One launch with one product computes
//     y = narrow_Y( act( unscale * sum round_f16(w * s_w) * round_f16(x * s_x)  + bias + widen(residual) ) )
// with the power-of-two scales s_w (pack header) and s_x (range descriptor) of the three-product launch, fp32 accumulation in the MFMA's
// order and one rounding at the store.  round_f16(w * s_w) is the hi plane, [part 0], of every slab of the ordinary pack.
//
// Instantiated (what model.ResBlock2DFused / ResBlockCustomFused launch with half_precision=True):
//   plain, one product   x fp32 | f16 | bf16 -> y fp32         the first conv of a ResBlock2D reads the block input in its own dtype
//                        x fp32 -> y fp32 | f16 | bf16         the second conv writes the block output in its dtype
//   two-source, one product   x1, x2 fp32 -> y fp32 | f16 | bf16
// The residual is fp32 or in y's dtype: a workgroup-uniform choice at run time, not an instantiation.
// LDS: 18432 (W hi) + 10368 (X hi) + 16 + 68 (the descriptor fold) (+ 128, two-source) bytes: five workgroups fit a CU's 160 KiB.  The
// kernels take 166-170 registers (a 168-register budget spills), so two waves per SIMD, as in the three-product kernels, bound the occupancy.
#include "conv2d_f16x3_tile.h"

namespace mphip {

__device__ unsigned long long g_conv2d_lp_saturated;

template <int XDT, int YDT, int NP>
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_lp_kernel(const dtype_t<XDT> *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                    const float *__restrict__ whdr, const float *__restrict__ bias, const void *__restrict__ residual, int residual_typed,
                    dtype_t<YDT> *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int relu, int tiles_w,
                    int tiles_h, unsigned nslots) {
    conv2d_k3_tile<false, &g_conv2d_lp_saturated, XDT, YDT, NP>(
        x, x_range, C2CatArgs{}, wslabs, whdr, bias, residual_typed ? nullptr : (const float *)residual, y, out_range, Ci, Co, H, W, relu,
        tiles_w, tiles_h, nslots, residual_typed ? (const dtype_t<YDT> *)residual : nullptr);
}

template <int YDT, int NP>
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_cat_lp_kernel(const float *__restrict__ x1, const float *__restrict__ x1_range, const C2CatArgs cat,
                        const _Float16 *__restrict__ wslabs, const float *__restrict__ whdr, const float *__restrict__ bias,
                        const void *__restrict__ residual, int residual_typed, dtype_t<YDT> *__restrict__ y, float *__restrict__ out_range,
                        int C1, int Co, int H, int W, int relu, int tiles_w, int tiles_h, unsigned nslots) {
    conv2d_k3_tile<true, &g_conv2d_lp_saturated, MPHIP_DTYPE_F32, YDT, NP>(
        x1, x1_range, cat, wslabs, whdr, bias, residual_typed ? nullptr : (const float *)residual, y, out_range, C1, Co, H, W, relu, tiles_w,
        tiles_h, nslots, residual_typed ? (const dtype_t<YDT> *)residual : nullptr);
}

int conv2d_lp_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_lp_saturated, count, reset); }

void conv2d_lp_launch(const C2Call &c, const C2Grid &g) {
    const _Float16 *slabs = (const _Float16 *)((const char *)c.w_packed + 16);
    const int rt = c.residual && c.residual_dtype != MPHIP_DTYPE_F32 ? 1 : 0;
    const C2CatArgs cat{c.aff1, (const float *)c.x2, c.aff2, c.x2_range, c.C2, c.relu1 ? 1 : 0, c.relu2 ? 1 : 0};
#define LP_LAUNCH(XD, YD)                                                                                                                \
    hipLaunchKernelGGL((conv2d_k3_lp_kernel<XD, YD, 1>), g.grid, dim3(C2_NTHR), 0, c.stream, (const dtype_t<XD> *)c.x1, c.x1_range, slabs, \
                       (const float *)c.w_packed, c.bias, c.residual, rt, (dtype_t<YD> *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.relu,   \
                       g.tiles_w, g.tiles_h, g.nslots)
#define LP_CAT_LAUNCH(YD)                                                                                                                \
    hipLaunchKernelGGL((conv2d_k3_cat_lp_kernel<YD, 1>), g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range, cat, slabs,  \
                       (const float *)c.w_packed, c.bias, c.residual, rt, (dtype_t<YD> *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.relu,   \
                       g.tiles_w, g.tiles_h, g.nslots)
    if (c.form == C2_CAT) {
        if (c.y_dtype == MPHIP_DTYPE_F32) LP_CAT_LAUNCH(MPHIP_DTYPE_F32);
        else if (c.y_dtype == MPHIP_DTYPE_F16) LP_CAT_LAUNCH(MPHIP_DTYPE_F16);
        else LP_CAT_LAUNCH(MPHIP_DTYPE_BF16);
    } else if (c.y_dtype == MPHIP_DTYPE_F32) {
        if (c.x_dtype == MPHIP_DTYPE_F32) LP_LAUNCH(MPHIP_DTYPE_F32, MPHIP_DTYPE_F32);
        else if (c.x_dtype == MPHIP_DTYPE_F16) LP_LAUNCH(MPHIP_DTYPE_F16, MPHIP_DTYPE_F32);
        else LP_LAUNCH(MPHIP_DTYPE_BF16, MPHIP_DTYPE_F32);
    } else if (c.y_dtype == MPHIP_DTYPE_F16) {
        LP_LAUNCH(MPHIP_DTYPE_F32, MPHIP_DTYPE_F16);
    } else {
        LP_LAUNCH(MPHIP_DTYPE_F32, MPHIP_DTYPE_BF16);
    }
#undef LP_LAUNCH
#undef LP_CAT_LAUNCH
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_fwd_typed(const void *x, int x_dtype, const float *x_range, const void *w_packed, const float *bias,
                                      const void *residual, int residual_dtype, void *y, int y_dtype, float *out_range, int N, int Ci,
                                      int Co, int H, int W, int relu, int products, void *workspace, size_t workspace_bytes, void *stream) {
    C2Call c = c2_call_f32("conv2d_fwd_typed", C2_PLAIN, x, x_range, w_packed, bias, residual, y, out_range, N, Ci, Co, H, W, relu, workspace,
                           workspace_bytes, stream);
    c.x_dtype = x_dtype, c.residual_dtype = residual_dtype, c.y_dtype = y_dtype, c.products = products;
    return conv2d_run(c);
}

extern "C" int mphip_conv2d_cat_fwd_typed(const void *x1, int x_dtype, const float *affine1, int relu1, const float *x1_range, int C1,
                                          const void *x2, const float *affine2, int relu2, const float *x2_range, int C2,
                                          const void *w_packed, const float *bias, const void *residual, int residual_dtype, void *y,
                                          int y_dtype, float *out_range, int N, int Co, int H, int W, int relu, int products,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    C2Call c = c2_call_f32("conv2d_cat_fwd_typed", C2_CAT, x1, x1_range, w_packed, bias, residual, y, out_range, N, C1, Co, H, W, relu, workspace,
                           workspace_bytes, stream);
    c.aff1 = affine1, c.relu1 = relu1;
    c.x2 = x2, c.aff2 = affine2, c.relu2 = relu2, c.x2_range = x2_range, c.C2 = C2;
    c.x_dtype = x_dtype, c.residual_dtype = residual_dtype, c.y_dtype = y_dtype, c.products = products;
    return conv2d_run(c);
}
