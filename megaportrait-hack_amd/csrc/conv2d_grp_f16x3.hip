// The grouped form of the 2-D 3x3 f16x3 conv (conv2d_f16x3_tile.h, GRP = true), for the thirteen groups = 2 blocks of 6DRepNet's
// RepVGG-B1g2 backbone in deploy form (3x3 conv + bias + ReLU each; model.RepVGGBlockFused):
//     y[n, g*Cog + o, h, w] = act( sum_{c < Cig, dy, dx} wt[g*Cog + o, c, dy, dx] * x[n, g*Cig + c, h+dy-1, w+dx-1] + bias[g*Cog + o] (+ residual) )
//     Cig = Ci / groups,   Cog = Co / groups,   wt [Co, Cig, 3, 3] (torch's grouped layout)
//
// Pack.  The ordinary one, mphip_pack_conv2d_weight(w, packed, Co, Cig): c2_cots(Co) x Cig / 16 slabs, one header scale for the whole weight.
// Grid.  The ordinary one, tiles x c2_cots(Co).  Cog % 64 == 0, so a workgroup's 64 output channels lie in one group, cot / (Cog / 64);
// its K loop runs over the Cig / 16 chunks that start at channel g * Cig of an image whose stride is Ci channels.  LDS layout, MFMA
// sequence per chunk, epilogue, out_range and saturation counting are conv2d_f16x3.hip's.  A group's sum is that of the dense conv whose
// [Co, Ci, 3, 3] weight has the group blocks on its diagonal and exact zeros elsewhere, less the chunks that add those zeros: with the
// same descriptor of x and the same max|w| the launch writes the bits of mphip_conv2d_fwd on that dense weight.
// fp32 maps, stride 1, one source and three products only.  groups == 1 is the plain kernel's launch (conv2d_grouped_launch).
#include "conv2d_f16x3_tile.h"

namespace mphip {

__device__ unsigned long long g_conv2d_grp_saturated;

// Ci: channels of x (the image stride); cig = Ci / groups; cots_per_group = Co / groups / 64
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_grp_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                           const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                           float *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int relu, int tiles_w,
                           int tiles_h, unsigned nslots, int cig, int cots_per_group) {
    conv2d_k3_tile<false, &g_conv2d_grp_saturated, MPHIP_DTYPE_F32, MPHIP_DTYPE_F32, 3, 0, true>(x, x_range, C2CatArgs{}, wslabs, whdr, bias,
                                                                                                residual, y, out_range, Ci, Co, H, W, relu,
                                                                                                tiles_w, tiles_h, nslots, nullptr, cig,
                                                                                                cots_per_group);
}

int conv2d_grp_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_grp_saturated, count, reset); }

// groups == 1: the plain rule.  Else whole groups, whole 16-channel chunks per group, and 64-channel output tiles that never straddle two.
bool c2_grouped_supported(int N, int Ci, int Co, int H, int W, int groups) {
    if (groups < 1 || !c2_supported(N, Ci, Co, H, W)) return false;
    if (groups == 1) return true;
    if (Ci % groups || Co % groups) return false;
    return (Ci / groups) % C2_KC == 0 && (Co / groups) % C2_COT == 0;
}

void conv2d_grouped_launch(const C2Call &c, const C2Grid &g) {
    if (c.groups == 1) return conv2d_plain_launch(c, g);
    hipLaunchKernelGGL(conv2d_k3_grp_f16x3_kernel, g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range,
                       (const _Float16 *)((const char *)c.w_packed + 16), (const float *)c.w_packed, c.bias, (const float *)c.residual,
                       (float *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.relu, g.tiles_w, g.tiles_h, g.nslots, c.C1 / c.groups,
                       c.Co / c.groups / C2_COT);
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_grouped_supported(int N, int Ci, int Co, int H, int W, int groups) {
    return c2_grouped_supported(N, Ci, Co, H, W, groups) ? 1 : 0;
}

extern "C" size_t mphip_conv2d_grouped_workspace_bytes(int N, int Ci, int Co, int H, int W, int groups) {
    return c2_grouped_supported(N, Ci, Co, H, W, groups) ? c2_workspace_bytes(1) : 0;   // the library-computed descriptor of x (x_range == NULL)
}

extern "C" int mphip_conv2d_grouped_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, const float *residual,
                                        float *y, float *out_range, int N, int Ci, int Co, int H, int W, int groups, int relu,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    C2Call c = c2_call_f32("conv2d_grouped_fwd", C2_GROUPED, x, x_range, w_packed, bias, residual, y, out_range, N, Ci, Co, H, W, relu, workspace,
                           workspace_bytes, stream);
    c.groups = groups;
    return conv2d_run(c);
}
