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

// [p, p + bytes) and [q, q + qbytes) share a byte
static bool c2_overlap(const void *p, size_t bytes, const void *q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return q != nullptr && a < b + qbytes && b < a + bytes;
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_cat_supported(int N, int C1, int C2, int Co, int H, int W) { return c2_cat_supported(N, C1, C2, Co, H, W) ? 1 : 0; }

extern "C" size_t mphip_conv2d_cat_workspace_bytes(int N, int C1, int C2, int Co, int H, int W) {
    if (!c2_cat_supported(N, C1, C2, Co, H, W)) return 0;
    return (size_t)2 * MPHIP_RANGE_FLOATS * sizeof(float);   // a library-computed descriptor per source (x1_range / x2_range == NULL)
}

extern "C" int mphip_conv2d_cat_fwd(const float *x1, const float *affine1, int relu1, const float *x1_range, int C1, const float *x2,
                                    const float *affine2, int relu2, const float *x2_range, int C2, const void *w_packed, const float *bias,
                                    const float *residual, float *y, float *out_range, int N, int Co, int H, int W, int relu,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(x1 && w_packed && bias && y, "conv2d_cat_fwd: null pointer");
    MPHIP_REQUIRE(C2 >= 0 && (x2 != nullptr) == (C2 > 0), "conv2d_cat_fwd: x2 and C2 = %d: a second source needs both, one source neither", C2);
    MPHIP_REQUIRE(c2_cat_supported(N, C1, C2, Co, H, W),
                  "conv2d_cat_fwd: unsupported shape N=%d C1=%d C2=%d Co=%d H=%d W=%d (C1 %% 16 == 0, C2 %% 16 == 0, Co %% 32 == 0, N, H, W >= "
                  "1, fewer than 2^31 elements per tensor)", N, C1, C2, Co, H, W);
    MPHIP_REQUIRE(((uintptr_t)w_packed & 15) == 0 && ((uintptr_t)x1 & 3) == 0 && ((uintptr_t)x2 & 3) == 0 && ((uintptr_t)y & 3) == 0,
                  "conv2d_cat_fwd: w_packed must be 16-byte aligned, x1, x2 and y 4-byte aligned");
    MPHIP_REQUIRE(((uintptr_t)affine1 & 3) == 0 && ((uintptr_t)affine2 & 3) == 0, "conv2d_cat_fwd: the affine tables must be 4-byte aligned");
    // the bound of a normalised source is not the maximum of its raw values: a scan of x would give the wrong operand scale
    MPHIP_REQUIRE(!affine1 || x1_range, "conv2d_cat_fwd: affine1 without x1_range (mphip_groupnorm_affine_table makes both)");
    MPHIP_REQUIRE(!affine2 || (x2 && x2_range), "conv2d_cat_fwd: affine2 without x2 / x2_range (mphip_groupnorm_affine_table makes both)");
    const size_t hw = (size_t)H * W, ybytes = (size_t)N * Co * hw * sizeof(float);
    MPHIP_REQUIRE(!c2_overlap(y, ybytes, x1, (size_t)N * C1 * hw * sizeof(float)) && !c2_overlap(y, ybytes, x2, (size_t)N * C2 * hw * sizeof(float)) &&
                      !c2_overlap(y, ybytes, residual, ybytes),
                  "conv2d_cat_fwd: y must not alias x1, x2 or residual (a workgroup reads the halo of tiles other workgroups write)");
    hipStream_t s = (hipStream_t)stream;
    const size_t one = (size_t)MPHIP_RANGE_FLOATS * sizeof(float);
    const size_t need = ((x1_range ? 0 : 1) + (x2 && !x2_range ? 1 : 0)) * one;
    if (need) {
        if (!workspace || workspace_bytes < need) {
            set_error("conv2d_cat_fwd: workspace %zu bytes < required %zu", workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        MPHIP_REQUIRE(((uintptr_t)workspace & 3) == 0, "conv2d_cat_fwd: the workspace must be 4-byte aligned");
        float *slot = (float *)workspace;
        if (!x1_range) {
            conv2d_range_launch(x1, (size_t)N * C1 * hw, slot, s);
            x1_range = slot;
            slot += MPHIP_RANGE_FLOATS;
        }
        if (x2 && !x2_range) {
            conv2d_range_launch(x2, (size_t)N * C2 * hw, slot, s);
            x2_range = slot;
        }
    }
    const int tiles_w = cdiv(W, C2_TW), tiles_h = cdiv(H, C2_TH);
    const long long tiles = (long long)N * tiles_h * tiles_w;
    MPHIP_REQUIRE(tiles < (1ll << 31), "conv2d_cat_fwd: %lld tiles do not fit a launch", tiles);
    const dim3 grid((unsigned)tiles, (unsigned)c2_cots(Co));
    const unsigned nslots = (unsigned)std::min<long long>(tiles * c2_cots(Co), (long long)RANGE_MAX_PARTS);
    if (out_range) conv2d_out_range_init_launch(out_range, nslots, s);
    const C2CatArgs cat{affine1, x2, affine2, x2_range, C2, relu1 ? 1 : 0, relu2 ? 1 : 0};
    hipLaunchKernelGGL(conv2d_k3_cat_f16x3_kernel, grid, dim3(C2_NTHR), 0, s, x1, x1_range, cat, (const _Float16 *)((const char *)w_packed + 16),
                       (const float *)w_packed, bias, residual, y, out_range, C1, Co, H, W, relu, tiles_w, tiles_h, nslots);
    return check_launch("conv2d_cat_fwd");
}
