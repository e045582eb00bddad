// The half-precision forms of the 2-D 3x3 conv: the instantiations of conv2d_f16x3_tile.h over the model dtype of the maps (XDT, YDT) and
// the product count (NP) that the fused 2-D blocks use in half and autocast runs, behind mphip_conv2d_fwd_typed / mphip_conv2d_cat_fwd_typed.
// conv2d_f16x3.hip and conv2d_gn_f16x3.hip keep the fp32, three-product kernels; an all-fp32 three-product call is handed to their entries.
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

static inline bool lp_dtype_known(int d) { return d == MPHIP_DTYPE_F32 || d == MPHIP_DTYPE_F16 || d == MPHIP_DTYPE_BF16; }
static inline size_t lp_dtype_bytes(int d) { return d == MPHIP_DTYPE_F32 ? 4 : 2; }

// The product count of a call: 3, 1, or 0 = the calling thread's policy flag.  -1: not one of them.
static int lp_products(int products) {
    if (products == 0) return conv_half_products() ? 1 : 3;
    return products == 1 || products == 3 ? products : -1;
}

// Is (form, dtypes, resolved product count) one of the kernels above, or the fp32 three-product kernel of the other two units?
static bool lp_instantiated(bool cat, int x_dtype, int y_dtype, int np) {
    if (np == 3) return x_dtype == MPHIP_DTYPE_F32 && y_dtype == MPHIP_DTYPE_F32;
    if (cat) return x_dtype == MPHIP_DTYPE_F32;
    return x_dtype == MPHIP_DTYPE_F32 || y_dtype == MPHIP_DTYPE_F32;
}

// The dtype rules of both typed entries, before any HIP call.  np: the resolved product count.
static int lp_check(const char *who, bool cat, int x_dtype, int residual_dtype, int y_dtype, int products, int &np) {
    MPHIP_REQUIRE(lp_dtype_known(x_dtype), "%s: unknown x dtype %d", who, x_dtype);
    MPHIP_REQUIRE(lp_dtype_known(residual_dtype), "%s: unknown residual dtype %d", who, residual_dtype);
    MPHIP_REQUIRE(lp_dtype_known(y_dtype), "%s: unknown y dtype %d", who, y_dtype);
    np = lp_products(products);
    MPHIP_REQUIRE(np > 0, "%s: products = %d (3, 1, or 0: the calling thread's mphip_conv3d_set_half_products flag)", who, products);
    const int ds[3] = {x_dtype, residual_dtype, y_dtype};
    bool f16 = false, bf16 = false;
    for (int d : ds) {
        f16 |= d == MPHIP_DTYPE_F16;
        bf16 |= d == MPHIP_DTYPE_BF16;
    }
    MPHIP_REQUIRE(!(f16 && bf16), "%s: two different half dtypes in one call (x %d, residual %d, y %d)", who, x_dtype, residual_dtype, y_dtype);
    MPHIP_REQUIRE(!cat || x_dtype == MPHIP_DTYPE_F32,
                  "%s: a typed source (x_dtype %d): the two-source form reads fp32 sources, widen them with mphip_cast_to_f32_range", who,
                  x_dtype);
    MPHIP_REQUIRE(residual_dtype == MPHIP_DTYPE_F32 || residual_dtype == y_dtype, "%s: residual_dtype %d: fp32 or the dtype of y (%d)", who,
                  residual_dtype, y_dtype);
    MPHIP_REQUIRE(lp_instantiated(cat, x_dtype, y_dtype, np),
                  "%s: no kernel for x dtype %d, y dtype %d and %d product(s) (mphip_conv2d_typed_supported)", who, x_dtype, y_dtype, np);
    return MPHIP_OK;
}

// [p, p + bytes) and [q, q + qbytes) share a byte
static bool lp_overlap(const void *p, size_t bytes, const void *q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return q != nullptr && a < b + qbytes && b < a + bytes;
}

struct LpGrid {
    dim3 grid;
    int tiles_w, tiles_h;
    unsigned nslots;
};
static bool lp_grid(int N, int Co, int H, int W, LpGrid &g) {
    g.tiles_w = cdiv(W, C2_TW);
    g.tiles_h = cdiv(H, C2_TH);
    const long long tiles = (long long)N * g.tiles_h * g.tiles_w;
    if (tiles >= (1ll << 31)) return false;
    g.grid = dim3((unsigned)tiles, (unsigned)c2_cots(Co));
    g.nslots = (unsigned)std::min<long long>(tiles * c2_cots(Co), (long long)RANGE_MAX_PARTS);
    return true;
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_typed_supported(int two_source, int x_dtype, int residual_dtype, int y_dtype, int products) {
    if (!lp_dtype_known(x_dtype) || !lp_dtype_known(residual_dtype) || !lp_dtype_known(y_dtype)) return 0;
    const int np = lp_products(products);
    if (np < 0) return 0;
    const bool f16 = x_dtype == MPHIP_DTYPE_F16 || residual_dtype == MPHIP_DTYPE_F16 || y_dtype == MPHIP_DTYPE_F16;
    const bool bf16 = x_dtype == MPHIP_DTYPE_BF16 || residual_dtype == MPHIP_DTYPE_BF16 || y_dtype == MPHIP_DTYPE_BF16;
    if (f16 && bf16) return 0;
    if (residual_dtype != MPHIP_DTYPE_F32 && residual_dtype != y_dtype) return 0;
    return lp_instantiated(two_source != 0, x_dtype, y_dtype, np) ? 1 : 0;
}

extern "C" int mphip_conv2d_fwd_typed(const void *x, int x_dtype, const float *x_range, const void *w_packed, const float *bias,
                                      const void *residual, int residual_dtype, void *y, int y_dtype, float *out_range, int N, int Ci,
                                      int Co, int H, int W, int relu, int products, void *workspace, size_t workspace_bytes, void *stream) {
    int np = 0;
    if (const int rc = lp_check("conv2d_fwd_typed", false, x_dtype, residual_dtype, y_dtype, products, np)) return rc;
    if (np == 3)   // (all fp32 by lp_check) the three-product kernel and every check of its entry
        return mphip_conv2d_fwd((const float *)x, x_range, w_packed, bias, (const float *)residual, (float *)y, out_range, N, Ci, Co, H, W,
                                relu, workspace, workspace_bytes, stream);
    MPHIP_REQUIRE(x && w_packed && bias && y, "conv2d_fwd_typed: null pointer");
    MPHIP_REQUIRE(c2_supported(N, Ci, Co, H, W),
                  "conv2d_fwd_typed: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d (Ci %% 16 == 0, Co %% 32 == 0, N, H, W >= 1, fewer than "
                  "2^31 elements per tensor)", N, Ci, Co, H, W);
    const size_t xa = lp_dtype_bytes(x_dtype) - 1, ya = lp_dtype_bytes(y_dtype) - 1, ra = lp_dtype_bytes(residual_dtype) - 1;
    MPHIP_REQUIRE(((uintptr_t)w_packed & 15) == 0 && ((uintptr_t)x & xa) == 0 && ((uintptr_t)y & ya) == 0 && ((uintptr_t)residual & ra) == 0,
                  "conv2d_fwd_typed: w_packed must be 16-byte aligned, x, y and residual aligned to their element size");
    const size_t hw = (size_t)H * W, ybytes = (size_t)N * Co * hw * lp_dtype_bytes(y_dtype);
    MPHIP_REQUIRE(!lp_overlap(y, ybytes, x, (size_t)N * Ci * hw * lp_dtype_bytes(x_dtype)) &&
                      !lp_overlap(y, ybytes, residual, (size_t)N * Co * hw * lp_dtype_bytes(residual_dtype)),
                  "conv2d_fwd_typed: y must not alias x or residual (a workgroup reads the halo of tiles other workgroups write)");
    hipStream_t s = (hipStream_t)stream;
    if (!x_range) {
        const size_t need = (size_t)MPHIP_RANGE_FLOATS * sizeof(float);
        if (!workspace || workspace_bytes < need) {
            set_error("conv2d_fwd_typed: workspace %zu bytes < required %zu", workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        MPHIP_REQUIRE(((uintptr_t)workspace & 3) == 0, "conv2d_fwd_typed: the workspace must be 4-byte aligned");
        if (x_dtype == MPHIP_DTYPE_F32) {
            conv2d_range_launch((const float *)x, (size_t)N * Ci * hw, (float *)workspace, s);
        } else if (const int rc = cast_range_launch(x, x_dtype, (size_t)N * Ci * hw, nullptr, (float *)workspace, s)) {
            return rc;   // (the descriptor of the widened values: widening is exact)
        }
        x_range = (const float *)workspace;
    }
    LpGrid g;
    MPHIP_REQUIRE(lp_grid(N, Co, H, W, g), "conv2d_fwd_typed: the tiles do not fit a launch");
    if (out_range) conv2d_out_range_init_launch(out_range, g.nslots, s);
    const _Float16 *slabs = (const _Float16 *)((const char *)w_packed + 16);
    const int rt = residual && residual_dtype != MPHIP_DTYPE_F32 ? 1 : 0;
#define LP_LAUNCH(XD, YD)                                                                                                              \
    hipLaunchKernelGGL((conv2d_k3_lp_kernel<XD, YD, 1>), g.grid, dim3(C2_NTHR), 0, s, (const dtype_t<XD> *)x, x_range, slabs,            \
                       (const float *)w_packed, bias, residual, rt, (dtype_t<YD> *)y, out_range, Ci, Co, H, W, relu, g.tiles_w, g.tiles_h, \
                       g.nslots)
    if (y_dtype == MPHIP_DTYPE_F32) {
        if (x_dtype == MPHIP_DTYPE_F32) LP_LAUNCH(MPHIP_DTYPE_F32, MPHIP_DTYPE_F32);
        else if (x_dtype == MPHIP_DTYPE_F16) LP_LAUNCH(MPHIP_DTYPE_F16, MPHIP_DTYPE_F32);
        else LP_LAUNCH(MPHIP_DTYPE_BF16, MPHIP_DTYPE_F32);
    } else if (y_dtype == MPHIP_DTYPE_F16) {
        LP_LAUNCH(MPHIP_DTYPE_F32, MPHIP_DTYPE_F16);
    } else {
        LP_LAUNCH(MPHIP_DTYPE_F32, MPHIP_DTYPE_BF16);
    }
#undef LP_LAUNCH
    return check_launch("conv2d_fwd_typed");
}

extern "C" int mphip_conv2d_cat_fwd_typed(const void *x1, int x_dtype, const float *affine1, int relu1, const float *x1_range, int C1,
                                          const void *x2, const float *affine2, int relu2, const float *x2_range, int C2,
                                          const void *w_packed, const float *bias, const void *residual, int residual_dtype, void *y,
                                          int y_dtype, float *out_range, int N, int Co, int H, int W, int relu, int products,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    int np = 0;
    if (const int rc = lp_check("conv2d_cat_fwd_typed", true, x_dtype, residual_dtype, y_dtype, products, np)) return rc;
    if (np == 3)
        return mphip_conv2d_cat_fwd((const float *)x1, affine1, relu1, x1_range, C1, (const float *)x2, affine2, relu2, x2_range, C2,
                                    w_packed, bias, (const float *)residual, (float *)y, out_range, N, Co, H, W, relu, workspace,
                                    workspace_bytes, stream);
    MPHIP_REQUIRE(x1 && w_packed && bias && y, "conv2d_cat_fwd_typed: null pointer");
    MPHIP_REQUIRE(C2 >= 0 && (x2 != nullptr) == (C2 > 0), "conv2d_cat_fwd_typed: x2 and C2 = %d: a second source needs both, one source neither",
                  C2);
    MPHIP_REQUIRE(mphip_conv2d_cat_supported(N, C1, C2, Co, H, W),
                  "conv2d_cat_fwd_typed: unsupported shape N=%d C1=%d C2=%d Co=%d H=%d W=%d (C1 %% 16 == 0, C2 %% 16 == 0, Co %% 32 == 0, N, H, "
                  "W >= 1, fewer than 2^31 elements per tensor)", N, C1, C2, Co, H, W);
    const size_t ya = lp_dtype_bytes(y_dtype) - 1, ra = lp_dtype_bytes(residual_dtype) - 1;
    MPHIP_REQUIRE(((uintptr_t)w_packed & 15) == 0 && ((uintptr_t)x1 & 3) == 0 && ((uintptr_t)x2 & 3) == 0 && ((uintptr_t)y & ya) == 0 &&
                      ((uintptr_t)residual & ra) == 0,
                  "conv2d_cat_fwd_typed: w_packed must be 16-byte aligned, x1 and x2 4-byte aligned, y and residual aligned to their element size");
    MPHIP_REQUIRE(((uintptr_t)affine1 & 3) == 0 && ((uintptr_t)affine2 & 3) == 0, "conv2d_cat_fwd_typed: the affine tables must be 4-byte aligned");
    MPHIP_REQUIRE(!affine1 || x1_range, "conv2d_cat_fwd_typed: affine1 without x1_range (mphip_groupnorm_affine_table makes both)");
    MPHIP_REQUIRE(!affine2 || (x2 && x2_range), "conv2d_cat_fwd_typed: affine2 without x2 / x2_range (mphip_groupnorm_affine_table makes both)");
    const size_t hw = (size_t)H * W, ybytes = (size_t)N * Co * hw * lp_dtype_bytes(y_dtype);
    MPHIP_REQUIRE(!lp_overlap(y, ybytes, x1, (size_t)N * C1 * hw * sizeof(float)) && !lp_overlap(y, ybytes, x2, (size_t)N * C2 * hw * sizeof(float)) &&
                      !lp_overlap(y, ybytes, residual, (size_t)N * Co * hw * lp_dtype_bytes(residual_dtype)),
                  "conv2d_cat_fwd_typed: y must not alias x1, x2 or residual (a workgroup reads the halo of tiles other workgroups write)");
    hipStream_t s = (hipStream_t)stream;
    const size_t one = (size_t)MPHIP_RANGE_FLOATS * sizeof(float);
    const size_t need = ((x1_range ? 0 : 1) + (x2 && !x2_range ? 1 : 0)) * one;
    if (need) {
        if (!workspace || workspace_bytes < need) {
            set_error("conv2d_cat_fwd_typed: workspace %zu bytes < required %zu", workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        MPHIP_REQUIRE(((uintptr_t)workspace & 3) == 0, "conv2d_cat_fwd_typed: the workspace must be 4-byte aligned");
        float *slot = (float *)workspace;
        if (!x1_range) {
            conv2d_range_launch((const float *)x1, (size_t)N * C1 * hw, slot, s);
            x1_range = slot;
            slot += MPHIP_RANGE_FLOATS;
        }
        if (x2 && !x2_range) {
            conv2d_range_launch((const float *)x2, (size_t)N * C2 * hw, slot, s);
            x2_range = slot;
        }
    }
    LpGrid g;
    MPHIP_REQUIRE(lp_grid(N, Co, H, W, g), "conv2d_cat_fwd_typed: the tiles do not fit a launch");
    if (out_range) conv2d_out_range_init_launch(out_range, g.nslots, s);
    const C2CatArgs cat{affine1, (const float *)x2, affine2, x2_range, C2, relu1 ? 1 : 0, relu2 ? 1 : 0};
    const _Float16 *slabs = (const _Float16 *)((const char *)w_packed + 16);
    const int rt = residual && residual_dtype != MPHIP_DTYPE_F32 ? 1 : 0;
#define LP_LAUNCH(YD)                                                                                                                   \
    hipLaunchKernelGGL((conv2d_k3_cat_lp_kernel<YD, 1>), g.grid, dim3(C2_NTHR), 0, s, (const float *)x1, x1_range, cat, slabs,            \
                       (const float *)w_packed, bias, residual, rt, (dtype_t<YD> *)y, out_range, C1, Co, H, W, relu, g.tiles_w, g.tiles_h, \
                       g.nslots)
    if (y_dtype == MPHIP_DTYPE_F32) LP_LAUNCH(MPHIP_DTYPE_F32);
    else if (y_dtype == MPHIP_DTYPE_F16) LP_LAUNCH(MPHIP_DTYPE_F16);
    else LP_LAUNCH(MPHIP_DTYPE_BF16);
#undef LP_LAUNCH
    return check_launch("conv2d_cat_fwd_typed");
}
