// The half-precision forms of the 2-D 3x3 conv: the instantiations of conv2d_f16x3_tile.h over the model dtype of the maps (XDT, YDT) and
// the product count (NP) that the fused 2-D blocks use in half and autocast runs, behind mphip_conv2d_fwd_typed / mphip_conv2d_cat_fwd_typed.
// conv2d_f16x3.hip and conv2d_gn_f16x3.hip keep the fp32, three-product kernels.  This unit also holds conv2d_run, the host routine behind all
// four entries (the fp32 entries are the typed ones with fp32 maps and three products): it knows the dtype rules, and hands an all-fp32
// three-product call to the launchers of the other two units.
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

// The dtype and product rules of the typed entries -> what is wrong with a combination, or nullptr.  np: the resolved product count.
static const char *lp_rule(bool cat, int x_dtype, int residual_dtype, int y_dtype, int products, int &np) {
    const int ds[3] = {x_dtype, residual_dtype, y_dtype};
    bool f16 = false, bf16 = false;
    for (int d : ds) {
        if (!lp_dtype_known(d)) return "unknown x, residual or y dtype";
        f16 |= d == MPHIP_DTYPE_F16;
        bf16 |= d == MPHIP_DTYPE_BF16;
    }
    np = lp_products(products);
    if (np < 0) return "products must be 3, 1, or 0 (the calling thread's mphip_conv3d_set_half_products flag)";
    if (f16 && bf16) return "two different half dtypes in one call";
    if (cat && x_dtype != MPHIP_DTYPE_F32) return "a typed source: the two-source form reads fp32 sources, widen them with mphip_cast_to_f32_range";
    if (residual_dtype != MPHIP_DTYPE_F32 && residual_dtype != y_dtype) return "residual_dtype must be fp32 or the dtype of y";
    if (!lp_instantiated(cat, x_dtype, y_dtype, np)) return "no kernel for these dtypes and this product count (mphip_conv2d_typed_supported)";
    return nullptr;
}

// [p, p + bytes) and [q, q + qbytes) share a byte
static bool c2_overlap(const void *p, size_t bytes, const void *q, size_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return q != nullptr && a < b + qbytes && b < a + bytes;
}

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
    if (c.cat) {
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

// The host side of every 2-D 3x3 conv entry (the stride-2 entry of conv2d_s2_f16x3.hip included: c.stride == 2, extents of y and
// residual from the halved map; and the two of conv2d_up2_f16x3.hip: c.up2 == 1, y and residual on the doubled map, c.up2 == 2, the
// residual on the halved one; and the grouped one of conv2d_grp_f16x3.hip: c.groups != 0, the group rule ahead of the plain shape rule;
// and the split-K one of conv2d_splitk_f16x3.hip: c.splits != 0, the split rule ahead of the group rule, the partial maps in the
// workspace behind the descriptor slot).
// The rules in the order they are checked, all before the first HIP call: dtypes and products (lp_rule), pointers, the second source, the shape, alignment, tables, aliasing (MPHIP_EINVAL each), then the workspace
// (MPHIP_EWORKSPACE for its size, then MPHIP_EINVAL for its alignment and, for the split-K entry, for partial maps that alias x, y or the
// residual: that check needs the workspace, so it is the last one).  Messages carry the called entry's name; a three-product call (all of its maps are fp32) is the fp32 entry's call
// under whichever name it came in, and reports under that entry's name.
int conv2d_run(C2Call c) {
    int np = 0;
    const char *why = lp_rule(c.cat, c.x_dtype, c.residual_dtype, c.y_dtype, c.products, np);
    MPHIP_REQUIRE(!why, "%s: %s (x dtype %d, residual dtype %d, y dtype %d, products %d)", c.who, why, c.x_dtype, c.residual_dtype, c.y_dtype,
                  c.products);
    c.products = np;
    const bool s2 = c.stride == 2;
    MPHIP_REQUIRE(!s2 || (!c.cat && np == 3), "%s: the stride-2 conv is the plain fp32 three-product form", c.who);
    const int up = c.up2;
    MPHIP_REQUIRE(up == 0 || ((up == 1 || up == 2) && !s2 && !c.cat && np == 3), "%s: the up2 convs are plain fp32 three-product forms", c.who);
    const int grp = c.groups;
    MPHIP_REQUIRE(grp == 0 || (!s2 && !up && !c.cat && np == 3), "%s: the grouped conv is the plain fp32 three-product form at stride 1", c.who);
    const int spl = c.splits;
    MPHIP_REQUIRE(spl == 0 || grp != 0, "%s: the split-K conv takes a group count", c.who);
    const char *who = s2 || up || grp ? c.who : c.products == 3 ? (c.cat ? "conv2d_cat_fwd" : "conv2d_fwd") : c.who;
    MPHIP_REQUIRE(c.x1 && c.w_packed && c.bias && c.y && (up != 2 || c.residual), "%s: null pointer", who);
    MPHIP_REQUIRE(c.C2 >= 0 && (c.x2 != nullptr) == (c.C2 > 0), "%s: x2 and C2 = %d: a second source needs both, one source neither", who, c.C2);
    MPHIP_REQUIRE(spl == 0 || c2_split_supported(c.N, c.C1, c.Co, c.H, c.W, grp, spl),
                  "%s: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d groups=%d splits=%d (the shape rule of conv2d_grouped_fwd; 1 <= splits <= %d, "
                  "a divisor of the (Ci / groups) / 16 chunks)", who, c.N, c.C1, c.Co, c.H, c.W, grp, spl, C2_MAX_SPLITS);
    MPHIP_REQUIRE(grp == 0 || c2_grouped_supported(c.N, c.C1, c.Co, c.H, c.W, grp),
                  "%s: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d groups=%d (groups >= 1; above 1: Ci and Co multiples of groups, (Ci / groups) "
                  "%% 16 == 0, (Co / groups) %% 64 == 0; and the shape rule of conv2d_fwd)", who, c.N, c.C1, c.Co, c.H, c.W, grp);
    MPHIP_REQUIRE(s2        ? c2_s2_supported(c.N, c.C1, c.Co, c.H, c.W)
                  : up == 1 ? c2_up2_supported(c.N, c.C1, c.Co, c.H, c.W)
                  : c.cat   ? mphip_conv2d_cat_supported(c.N, c.C1, c.C2, c.Co, c.H, c.W)
                          : mphip_conv2d_supported(c.N, c.C1, c.Co, c.H, c.W),
                  "%s: unsupported shape N=%d C1=%d C2=%d Co=%d H=%d W=%d (C1 %% 16 == 0, C2 %% 16 == 0, Co %% 32 == 0, N, H, W >= 1, fewer than "
                  "2^31 elements per tensor)", who, c.N, c.C1, c.C2, c.Co, c.H, c.W);
    MPHIP_REQUIRE(up != 2 || (c.H % 2 == 0 && c.W % 2 == 0), "%s: H = %d, W = %d: the map of an up-sampled residual has even extents", who, c.H, c.W);
    const size_t xb = lp_dtype_bytes(c.x_dtype), yb = lp_dtype_bytes(c.y_dtype), rb = lp_dtype_bytes(c.residual_dtype);
    MPHIP_REQUIRE(((uintptr_t)c.w_packed & 15) == 0 && ((uintptr_t)c.x1 & (xb - 1)) == 0 && ((uintptr_t)c.x2 & 3) == 0 &&
                      ((uintptr_t)c.y & (yb - 1)) == 0 && ((uintptr_t)c.residual & (rb - 1)) == 0,
                  "%s: w_packed must be 16-byte aligned, the sources, y and residual aligned to their element size", who);
    MPHIP_REQUIRE(((uintptr_t)c.aff1 & 3) == 0 && ((uintptr_t)c.aff2 & 3) == 0, "%s: the affine tables must be 4-byte aligned", who);
    // the bound of a normalised source is not the maximum of its raw values: a scan of x would give the wrong operand scale
    MPHIP_REQUIRE(!c.aff1 || c.x1_range, "%s: affine1 without x1_range (mphip_groupnorm_affine_table makes both)", who);
    MPHIP_REQUIRE(!c.aff2 || (c.x2 && c.x2_range), "%s: affine2 without x2 / x2_range (mphip_groupnorm_affine_table makes both)", who);
    const int Ho = s2 ? (c.H + 1) / 2 : up == 1 ? 2 * c.H : c.H, Wo = s2 ? (c.W + 1) / 2 : up == 1 ? 2 * c.W : c.W;   // the map of y and residual
    const size_t hw = (size_t)c.H * c.W, n1 = (size_t)c.N * c.C1 * hw, n2 = (size_t)c.N * c.C2 * hw, ny = (size_t)c.N * c.Co * Ho * Wo;
    const size_t nr = up == 2 ? ny / 4 : ny;   // (an up-sampled residual lives on the halved map)
    MPHIP_REQUIRE(!c2_overlap(c.y, ny * yb, c.x1, n1 * xb) && !c2_overlap(c.y, ny * yb, c.x2, n2 * sizeof(float)) &&
                      !c2_overlap(c.y, ny * yb, c.residual, nr * rb),
                  "%s: y must not alias a source or residual (a workgroup reads the halo of tiles other workgroups write)", who);
    const bool scan1 = !c.x1_range, scan2 = c.x2 && !c.x2_range;
    const size_t part_bytes = spl > 1 ? (size_t)spl * ny * sizeof(float) : 0;   // the split-K partial maps, behind the descriptor slots
    float *part = nullptr;
    if (scan1 || scan2 || part_bytes) {
        const size_t need = c2_workspace_bytes((scan1 ? 1 : 0) + (scan2 ? 1 : 0)) + part_bytes;
        if (!c.workspace || c.workspace_bytes < need) {
            set_error("%s: workspace %zu bytes < required %zu", who, c.workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        MPHIP_REQUIRE(((uintptr_t)c.workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", who);
        float *slot = (float *)c.workspace;
        if (part_bytes) {   // the last refusal, still ahead of the scans below: the first HIP call
            part = slot + ((scan1 ? 1 : 0) + (scan2 ? 1 : 0)) * MPHIP_RANGE_FLOATS;
            MPHIP_REQUIRE(!c2_overlap(part, part_bytes, c.y, ny * yb) && !c2_overlap(part, part_bytes, c.x1, n1 * xb) &&
                              !c2_overlap(part, part_bytes, c.residual, nr * rb),
                          "%s: the workspace's partial maps must not alias x, y or residual", who);
        }
        if (scan1) {
            if (c.x_dtype == MPHIP_DTYPE_F32) {
                conv2d_range_launch((const float *)c.x1, n1, slot, c.stream);
            } else if (const int rc = cast_range_launch(c.x1, c.x_dtype, n1, nullptr, slot, c.stream)) {
                return rc;   // (the descriptor of the widened values: widening is exact)
            }
            c.x1_range = slot;
            slot += MPHIP_RANGE_FLOATS;
        }
        if (scan2) {
            conv2d_range_launch((const float *)c.x2, n2, slot, c.stream);
            c.x2_range = slot;
        }
    }
    C2Grid g;
    g.tiles_w = cdiv(Wo, s2 ? C2S2_TW : C2_TW), g.tiles_h = cdiv(Ho, s2 ? C2S2_TH : C2_TH);
    const long long tiles = (long long)c.N * g.tiles_h * g.tiles_w;   // (N * H * W < 2^31 by the shape rule: they fit grid.x)
    g.grid = dim3((unsigned)tiles, (unsigned)c2_cots(c.Co));
    g.nslots = (unsigned)std::min<long long>(part ? (long long)c2_split_finish_blocks(ny) : tiles * c2_cots(c.Co), (long long)RANGE_MAX_PARTS);
    if (c.out_range) conv2d_out_range_init_launch(c.out_range, g.nslots, c.stream);
    if (s2) conv2d_s2_launch(c, g);
    else if (up) conv2d_up2_launch(c, g);
    else if (part) conv2d_split_launch(c, g, part);
    else if (grp > 1) conv2d_grouped_launch(c, g);
    else if (c.products == 1) conv2d_lp_launch(c, g);
    else if (c.cat) conv2d_cat_launch(c, g);
    else conv2d_plain_launch(c, g);
    return check_launch(who);
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_typed_supported(int two_source, int x_dtype, int residual_dtype, int y_dtype, int products) {
    int np;
    return lp_rule(two_source != 0, x_dtype, residual_dtype, y_dtype, products, np) ? 0 : 1;
}

extern "C" int mphip_conv2d_fwd_typed(const void *x, int x_dtype, const float *x_range, const void *w_packed, const float *bias,
                                      const void *residual, int residual_dtype, void *y, int y_dtype, float *out_range, int N, int Ci,
                                      int Co, int H, int W, int relu, int products, void *workspace, size_t workspace_bytes, void *stream) {
    C2Call c{};
    c.who = "conv2d_fwd_typed";
    c.x1 = x, c.x1_range = x_range, c.C1 = Ci;
    c.x_dtype = x_dtype, c.residual_dtype = residual_dtype, c.y_dtype = y_dtype, c.products = products;
    c.w_packed = w_packed, c.bias = bias, c.residual = residual, c.y = y, c.out_range = out_range;
    c.N = N, c.Co = Co, c.H = H, c.W = W, c.relu = relu;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = (hipStream_t)stream;
    return conv2d_run(c);
}

extern "C" int mphip_conv2d_cat_fwd_typed(const void *x1, int x_dtype, const float *affine1, int relu1, const float *x1_range, int C1,
                                          const void *x2, const float *affine2, int relu2, const float *x2_range, int C2,
                                          const void *w_packed, const float *bias, const void *residual, int residual_dtype, void *y,
                                          int y_dtype, float *out_range, int N, int Co, int H, int W, int relu, int products,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    C2Call c{};
    c.who = "conv2d_cat_fwd_typed", c.cat = true;
    c.x1 = x1, c.aff1 = affine1, c.relu1 = relu1, c.x1_range = x1_range, c.C1 = C1;
    c.x2 = x2, c.aff2 = affine2, c.relu2 = relu2, c.x2_range = x2_range, c.C2 = C2;
    c.x_dtype = x_dtype, c.residual_dtype = residual_dtype, c.y_dtype = y_dtype, c.products = products;
    c.w_packed = w_packed, c.bias = bias, c.residual = residual, c.y = y, c.out_range = out_range;
    c.N = N, c.Co = Co, c.H = H, c.W = W, c.relu = relu;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = (hipStream_t)stream;
    return conv2d_run(c);
}
