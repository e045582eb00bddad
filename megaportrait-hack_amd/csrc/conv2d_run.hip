// The host side of every 2-D conv entry (the 3x3 forms and the pointwise one): conv2d_run, the dtype and product rules of the typed
// entries, and the table of forms that says per C2Form what the entries differ in.  No kernels: each form's kernels, launcher and shape
// rule live in its own unit.
#include "conv2d_f16x3_tile.h"

namespace mphip {

static inline bool lp_dtype_known(int d) { return d == MPHIP_DTYPE_F32 || d == MPHIP_DTYPE_F16 || d == MPHIP_DTYPE_BF16; }
static inline size_t lp_dtype_bytes(int d) { return d == MPHIP_DTYPE_F32 ? 4 : 2; }

// The product count of a call: 3, 1, or 0 = the calling thread's policy flag.  -1: not one of them.
static int lp_products(int products) {
    if (products == 0) return conv_half_products() ? 1 : 3;
    return products == 1 || products == 3 ? products : -1;
}

// Is (form, dtypes, resolved product count) one of conv2d_lp.hip's kernels, or the fp32 three-product kernel of the other units?
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

// The three texts of a refused shape.  A group or split count below 1 is reported as -1, as it was when the entries stored one in a
// field whose 0 meant "not this entry's call": the texts are part of the entries' contract.
static int c2_shown(int count) { return count < 1 ? -1 : count; }
static void c2_refuse_shape(const char *who, const C2Call &c) {
    set_error("%s: unsupported shape N=%d C1=%d C2=%d Co=%d H=%d W=%d (C1 %% 16 == 0, C2 %% 16 == 0, Co %% 32 == 0, N, H, W >= 1, fewer than "
              "2^31 elements per tensor)", who, c.N, c.C1, c.C2, c.Co, c.H, c.W);
}
static void c2_refuse_groups(const char *who, const C2Call &c) {
    set_error("%s: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d groups=%d (groups >= 1; above 1: Ci and Co multiples of groups, (Ci / groups) "
              "%% 16 == 0, (Co / groups) %% 64 == 0; and the shape rule of conv2d_fwd)", who, c.N, c.C1, c.Co, c.H, c.W, c2_shown(c.groups));
}
static void c2_refuse_pw(const char *who, const C2Call &c) {
    set_error("%s: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d stride=%d (stride 1 or 2, Ci %% 16 == 0, Co %% 32 == 0, N, H, W >= 1, fewer "
              "than 2^31 elements per tensor)", who, c.N, c.C1, c.Co, c.H, c.W, c.stride);
}
static void c2_refuse_splits(const char *who, const C2Call &c) {
    set_error("%s: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d groups=%d splits=%d (the shape rule of conv2d_grouped_fwd; 1 <= splits <= %d, "
              "a divisor of the (Ci / groups) / 16 chunks)", who, c.N, c.C1, c.Co, c.H, c.W, c2_shown(c.groups), c2_shown(c.splits),
              C2_MAX_SPLITS);
}

// A typed-capable form's kernel depends on the call: one product or three, then two sources or one
static void c2_typed_launch(const C2Call &c, const C2Grid &g) {
    if (c.products == 1) conv2d_lp_launch(c, g);
    else if (c.form == C2_CAT) conv2d_cat_launch(c, g);
    else conv2d_plain_launch(c, g);
}

// an extent of y or of the residual from the same extent (H or W) of the call
static int c2_same(const C2Call &, int e) { return e; }
static int c2_strided(const C2Call &, int e) { return (e + 1) / 2; }
static int c2_doubled(const C2Call &, int e) { return 2 * e; }
static int c2_halved(const C2Call &, int e) { return e / 2; }
static int c2_by_stride(const C2Call &c, int e) { return (e + c.stride - 1) / c.stride; }   // (after the shape rule: stride is 1 or 2)

// What the forms differ in; conv2d_run looks everything else up here.
struct C2FormRow {
    bool typed;                                         // admits typed maps and one product; else fp32 maps and three products only
    const char *fp32_name;                              // a typed form's three-product call (all of its maps are fp32) is the fp32 entry's
                                                        // call under whichever name it came in, and reports under this one; else NULL
    bool lowres_residual;                               // the residual is required and lives on the halved map: H and W even
    bool (*shape)(const C2Call &);                      // the shape rule ...
    void (*refuse)(const char *who, const C2Call &);    // ... and the message of a call that fails it
    int (*y_extent)(const C2Call &, int), (*residual_extent)(const C2Call &, int);
    int th, tw;                                         // output pixels per workgroup; th == 0: tw pixels of the FLAT index Ho * Wo
    bool partials;                                      // c.splits > 1: that many partial maps of y's size in the workspace
    void (*launch)(const C2Call &, const C2Grid &);
};
static const C2FormRow C2_FORM_TABLE[] = {
    /* C2_PLAIN   */ {true, "conv2d_fwd", false, [](const C2Call &c) { return mphip_conv2d_supported(c.N, c.C1, c.Co, c.H, c.W) != 0; },
                      c2_refuse_shape, c2_same, c2_same, C2_TH, C2_TW, false, c2_typed_launch},
    /* C2_CAT     */ {true, "conv2d_cat_fwd", false, [](const C2Call &c) { return mphip_conv2d_cat_supported(c.N, c.C1, c.C2, c.Co, c.H, c.W) != 0; },
                      c2_refuse_shape, c2_same, c2_same, C2_TH, C2_TW, false, c2_typed_launch},
    /* C2_S2      */ {false, nullptr, false, [](const C2Call &c) { return c2_s2_supported(c.N, c.C1, c.Co, c.H, c.W); },
                      c2_refuse_shape, c2_strided, c2_strided, C2S2_TH, C2S2_TW, false, conv2d_s2_launch},
    /* C2_UP2     */ {false, nullptr, false, [](const C2Call &c) { return c2_up2_supported(c.N, c.C1, c.Co, c.H, c.W); },
                      c2_refuse_shape, c2_doubled, c2_doubled, C2_TH, C2_TW, false, conv2d_up2_launch},
    /* C2_RESUP2  */ {false, nullptr, true, [](const C2Call &c) { return mphip_conv2d_supported(c.N, c.C1, c.Co, c.H, c.W) != 0; },
                      c2_refuse_shape, c2_same, c2_halved, C2_TH, C2_TW, false, conv2d_up2_launch},
    /* C2_GROUPED */ {false, nullptr, false, [](const C2Call &c) { return c2_grouped_supported(c.N, c.C1, c.Co, c.H, c.W, c.groups); },
                      c2_refuse_groups, c2_same, c2_same, C2_TH, C2_TW, false, conv2d_grouped_launch},
    /* C2_SPLIT   */ {false, nullptr, false, [](const C2Call &c) { return c2_split_supported(c.N, c.C1, c.Co, c.H, c.W, c.groups, c.splits); },
                      c2_refuse_splits, c2_same, c2_same, C2_TH, C2_TW, true, conv2d_split_launch},
    /* C2_PW      */ {false, nullptr, false, [](const C2Call &c) { return c2_pw_supported(c.N, c.C1, c.Co, c.H, c.W, c.stride); },
                      c2_refuse_pw, c2_by_stride, c2_by_stride, 0, C2PW_PIX, false, conv2d_pw_launch},
};
static_assert(sizeof(C2_FORM_TABLE) / sizeof(C2_FORM_TABLE[0]) == C2_FORMS, "one row per C2Form, in its order");

// The rules in the order they are checked, all before the first HIP call: dtypes and products (lp_rule), the form's admissibility,
// pointers, the second source, the shape, alignment, tables, aliasing (MPHIP_EINVAL each); then the workspace: MPHIP_EWORKSPACE for its
// size, then MPHIP_EINVAL for its alignment and for partial maps that alias x, y or the residual (that check needs the workspace, so it
// is the last one).  Then the scans, the grid, out_range's init launch and the form's launcher.  Messages carry the called entry's
// name, but for C2FormRow::fp32_name.
int conv2d_run(C2Call c) {
    const C2FormRow &f = C2_FORM_TABLE[c.form];
    int np = 0;
    const char *why = lp_rule(c.form == C2_CAT, c.x_dtype, c.residual_dtype, c.y_dtype, c.products, np);
    MPHIP_REQUIRE(!why, "%s: %s (x dtype %d, residual dtype %d, y dtype %d, products %d)", c.who, why, c.x_dtype, c.residual_dtype, c.y_dtype,
                  c.products);
    c.products = np;
    MPHIP_REQUIRE(f.typed || np == 3, "%s: this form takes fp32 maps and three products only", c.who);
    const char *who = f.fp32_name && np == 3 ? f.fp32_name : c.who;
    MPHIP_REQUIRE(c.x1 && c.w_packed && c.bias && c.y && (!f.lowres_residual || c.residual), "%s: null pointer", who);
    MPHIP_REQUIRE(c.C2 >= 0 && (c.x2 != nullptr) == (c.C2 > 0), "%s: x2 and C2 = %d: a second source needs both, one source neither", who, c.C2);
    if (!f.shape(c)) {
        f.refuse(who, c);
        return MPHIP_EINVAL;
    }
    MPHIP_REQUIRE(!f.lowres_residual || (c.H % 2 == 0 && c.W % 2 == 0), "%s: H = %d, W = %d: the map of an up-sampled residual has even extents",
                  who, c.H, c.W);
    const size_t xb = lp_dtype_bytes(c.x_dtype), yb = lp_dtype_bytes(c.y_dtype), rb = lp_dtype_bytes(c.residual_dtype);
    MPHIP_REQUIRE(((uintptr_t)c.w_packed & 15) == 0 && ((uintptr_t)c.x1 & (xb - 1)) == 0 && ((uintptr_t)c.x2 & 3) == 0 &&
                      ((uintptr_t)c.y & (yb - 1)) == 0 && ((uintptr_t)c.residual & (rb - 1)) == 0,
                  "%s: w_packed must be 16-byte aligned, the sources, y and residual aligned to their element size", who);
    MPHIP_REQUIRE(((uintptr_t)c.aff1 & 3) == 0 && ((uintptr_t)c.aff2 & 3) == 0, "%s: the affine tables must be 4-byte aligned", who);
    // the bound of a normalised source is not the maximum of its raw values: a scan of x would give the wrong operand scale
    MPHIP_REQUIRE(!c.aff1 || c.x1_range, "%s: affine1 without x1_range (mphip_groupnorm_affine_table makes both)", who);
    MPHIP_REQUIRE(!c.aff2 || (c.x2 && c.x2_range), "%s: affine2 without x2 / x2_range (mphip_groupnorm_affine_table makes both)", who);
    const int Ho = f.y_extent(c, c.H), Wo = f.y_extent(c, c.W);
    const size_t hw = (size_t)c.H * c.W, n1 = (size_t)c.N * c.C1 * hw, n2 = (size_t)c.N * c.C2 * hw, ny = (size_t)c.N * c.Co * Ho * Wo;
    const size_t nr = (size_t)c.N * c.Co * f.residual_extent(c, c.H) * f.residual_extent(c, c.W);
    MPHIP_REQUIRE(!c2_overlap(c.y, ny * yb, c.x1, n1 * xb) && !c2_overlap(c.y, ny * yb, c.x2, n2 * sizeof(float)) &&
                      !c2_overlap(c.y, ny * yb, c.residual, nr * rb),
                  "%s: y must not alias a source or residual (a workgroup reads the halo of tiles other workgroups write)", who);
    const bool scan1 = !c.x1_range, scan2 = c.x2 && !c.x2_range;
    const size_t part_bytes = f.partials && c.splits > 1 ? (size_t)c.splits * ny * sizeof(float) : 0;   // behind the descriptor slots
    C2Grid g{};
    if (scan1 || scan2 || part_bytes) {
        const size_t need = c2_workspace_bytes((scan1 ? 1 : 0) + (scan2 ? 1 : 0)) + part_bytes;
        if (!c.workspace || c.workspace_bytes < need) {
            set_error("%s: workspace %zu bytes < required %zu", who, c.workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        MPHIP_REQUIRE(((uintptr_t)c.workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", who);
        float *slot = (float *)c.workspace;
        if (part_bytes) {   // the last refusal, still ahead of the scans below: the first HIP call
            g.part = slot + ((scan1 ? 1 : 0) + (scan2 ? 1 : 0)) * MPHIP_RANGE_FLOATS;
            MPHIP_REQUIRE(!c2_overlap(g.part, part_bytes, c.y, ny * yb) && !c2_overlap(g.part, part_bytes, c.x1, n1 * xb) &&
                              !c2_overlap(g.part, part_bytes, c.residual, nr * rb),
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
    if (f.th) g.tiles_w = cdiv(Wo, f.tw), g.tiles_h = cdiv(Ho, f.th);
    else g.tiles_w = cdiv((long)Ho * Wo, f.tw), g.tiles_h = 1;
    const long long tiles = (long long)c.N * g.tiles_h * g.tiles_w;   // (N * H * W < 2^31 by the shape rule: they fit grid.x)
    g.grid = dim3((unsigned)tiles, (unsigned)c2_cots(c.Co));
    g.nslots = (unsigned)std::min<long long>(g.part ? (long long)c2_split_finish_blocks(ny) : tiles * c2_cots(c.Co), (long long)RANGE_MAX_PARTS);
    if (c.out_range) conv2d_out_range_init_launch(c.out_range, g.nslots, c.stream);
    f.launch(c, g);
    return check_launch(who);
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_typed_supported(int two_source, int x_dtype, int residual_dtype, int y_dtype, int products) {
    int np;
    return lp_rule(two_source != 0, x_dtype, residual_dtype, y_dtype, products, np) ? 0 : 1;
}
