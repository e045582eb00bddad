// The tile code of the 2-D 3x3 f16x3 conv, shared by its two translation units:
//   conv2d_f16x3.hip     conv2d_k3_f16x3_kernel      one source, staged as it is                      (CAT = false)
//   conv2d_gn_f16x3.hip  conv2d_k3_cat_f16x3_kernel  two sources, each optionally normalised in staging (CAT = true)
// Tile, LDS layout, MFMA sequence, epilogue and saturation counting are one piece of code; only the staging of X differs.  The header of
// conv2d_f16x3.hip describes the arithmetic and the tile.
//
// CAT staging.  The K loop runs over the C1/16 chunks of x1 [N,C1,H,W], then over the C2/16 chunks of x2 [N,C2,H,W]: the conv of the
// channel concatenation [x1 ; x2] with an ordinary pack of an OIHW weight with Ci = C1 + C2, without the concatenation being written.
// Each source may bring a table [N][C][2] = (scale, shift) (mphip_groupnorm_affine_table) and a ReLU flag: an in-image pixel is staged as
//     v = x * scale + shift   (a multiply, then an add: -ffp-contract=off),   v = max(v, 0) if the flag is set,
// then scaled and split like any other.  Padding and the ragged edge are zeros OF THE ACTIVATED MAP: a masked pixel stages 0, never
// relu(shift).  A chunk's 16 (scale, shift) pairs are fetched by 32 lanes with the chunk's global loads, parked in 128 bytes of LDS and
// read back (two 16-byte reads per thread) when the chunk is written: nothing of them is live across the MFMAs.  Both sources share the
// accumulator, so they share one power-of-two operand scale: the smaller of the two their range descriptors give.
//
// Two more axes, instantiated by conv2d_lp.hip (the two units above are XDT = YDT = fp32, NP = 3):
//   XDT, YDT  the model dtype (MPHIP_DTYPE_*) of x and of y.  A typed x is loaded with 2-byte loads (any W, any row alignment), kept as it
//             is across the MFMAs and widened when it is written to LDS: a power-of-two scale-up of a half value is exact, so a typed x
//             stages the bits of its widened copy.  A typed y is the fp32 epilogue value rounded once at the store (narrow<YDT>); out_range
//             then describes the ROUNDED values.  The residual is fp32 (`residual`) or in y's dtype (`residual_t`): at most one is set.
//   NP        products per multiply.  3: Wlo*Xhi + Whi*Xhi + Whi*Xlo.  1: Whi*Xhi alone, the autocast(float16) policy: split_f16 becomes
//             the one rounding round_f16(v * scale), no lo half is fetched, staged or read, and LDS holds the hi planes only (18432 +
//             10368 bytes).  The hi plane is [part 0] of every slab of the ordinary pack: the same packed weights serve both.
//
// One more axis, instantiated by conv2d_up2_f16x3.hip (every other unit is UP = 0; the arithmetic of up2 is in that unit's header):
//   UP = 1    the source is up2(x), x [N,Ci,H/2,W/2] (H, W stay the OUTPUT map's): per chunk the 10 x 10 source pixels per channel that
//             the 18 x 18 halo blends from are loaded (7 loads per thread instead of 22), parked in 6400 bytes of LDS and blended when
//             the chunk is written; a halo pixel's (offset of row i0, of row i1, lambda, in-image) and the same per column are two
//             18-entry tables in LDS, computed once per workgroup.  The up-sampled map is never written.
//   UP = 2    the residual is up2(r), r [N,Co,H/2,W/2] (H, W even): staging is the plain one, the epilogue adds the blend of four loads
//             of r; a lane's coordinates depend on its pixel only and are computed once, before the channel loops.
//
// And one instantiated by conv2d_grp_f16x3.hip (every other unit is GRP = false; the unit's header has the contract):
//   GRP       a grouped conv: x is [N,Ci,H,W], the weight [Co,Ci/groups,3,3] in the ordinary pack, and output channel tile `cot` belongs
//             to group cot / grp_cots (grp_cots = 64-channel tiles per group).  The K loop runs over the grp_cig / 16 chunks that start
//             at channel group * grp_cig of an image whose stride is Ci channels.  Nothing else differs.
//
// And one instantiated by conv2d_splitk_f16x3.hip, alone and with GRP (every other unit is SPLIT = false; the unit's header has the contract):
//   SPLIT     one K range of a conv whose reduction is split over gridDim.z workgroups: workgroup z runs chunks [z * nchunks / Z,
//             (z + 1) * nchunks / Z) of the K loop (GRP: of its group's chunks) and stores its raw fp32 accumulators, neither unscaled nor
//             biased, to y + z * part_stride, masked like any store; bias, residual, relu and out_range are not read.
#pragma once
#include <algorithm>

#include "mphip_common.h"
#include "mphip_conv.h"
#include "mphip_f16x3.h"

namespace mphip {

constexpr int C2_KC = 16;                              // input channels per chunk = K of one MFMA
constexpr int C2_COT = 64;                             // output channels per workgroup (2 MFMA row tiles)
constexpr int C2_TH = 16, C2_TW = 16;                  // output pixels per workgroup
constexpr int C2_HH = C2_TH + 2, C2_HW = C2_TW + 2;    // halo tile
constexpr int C2_XV = C2_HH * C2_HW;                   // 324 halo pixels
constexpr int C2_X_PART = 2 * C2_XV * 8;               // halfs per part (hi or lo): [kg][pixel][8]
constexpr int C2_SLAB_HALFS = 2 * 9 * 2 * C2_COT * 8;  // [part][tap][kg][co][8] = 18432 halfs = 36864 B per (co tile, chunk)
constexpr int C2_NTHR = 256;

inline int c2_cots(int Co) { return (Co + C2_COT - 1) / C2_COT; }
inline size_t c2_packed_bytes(int Co, int Ci) { return 16 + (size_t)c2_cots(Co) * (Ci / C2_KC) * C2_SLAB_HALFS * 2; }

inline bool c2_supported(int N, int Ci, int Co, int H, int W) {
    if (N < 1 || Ci < C2_KC || Co < 32 || H < 1 || W < 1 || Ci % C2_KC || Co % 32) return false;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return false;
    if ((unsigned long long)N * Ci * hw >= (1ull << 31) || (unsigned long long)N * Co * hw >= (1ull << 31)) return false;
    return c2_cots(Co) <= 65535;
}

// conv2d_f16x3.hip: launches of its helper kernels for the other unit (a library-computed descriptor of x; the output's descriptor
// before the conv fills it)
void conv2d_range_launch(const float *x, size_t n, float *range, hipStream_t s);
void conv2d_out_range_init_launch(float *range, unsigned nslots, hipStream_t s);

// What the CAT form takes beyond the plain kernel's arguments (x, x_range, Ci of the plain form are the first source's).
struct C2CatArgs {
    const float *aff1;       // table of the first source or NULL
    const float *x2;         // second source or NULL (C2 == 0)
    const float *aff2;
    const float *x2_range;
    int C2, relu1, relu2;
};

// CAT: 128 bytes of LDS for the chunk's (scale, shift) pairs, [channel][2]
template <bool CAT>
__device__ __forceinline__ float *c2_affine_lds() {
    if constexpr (CAT) {
        __shared__ __attribute__((aligned(16))) float pairs[2 * C2_KC];
        return pairs;
    } else {
        return nullptr;
    }
}

// UP = 1: the source patch of a tile.  Halo rows 16k-1 .. 16k+16 of the up-sampled map blend from source rows 8k-1 .. 8k+8 (up2_coord).
constexpr int C2_UP_P = 10;                            // patch rows and columns
constexpr int C2_UP_CS = C2_UP_P * C2_UP_P;            // floats per channel
constexpr int C2_UP_PATCH = C2_KC * C2_UP_CS;          // floats per chunk: 6400 B
constexpr int C2_UP_PI = (C2_UP_PATCH + C2_NTHR - 1) / C2_NTHR;   // 7 loads per thread
// UP = 1: the patch [channel][row][column], then the row table and the column table [18][4] = (offset of i0, offset of i1, lambda, in-image)
template <int UP>
__device__ __forceinline__ float *c2_up2_lds() {
    if constexpr (UP == 1) {
        __shared__ __attribute__((aligned(16))) float up[C2_UP_PATCH + 2 * C2_HH * 4];
        return up;
    } else {
        return nullptr;
    }
}

// One correctly rounded fp32 division of two fp32 values: the fp64 quotient of two 24-bit significands rounded to 24 bits is the
// correctly rounded quotient (53 >= 2 * 24 + 2), whatever the compiler's fp32 division expands to.
__device__ __forceinline__ float div_rn_f32(float a, float b) { return (float)((double)a / (double)b); }

// Row (or column) i in [0, 2l) of up2 of a map with l rows: i0 = i(l-1) div (2l-1), lambda = float(i(l-1) mod (2l-1)) / float(2l-1),
// i1 = min(i0 + 1, l - 1).  Quotient and remainder in closed form (exact integer identities, no wide product and no integer division):
//   i = 2m+1: (m, l-1-m);   i = 2m, m >= 1: (m-1, 2l-1-m);   i = 0: (0, 0).   l == 1 gives (0, 0) and lambda = 0 / 1.
__device__ __forceinline__ void up2_coord(int i, int l, int &i0, int &i1, float &lam) {
    const int m = i >> 1;
    const bool odd = (i & 1) != 0;
    i0 = odd ? m : max(m - 1, 0);
    const int rem = odd ? l - 1 - m : (m ? 2 * l - 1 - m : 0);
    lam = div_rn_f32((float)rem, (float)(2 * l - 1));
    i1 = min(i0 + 1, l - 1);
}
// The blend of up2, every product, sum and 1 - x rounded to fp32 on its own (-ffp-contract=off): horizontal first.
__device__ __forceinline__ float up2_blend(float x00, float x01, float x10, float x11, float mu, float lam) {
    const float om = 1.0f - mu, ol = 1.0f - lam;
    const float ta = x00 * om, tb = x01 * mu, ba = x10 * om, bb = x11 * mu;
    const float top = ta + tb, bot = ba + bb;
    const float ua = top * ol, ub = bot * lam;
    return ua + ub;
}

// SAT: the instantiating unit's saturation counter
template <bool CAT, unsigned long long *SAT, int XDT = MPHIP_DTYPE_F32, int YDT = MPHIP_DTYPE_F32, int NP = 3, int UP = 0, bool GRP = false,
          bool SPLIT = false>
__device__ __forceinline__ void conv2d_k3_tile(const dtype_t<XDT> *__restrict__ x, const float *__restrict__ x_range, const C2CatArgs cat,
                                               const _Float16 *__restrict__ wslabs, const float *__restrict__ whdr,
                                               const float *__restrict__ bias, const float *__restrict__ residual,
                                               dtype_t<YDT> *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W,
                                               int relu, int tiles_w, int tiles_h, unsigned nslots,
                                               const dtype_t<YDT> *__restrict__ residual_t = nullptr, int grp_cig = 0, int grp_cots = 1,
                                               size_t part_stride = 0) {
    static_assert(NP == 3 || NP == 1, "three products (f16x3) or one (the autocast policy)");
    static_assert(!CAT || XDT == MPHIP_DTYPE_F32, "the two-source form stages fp32 sources");
    static_assert(UP == 0 || (!CAT && XDT == MPHIP_DTYPE_F32 && YDT == MPHIP_DTYPE_F32 && NP == 3), "the up2 forms: one fp32 source, three products");
    static_assert(!GRP || (!CAT && XDT == MPHIP_DTYPE_F32 && YDT == MPHIP_DTYPE_F32 && NP == 3 && UP == 0), "the grouped form: one fp32 source, three products");
    static_assert(!SPLIT || (!CAT && XDT == MPHIP_DTYPE_F32 && YDT == MPHIP_DTYPE_F32 && NP == 3 && UP == 0), "the split-K form: one fp32 source, three products");
    constexpr int NPART = NP == 3 ? 2 : 1;                   // operand halves in LDS: hi and lo, or hi alone
    constexpr int W_HALFS = C2_SLAB_HALFS / 2 * NPART;       // of a slab, the planes this kernel fetches
    __shared__ __attribute__((aligned(16))) _Float16 smem[W_HALFS + NPART * C2_X_PART];
    __shared__ unsigned red[4];
    float *const affs = c2_affine_lds<CAT>();
    float *const ups = c2_up2_lds<UP>();   // UP = 1: patch, row table, column table
    _Float16 *const Ws = smem;             // [part][tap][kg][co][8]
    _Float16 *const Xs = smem + W_HALFS;   // [part][kg][pixel][8]

    float x_scale, x_unscale;
    range_scale_block(x_range, x_scale, x_unscale);   // (folds the producer's partial maxima; barriers inside)
    if constexpr (CAT) {
        if (cat.C2) {   // one accumulator, one operand scale: the smaller one keeps both sources inside the f16 range
            float s2, u2;
            range_scale_block(cat.x2_range, s2, u2);
            if (s2 < x_scale) {
                x_scale = s2;
                x_unscale = u2;
            }
        }
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kg = lane >> 5;
    int bid = blockIdx.x;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int n = bid / tiles_h;
    const int cot = blockIdx.y;
    const int h0 = th * C2_TH, w0 = tw * C2_TW;
    const int nch1 = (GRP ? grp_cig : Ci) / C2_KC;              // chunks of the first source (GRP: of this tile's group)
    const int nchunks = nch1 + (CAT ? cat.C2 / C2_KC : 0);
    const size_t HW = (size_t)H * W;
    const unsigned HWu = (unsigned)HW;   // (a chunk's 16 channels hold fewer than 2^31 elements: 32-bit element offsets)
    const int xh = H >> 1, xw = W >> 1;                                 // UP = 1: the source map ...
    const size_t XHW = UP == 1 ? (size_t)xh * xw : HW;                  // ... and a channel of it (else the map itself)
    const int pr0 = h0 ? (h0 >> 1) - 1 : 0, pc0 = w0 ? (w0 >> 1) - 1 : 0;   // UP = 1: the patch's first row and column (i0 of the halo's first)
    const dtype_t<XDT> *xn = x + (size_t)n * Ci * XHW;
    if constexpr (GRP) xn += (size_t)(cot / grp_cots) * grp_cig * XHW;   // the group's first channel; the image stride stays Ci
    const float *const x2n = CAT && cat.C2 ? cat.x2 + (size_t)n * cat.C2 * HW : nullptr;

    // X staging: an item is (channel pair p, halo pixel r): two 4-byte loads (the zero padding and the ragged edge are the mask), scale,
    // split, one b32 write of hi and one of lo.  The four pairs of a 16-byte fragment go to neighbouring lanes: conflict-free writes.
    constexpr int NX = 8 * C2_XV;                        // items per chunk
    constexpr int XI = (NX + C2_NTHR - 1) / C2_NTHR;     // 11 per thread
    constexpr int WPIECES = W_HALFS * 2 / 16;            // 16-byte pieces of the weight planes fetched
    constexpr int WI = (WPIECES + C2_NTHR - 1) / C2_NTHR; // 9 per thread; hi plane alone: 4, and a fifth in the lower half of the threads
    constexpr bool W_WHOLE = WPIECES % C2_NTHR == 0;
    constexpr int W_LAST = WPIECES - (WI - 1) * C2_NTHR;   // threads that take a piece in the last round
    static_assert(C2_SLAB_HALFS * 2 % (16 * C2_NTHR) == 0, "weight slab / thread count");
    static_assert(C2_NTHR % 4 == 0, "a thread's items all belong to channel pair (tid & 3) of their k group");
    dtype_t<XDT> xa[XI], xb[XI];   // as loaded: widened when written to LDS
    float pv[UP == 1 ? C2_UP_PI : 1];   // UP = 1: the chunk's patch, from its loads to LDS, instead of xa / xb
    float affv = 0.0f;   // CAT: lanes 0-31 carry the next chunk's table entries from its loads to LDS
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 wq[WI];
    unsigned sat = 0, okm = 0;
#define C2_LOAD_CHUNK(c_)                                                                              \
    {                                                                                                  \
        const dtype_t<XDT> *xc_ = xn + (size_t)(c_) * C2_KC * XHW;                                     \
        if constexpr (CAT) {                                                                           \
            const bool first_ = (c_) < nch1;   /* workgroup-uniform */                                 \
            if (!first_) xc_ = x2n + (size_t)((c_) - nch1) * C2_KC * HW;                               \
            const float *const tab_ = first_ ? cat.aff1 : cat.aff2;                                    \
            const size_t ch_ = first_ ? (size_t)n * Ci + (size_t)(c_) * C2_KC : (size_t)n * cat.C2 + (size_t)((c_) - nch1) * C2_KC; \
            if (tab_ && tid < 2 * C2_KC) affv = tab_[ch_ * 2 + tid];                                   \
        }                                                                                              \
        int tid_ = tid;                                                                                \
        asm volatile("" : "+v"(tid_)); /* opaque: keeps the per-item offsets out of registers across the K loop */ \
        if constexpr (UP == 1) {   /* the patch: rows and columns clamped at the source map's last */  \
            _Pragma("unroll") for (int i = 0; i < C2_UP_PI; ++i) {                                     \
                const int e_ = min(i * C2_NTHR + tid_, C2_UP_PATCH - 1), q_ = e_ % C2_UP_CS;           \
                const unsigned off_ = (unsigned)(e_ / C2_UP_CS) * (unsigned)XHW + (unsigned)min(pr0 + q_ / C2_UP_P, xh - 1) * xw + \
                                      min(pc0 + q_ % C2_UP_P, xw - 1);                                 \
                pv[i] = xc_[off_];                                                                     \
            }                                                                                          \
        } else {                                                                                       \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                               \
            const int e_ = i * C2_NTHR + tid_, ec_ = min(e_, NX - 1);                                  \
            const int rest_ = ec_ >> 2;                                                                \
            const int p_ = (rest_ / C2_XV) * 4 + (ec_ & 3), r_ = rest_ % C2_XV;                        \
            const int gh_ = h0 - 1 + r_ / C2_HW, gw_ = w0 - 1 + r_ % C2_HW;                            \
            const bool ok_ = e_ < NX && (unsigned)gh_ < (unsigned)H && (unsigned)gw_ < (unsigned)W;    \
            /* unconditional loads from a clamped (always valid) address, a select later: no branch per load */ \
            const unsigned off_ = (unsigned)(2 * p_) * HWu + (unsigned)min(max(gh_, 0), H - 1) * W + min(max(gw_, 0), W - 1); \
            xa[i] = xc_[off_];                                                                         \
            xb[i] = xc_[off_ + HWu];                                                                   \
            okm = ok_ ? okm | (1u << i) : okm & ~(1u << i);   /* the select waits until the values are written to LDS */ \
        }                                                                                              \
        }                                                                                              \
        /* opaque: with a third of the MFMAs hipcc else keeps the 11 lane masks in scalar pairs and spills kernel arguments */ \
        if constexpr (NP == 1) asm volatile("" : "+v"(okm));                                           \
        const u32x4 *const ws_ = reinterpret_cast<const u32x4 *>(wslabs + ((size_t)cot * nchunks + (c_)) * C2_SLAB_HALFS); \
        _Pragma("unroll") for (int i = 0; i < WI; ++i)                                                 \
            if (W_WHOLE || i < WI - 1 || tid_ < W_LAST) wq[i] = ws_[i * C2_NTHR + tid_];              \
    }
    // CAT: parks the loaded chunk's table entries in LDS; a barrier separates it from C2_WRITE_CHUNK, whose reads of the previous
    // chunk's entries lie before the barrier that closed that write
#define C2_PARK_AFFINE()                                                                               \
    if constexpr (CAT) {                                                                               \
        if (tid < 2 * C2_KC) affs[tid] = affv;                                                         \
    }                                                                                                  \
    if constexpr (UP == 1) {   /* the loaded chunk's patch, under the same two barriers */             \
        _Pragma("unroll") for (int i = 0; i < C2_UP_PI; ++i)                                           \
            if (i * C2_NTHR + tid < C2_UP_PATCH) ups[i * C2_NTHR + tid] = pv[i];                       \
    }
#define C2_WRITE_CHUNK(c_)                                                                             \
    {                                                                                                  \
        bool aff_on_ = false, relu_on_ = false;   /* workgroup-uniform */                              \
        f32x4 q0_ = {1.0f, 0.0f, 1.0f, 0.0f}, q1_ = q0_;   /* (scale, shift) of channels 2p, 2p + 1: p = tid & 3 of k group 0 and of 1 */ \
        if constexpr (CAT) {                                                                           \
            const bool first_ = (c_) < nch1;                                                           \
            aff_on_ = (first_ ? cat.aff1 : cat.aff2) != nullptr;                                       \
            relu_on_ = (first_ ? cat.relu1 : cat.relu2) != 0;                                          \
            if (aff_on_) {                                                                             \
                q0_ = *reinterpret_cast<const f32x4 *>(affs + (tid & 3) * 4);                          \
                q1_ = *reinterpret_cast<const f32x4 *>(affs + C2_KC + (tid & 3) * 4);                  \
            }                                                                                          \
        }                                                                                              \
        int tid_ = tid;                                                                                \
        asm volatile("" : "+v"(tid_));                                                                 \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                               \
            const int e_ = i * C2_NTHR + tid_;                                                         \
            if (e_ < NX) {                                                                             \
                const int dst_ = (e_ >> 2) * 8 + (e_ & 3) * 2;   /* e_ >> 2 = kg * C2_XV + pixel */    \
                bool ok_;                                                                              \
                float a_, b_;                                                                          \
                if constexpr (UP == 1) {   /* the halo pixel's two table entries, four patch values per channel */ \
                    const int rest_ = e_ >> 2, r_ = rest_ % C2_XV;                                     \
                    const u32x4 rt_ = *reinterpret_cast<const u32x4 *>(ups + C2_UP_PATCH + (r_ / C2_HW) * 4);           \
                    const u32x4 ct_ = *reinterpret_cast<const u32x4 *>(ups + C2_UP_PATCH + (C2_HH + r_ % C2_HW) * 4);   \
                    const float *const pa_ = ups + (2 * ((rest_ / C2_XV) * 4 + (e_ & 3))) * C2_UP_CS;  \
                    const float lam_ = __uint_as_float(rt_[2]), mu_ = __uint_as_float(ct_[2]);         \
                    const unsigned o00_ = rt_[0] + ct_[0], o01_ = rt_[0] + ct_[1], o10_ = rt_[1] + ct_[0], o11_ = rt_[1] + ct_[1]; \
                    a_ = up2_blend(pa_[o00_], pa_[o01_], pa_[o10_], pa_[o11_], mu_, lam_);             \
                    b_ = up2_blend(pa_[C2_UP_CS + o00_], pa_[C2_UP_CS + o01_], pa_[C2_UP_CS + o10_], pa_[C2_UP_CS + o11_], mu_, lam_); \
                    ok_ = (rt_[3] & ct_[3]) != 0;   /* outside the up-sampled map: a zero of that map */ \
                } else {                                                                               \
                    ok_ = (okm >> i) & 1u;                                                             \
                    a_ = widen(xa[i]), b_ = widen(xb[i]);                                              \
                }                                                                                      \
                if constexpr (CAT) {                                                                   \
                    if (aff_on_) {                                                                     \
                        /* the item's k group: known at compile time except for the one i that straddles 4 * C2_XV */ \
                        const bool k1_ = i * C2_NTHR >= 4 * C2_XV || ((i + 1) * C2_NTHR > 4 * C2_XV && tid >= 4 * C2_XV - i * C2_NTHR); \
                        const f32x4 q_ = k1_ ? q1_ : q0_;                                              \
                        a_ = a_ * q_[0];                                                               \
                        a_ = a_ + q_[1];                                                               \
                        b_ = b_ * q_[2];                                                               \
                        b_ = b_ + q_[3];                                                               \
                        if (relu_on_) {                                                                \
                            a_ = a_ < 0.0f ? 0.0f : a_;   /* (keeps NaN, like torch's relu) */         \
                            b_ = b_ < 0.0f ? 0.0f : b_;                                                \
                        }                                                                              \
                    }                                                                                  \
                }                                                                                      \
                const float v0_ = ok_ ? a_ * x_scale : 0.0f, v1_ = ok_ ? b_ * x_scale : 0.0f;          \
                sat += !(fabsf(v0_) <= F16_CLAMP) + !(fabsf(v1_) <= F16_CLAMP);   /* NaN counts */     \
                if constexpr (NP == 3) {                                                               \
                    _Float16 hA_, lA_, hB_, lB_;                                                       \
                    split_f16(v0_, hA_, lA_);                                                          \
                    split_f16(v1_, hB_, lB_);                                                          \
                    const half2v hv_ = {hA_, hB_}, lv_ = {lA_, lB_};                                   \
                    *reinterpret_cast<half2v *>(Xs + dst_) = hv_;                                      \
                    *reinterpret_cast<half2v *>(Xs + C2_X_PART + dst_) = lv_;                          \
                } else {   /* one rounding (|v| > 65504 -> +-Inf, NaN -> NaN, like split_f16's hi) */  \
                    const half2v hv_ = {(_Float16)v0_, (_Float16)v1_};                                 \
                    *reinterpret_cast<half2v *>(Xs + dst_) = hv_;                                      \
                }                                                                                      \
            }                                                                                          \
        }                                                                                              \
        _Pragma("unroll") for (int i = 0; i < WI; ++i)                                                 \
            if (W_WHOLE || i < WI - 1 || tid_ < W_LAST) reinterpret_cast<u32x4 *>(Ws)[i * C2_NTHR + tid_] = wq[i]; \
    }

    // ds_read_b128 is serviced in 16-lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} per half-wave: slot jv gives each group one
    // whole 16-pixel row (256 contiguous bytes = every bank once).  Slots only name accumulator columns, any bijection works.
    const int jg = ((j >> 2) & 1) ^ ((j >> 3) & 1) ^ ((j >> 4) & 1);
    const int jpos = j < 4 ? j : j < 12 ? j - 4 : j < 20 ? j - 8 : j < 28 ? j - 12 : j - 16;
    const int jv = jg * 16 + jpos;
    const int prow = wave * 4 + (jv >> 4), pcol = jv & 15;       // this lane's pixel in column tile t: (prow + 2t, pcol)
    const int a_base = (kg * C2_COT + j) * 8;                    // + ((part*9 + tap)*2*64 + m*32)*8
    const int b_base = (kg * C2_XV + prow * C2_HW + pcol) * 8;   // + (t*2*18 + tap offset)*8

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;

    if constexpr (UP == 1) {   // the two tables: thread k < 18 halo row k, thread 18 + k halo column k
        if (tid < 2 * C2_HH) {
            const bool col = tid >= C2_HH;
            const int L = col ? W : H, g = (col ? w0 : h0) - 1 + (col ? tid - C2_HH : tid);
            int i0, i1;
            float lam;
            up2_coord(min(max(g, 0), L - 1), L >> 1, i0, i1, lam);
            // (both rows lie inside the patch, see C2_UP_P; the clamp keeps every offset inside it whatever the arguments)
            const int base = col ? pc0 : pr0, step = col ? 1 : C2_UP_P;
            const u32x4 ent = {(unsigned)(min(max(i0 - base, 0), C2_UP_P - 1) * step), (unsigned)(min(max(i1 - base, 0), C2_UP_P - 1) * step),
                               __float_as_uint(lam), (unsigned)g < (unsigned)L ? 1u : 0u};
            *reinterpret_cast<u32x4 *>(ups + C2_UP_PATCH + tid * 4) = ent;
        }
    }
    int c_lo = 0, c_hi = nchunks;   // the K range of this workgroup: all of it unless SPLIT
    if constexpr (SPLIT) {
        const int z = blockIdx.z, nz = gridDim.z;
        c_lo = z * nchunks / nz, c_hi = (z + 1) * nchunks / nz;
    }
    C2_LOAD_CHUNK(c_lo)
    if constexpr (CAT || UP == 1) {
        C2_PARK_AFFINE()
        __syncthreads();
    }
    C2_WRITE_CHUNK(c_lo)
    __syncthreads();
    for (int c = c_lo; c < c_hi; ++c) {
        const bool more = c + 1 < c_hi;
        if (more) C2_LOAD_CHUNK(c + 1)   // in flight during this chunk's MFMAs
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            half8 ah[2], al[2], bh[2], bl[2];
            const int toff = ((tap / 3) * C2_HW + tap % 3) * 8;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                ah[m] = *reinterpret_cast<const half8 *>(Ws + a_base + (tap * 2 * C2_COT + m * 32) * 8);
                if constexpr (NP == 3) al[m] = *reinterpret_cast<const half8 *>(Ws + C2_SLAB_HALFS / 2 + a_base + (tap * 2 * C2_COT + m * 32) * 8);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                bh[t] = *reinterpret_cast<const half8 *>(Xs + b_base + t * 2 * C2_HW * 8 + toff);
                if constexpr (NP == 3) bl[t] = *reinterpret_cast<const half8 *>(Xs + C2_X_PART + b_base + t * 2 * C2_HW * 8 + toff);
            }
            if constexpr (NP == 3) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[m], bh[t], acc[m][t], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bh[t], acc[m][t], 0, 0, 0);
            if constexpr (NP == 3) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bl[t], acc[m][t], 0, 0, 0);
            }
        }
        if (more) {
            C2_PARK_AFFINE()
            __syncthreads();   // every wave is past its last fragment read of this chunk
            C2_WRITE_CHUNK(c + 1)
            __syncthreads();
        }
    }

#undef C2_LOAD_CHUNK
#undef C2_PARK_AFFINE
#undef C2_WRITE_CHUNK

    // epilogue: unscale (two powers of two, one after the other: their product can underflow where the result does not), bias, residual,
    // ReLU in fp32; stores masked at the ragged edge and past Co
    const Unscale u = {SPLIT ? 0.0f : whdr[0], x_unscale};   // (SPLIT: no header is read)
    unsigned ymax = 0;
    unsigned ro[2][4];          // UP = 2: this lane's four offsets into a channel of r, per column tile, ...
    float rlam[2], rmu = 0.0f;  // ... and its weights
    if constexpr (UP == 2) {
        int j0, j1;
        up2_coord(min(w0 + pcol, W - 1), xw, j0, j1, rmu);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            int i0, i1;
            up2_coord(min(h0 + prow + 2 * t, H - 1), xh, i0, i1, rlam[t]);
            ro[t][0] = (unsigned)i0 * xw + j0, ro[t][1] = (unsigned)i0 * xw + j1;
            ro[t][2] = (unsigned)i1 * xw + j0, ro[t][3] = (unsigned)i1 * xw + j1;
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int co0 = cot * C2_COT + m * 32;
        if (co0 < Co) {   // (Co % 32 == 0: a row tile is whole or absent; workgroup-uniform)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int gh = h0 + prow + 2 * t, gw = w0 + pcol;
                if (gh < H && gw < W) {
                    const size_t o = ((size_t)n * Co + co0 + 4 * kg) * HW + (size_t)gh * W + gw;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = (reg & 3) + 8 * (reg >> 2);
                        const size_t oi = o + (size_t)row * HW;
                        if constexpr (SPLIT) {   // the raw accumulator of this K range: the finish kernel owns the epilogue
                            y[(size_t)blockIdx.z * part_stride + oi] = acc[m][t][reg];
                            continue;
                        }
                        float v = unscaled(acc[m][t][reg], u, bias[co0 + 4 * kg + row]);
                        if constexpr (UP == 2) {   // + up2(r): the blend, then one add
                            const float *const rc = residual + ((size_t)n * Co + co0 + 4 * kg + row) * ((size_t)xh * xw);
                            v += up2_blend(rc[ro[t][0]], rc[ro[t][1]], rc[ro[t][2]], rc[ro[t][3]], rmu, rlam[t]);
                        } else {
                            if (residual) v += residual[oi];
                        }
                        if constexpr (YDT != MPHIP_DTYPE_F32) {
                            if (residual_t) v += widen(residual_t[oi]);   // (workgroup-uniform; at most one of the two is set)
                        }
                        if (relu) v = v < 0.0f ? 0.0f : v;   // (keeps NaN, like torch's relu)
                        const dtype_t<YDT> vy = narrow<YDT>(v);   // the one rounding of a typed y
                        y[oi] = vy;
                        ymax = max(ymax, range_bits(widen(vy)));   // of the value the next conv reads
                    }
                }
            }
        }
    }
    if (!SPLIT && out_range) {   // workgroup-uniform
        ymax = wave_umax(ymax);
        if (lane == 0) red[wave] = ymax;
        __syncthreads();
        if (tid == 0) {
            const unsigned mx = max(max(red[0], red[1]), max(red[2], red[3]));
            const unsigned slot = (blockIdx.x + gridDim.x * blockIdx.y) % nslots;
            if (mx) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + slot, mx);
        }
    }
    if (__builtin_amdgcn_ballot_w64(sat != 0) != 0) {  // never taken in normal operation
        unsigned tot = sat;
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) tot += __shfl_xor(tot, sft, 64);
        if (lane == 0) atomicAdd(SAT, (unsigned long long)tot);
    }
}

}  // namespace mphip
