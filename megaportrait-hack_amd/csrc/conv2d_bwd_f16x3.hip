// Conv2d 3x3 (stride 1, padding 1) backward-weight on the f16 matrix cores with split precision ("f16x3"), NCHW fp32:
//   dW[co][ci][kh][kw] = sum_{n,h,w} dY[n][co][h][w] * X[n][ci][h+kh-1][w+kw-1]      (zero padding)
// The arithmetic is conv3d_bwd_f16x3.hip's with the depth axis dropped: both operands are scaled by their own power of two and split
// v*S = hi + lo (two f16) while the tile is staged; each product is lo*hi + hi*lo + hi*hi accumulated in fp32 by
// v_mfma_f32_32x32x16_f16.  X is scaled from its range descriptor (range_scale_block), dY by the explicit scale mphip_grad_prep writes
// (S = H*W: the same pass yields the bias gradient).  Non-finite values are not clamped: they propagate, so a GradScaler sees an overflow.
//
// GEMM view per tap: M = co, N = ci, K = pixels.  A lane's K group is 8 consecutive W pixels of one row: dY fragments are 16-byte LDS
// reads, and the three kw fragments of a 10-pixel halo row come from ONE 20-byte read shifted with v_alignbit.
//
// Workgroup = 4 waves on a (64 co x 64 ci) block of all 9 taps, streaming 8 x 8-pixel tiles of its pixel range.  Wave w owns the
// 32 x 32 block (co-tile w & 1, ci-tile w >> 1) of all 3 kh x 3 kw taps: 9 accumulators (144 registers), and per 16-pixel K step
// 2 + 6 fragment reads feed 27 MFMAs.  The co tile is 64 (the body's channel counts are 64 .. 512: a 96-wide tile would idle a third of
// the MFMAs at Co = 64).  LDS: (hi plane + lo plane) x (64 x 72 + 64 x 124) f16 = 50176 bytes, single buffered: inside a workgroup
// staging (through registers, between two barriers, as in the 3-D kernel) and the MFMAs are serial.  The kernel is held to 256
// registers so that two workgroups share a CU: whatever overlap there is comes from the second resident workgroup, which may stage
// while the first multiplies.  At 64 -> 64 channels on a 512 x 512 map the slabs are 512 x 64 x 64 x 9 floats = 75 MB, written once and
// read once by the reduce; profiles/g2d_body_train_timing.json has the one launch that was timed on its own (512 -> 512 at 64 x 64).
//
// Split over pixels: workgroup z accumulates tiles [z * tps, (z + 1) * tps) and stores its RAW fp32 accumulators (still in the scaled
// domain: always finite for finite inputs) to slab z with plain stores, every element of it; the slab reduce sums the slabs in z order
// and only then applies the unscale, as two factors one after the other (1 / scale_dy, then 1 / scale_x: their single product can leave
// the fp32 range although the result does not, and partial sums unscaled before the reduce could overflow to +Inf and -Inf and meet as
// NaN).  No floating-point atomics, no memset: the result is bit-reproducible and the launches can be captured.  The two factors travel
// from the conv kernel to the reduce through two floats of the workspace (workgroup (0, 0) writes them).
//
// Two instantiations: VEC (W % 8 == 0: every tile row is whole and 16-byte aligned when x and dy are, so rows are two float4 loads) and
// the masked one (any W: element loads, each masked against the map's edge).  H, ragged channel blocks and the last tile are masked in both.
#include "conv2d_f16x3_tile.h"

namespace mphip {

typedef unsigned b2_u32x4 __attribute__((ext_vector_type(4)));

constexpr int B2_CO = 64, B2_CI = 64;               // channel block of a workgroup
constexpr int B2_TH = 8, B2_TW = 8;                 // pixel tile: 4 K steps of 16 pixels (2 rows of 8)
constexpr int B2_AP = B2_TH * B2_TW + 8;            // halves per co row of the dY tile: 64 pixels + 8 (pitch 36 dwords)
constexpr int B2_XROW = 12;                         // halves per halo row: 10 pixels + 2 (24 B, 8-B aligned)
constexpr int B2_XCI = (B2_TH + 2) * B2_XROW + 4;   // halves per input channel: 10 halo rows (+4: pitch 62 dwords, 8-B aligned)
constexpr int B2_A_PART = B2_CO * B2_AP;
constexpr int B2_X_PART = B2_CI * B2_XCI;
constexpr int B2_NTHR = 256;
constexpr int B2_TARGET_WGS = 512;                  // two workgroups per CU on 256 CUs: what (channel blocks) x splits fills
constexpr size_t B2_WS_HEAD = (size_t)MPHIP_RANGE_FLOATS * sizeof(float) + 256;   // descriptor slot of x, then the two unscale factors
static_assert(B2_WS_HEAD % 16 == 0, "the slabs start 16-byte aligned");
static_assert((B2_AP * 2) % 16 == 0 && (B2_XCI * 2) % 8 == 0 && (B2_XROW * 2) % 8 == 0, "fragment reads are aligned");

__device__ __forceinline__ half8 b2_as_half8(unsigned a, unsigned b, unsigned c, unsigned d) {
    b2_u32x4 u = {a, b, c, d};
    return __builtin_bit_cast(half8, u);
}

// the three kw-shifted 8-pixel fragments of one halo row (10 halves at `row`, 8-B aligned)
__device__ __forceinline__ void b2_halo_row_frags(const _Float16 *row, half8 f[3]) {
    const uint2 a = *reinterpret_cast<const uint2 *>(row);
    const uint2 b = *reinterpret_cast<const uint2 *>(row + 4);
    const unsigned c = *reinterpret_cast<const unsigned *>(row + 8);
    f[0] = b2_as_half8(a.x, a.y, b.x, b.y);
    f[1] = b2_as_half8(__builtin_amdgcn_alignbit(a.y, a.x, 16), __builtin_amdgcn_alignbit(b.x, a.y, 16),
                       __builtin_amdgcn_alignbit(b.y, b.x, 16), __builtin_amdgcn_alignbit(c, b.y, 16));
    f[2] = b2_as_half8(a.y, b.x, b.y, c);
}

#define B2_MFMA3(ACC, AH, AL, BH, BL)                                           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(AL, BH, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(AH, BL, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(AH, BH, ACC, 0, 0, 0);

template <bool VEC>
__global__ void __launch_bounds__(B2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_bwd_weight_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ gscale,
                               const float *__restrict__ x_range, float *__restrict__ slabs, float *__restrict__ unscale_out, int N, int Ci,
                               int Co, int H, int W, int tiles_h, int tiles_w, int tiles_per_split) {
    __shared__ __attribute__((aligned(16))) _Float16 smem[2 * B2_A_PART + 2 * B2_X_PART];
    _Float16 *const As = smem;                  // [part][co 64][B2_AP]
    _Float16 *const Xs = smem + 2 * B2_A_PART;  // [part][ci 64][row 10][B2_XROW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kb = lane >> 5;
    const size_t HW = (size_t)H * W;
    const int ci_blocks = (Ci + B2_CI - 1) / B2_CI;
    const int ci0 = (blockIdx.x % ci_blocks) * B2_CI;
    const int co0 = (blockIdx.x / ci_blocks) * B2_CO;
    const int ntiles = N * tiles_h * tiles_w;
    const int t_begin = blockIdx.z * tiles_per_split;
    const int t_end = min(ntiles, t_begin + tiles_per_split);
    const float dscale = gscale[0];
    float xscale, xinv;   // the saved activation's own operand scale (its range descriptor)
    range_scale_block(x_range, xscale, xinv);
    if (blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) {   // what the slab reduce unscales with: two factors, never their product
        unscale_out[0] = gscale[1];
        unscale_out[1] = xinv;
    }
    const int cot = wave & 1, cit = wave >> 1;   // this wave's 32 co x 32 ci block

    f32x16 acc[3][3];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kh][t][r] = 0.0f;

    for (int tile = t_begin; tile < t_end; ++tile) {
        int r_ = tile;
        const int tw = r_ % tiles_w; r_ /= tiles_w;
        const int th = r_ % tiles_h;
        const int n = r_ / tiles_h;
        const int h0 = th * B2_TH, w0 = tw * B2_TW;
        __syncthreads();  // the previous tile is fully consumed
        int tz = 0;
        asm volatile("" : "+v"(tz));  // opaque 0, new per tile: keeps the staging code's index math out of registers held across the MFMAs
        {   // ---- dY tile: 64 co x 8 rows of 8 pixels, 2 rows per thread
            float v[2][8];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q = tid + i * B2_NTHR + tz, co = q >> 3, rr = q & 7;
                const int gh = h0 + rr;
                const bool ok = co0 + co < Co && gh < H;
                const float *p = dy + (ok ? ((size_t)n * Co + co0 + co) * HW + (size_t)gh * W + w0 : 0);
                if constexpr (VEC) {
                    float4 a = *reinterpret_cast<const float4 *>(p);
                    float4 b = *reinterpret_cast<const float4 *>(p + 4);
                    if (!ok) a = b = make_float4(0.f, 0.f, 0.f, 0.f);
                    v[i][0] = a.x; v[i][1] = a.y; v[i][2] = a.z; v[i][3] = a.w;
                    v[i][4] = b.x; v[i][5] = b.y; v[i][6] = b.z; v[i][7] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool oke = ok && w0 + e < W;
                        const float t = *(oke ? p + e : dy);
                        v[i][e] = oke ? t : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q = tid + i * B2_NTHR + tz, co = q >> 3, rr = q & 7;
                half8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    _Float16 h, l;
                    split_f16(v[i][e] * dscale, h, l);
                    hi[e] = h;
                    lo[e] = l;
                }
                *reinterpret_cast<half8 *>(As + co * B2_AP + rr * 8) = hi;
                *reinterpret_cast<half8 *>(As + B2_A_PART + co * B2_AP + rr * 8) = lo;
            }
        }
        {   // ---- X halo: 64 ci x 10 rows of 10 pixels (zero outside the map), <= 3 rows per thread
            float v[3][10];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int q = tid + i * B2_NTHR + tz;
                const int ci = q / 10, pr = q % 10;
                const int gh = h0 - 1 + pr;
                const bool ok = q < B2_CI * 10 && ci0 + ci < Ci && (unsigned)gh < (unsigned)H;
                const float *p = x + (ok ? ((size_t)n * Ci + ci0 + ci) * HW + (size_t)gh * W + w0 : 0);
                if constexpr (VEC) {
                    const bool okl = ok && w0 > 0, okr = ok && w0 + 8 < W;
                    float4 a = *reinterpret_cast<const float4 *>(p);
                    float4 b = *reinterpret_cast<const float4 *>(p + 4);
                    const float l = *(okl ? p - 1 : x), r = *(okr ? p + 8 : x);
                    if (!ok) a = b = make_float4(0.f, 0.f, 0.f, 0.f);
                    v[i][0] = okl ? l : 0.0f;
                    v[i][1] = a.x; v[i][2] = a.y; v[i][3] = a.z; v[i][4] = a.w;
                    v[i][5] = b.x; v[i][6] = b.y; v[i][7] = b.z; v[i][8] = b.w;
                    v[i][9] = okr ? r : 0.0f;
                } else {
#pragma unroll
                    for (int e = 0; e < 10; ++e) {
                        const int col = w0 - 1 + e;
                        const bool oke = ok && (unsigned)col < (unsigned)W;
                        const float t = *(oke ? p + (e - 1) : x);
                        v[i][e] = oke ? t : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int q = tid + i * B2_NTHR + tz;
                if (q < B2_CI * 10) {
                    const int ci = q / 10, pr = q % 10;
                    half2v hp[5], lp[5];
#pragma unroll
                    for (int e = 0; e < 5; ++e) {
                        _Float16 h0_, l0_, h1_, l1_;
                        split_f16(v[i][2 * e] * xscale, h0_, l0_);
                        split_f16(v[i][2 * e + 1] * xscale, h1_, l1_);
                        hp[e] = half2v{h0_, h1_};
                        lp[e] = half2v{l0_, l1_};
                    }
                    _Float16 *dst = Xs + ci * B2_XCI + pr * B2_XROW;
#pragma unroll
                    for (int e = 0; e < 5; ++e) {
                        *reinterpret_cast<half2v *>(dst + 2 * e) = hp[e];
                        *reinterpret_cast<half2v *>(dst + B2_X_PART + 2 * e) = lp[e];
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < B2_TH / 2; ++ks) {
            const int hrow = 2 * ks + kb;   // this lane's K group: row hrow of the tile, its 8 pixels
            const _Float16 *arow = As + (cot * 32 + j) * B2_AP + hrow * 8;
            const half8 ah = *reinterpret_cast<const half8 *>(arow);
            const half8 al = *reinterpret_cast<const half8 *>(arow + B2_A_PART);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                half8 bh[3], bl[3];
                const _Float16 *xrow = Xs + (cit * 32 + j) * B2_XCI + (hrow + kh) * B2_XROW;
                b2_halo_row_frags(xrow, bh);
                b2_halo_row_frags(xrow + B2_X_PART, bl);
#pragma unroll
                for (int t = 0; t < 3; ++t) { B2_MFMA3(acc[kh][t], ah, al, bh[t], bl[t]) }
            }
        }
    }

    // slab layout [9][Co][Ci] (a store covers 32 consecutive ci); C/D: column = lane&31 = ci, rows = co.  Raw accumulators: the reduce unscales.
    float *slab = slabs + (size_t)blockIdx.z * Co * Ci * 9;
    const int ci = ci0 + cit * 32 + j;
    if (ci < Ci) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int co = co0 + cot * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kb;
                    if (co < Co) slab[((size_t)(kh * 3 + t) * Co + co) * Ci + ci] = acc[kh][t][reg];
                }
    }
}

// slabs [split][9][Co*Ci] (ci contiguous: the kernel's stores are coalesced) -> OIHW [Co*Ci][9], summed in split order, then unscaled by
// the two factors in turn; 64 (co,ci) pairs per workgroup, transposed through LDS so reads and writes are both contiguous.
__global__ void __launch_bounds__(256)
conv2d_bwd_slab_reduce_kernel(const float *__restrict__ slabs, const float *__restrict__ unscale, float *__restrict__ out, size_t ncc,
                              int splits) {
    __shared__ float tile[64 * 9];
    const float u_dy = unscale[0], u_x = unscale[1];
    const size_t cc0 = (size_t)blockIdx.x * 64;
    const int c = threadIdx.x & 63;
    for (int tap = threadIdx.x >> 6; tap < 9; tap += 4)
        if (cc0 + c < ncc) tile[c * 9 + tap] = (sum_slabs(slabs, splits, ncc * 9, (size_t)tap * ncc + cc0 + c) * u_dy) * u_x;
    __syncthreads();
    const size_t n_here = min((size_t)64, ncc - cc0) * 9;
    for (size_t i = threadIdx.x; i < n_here; i += 256) out[cc0 * 9 + i] = tile[i];
}

// The one decision of a launch: the launcher, the workspace size and mphip_debug_conv2d_bwd_weight_plan all read it.
struct Conv2dBwdWeightPlan {
    int kernel;   // 0 = the shape is not supported, 1 = the VEC instantiation (W % 8 == 0), 2 = the masked one
    int splits;   // slabs = grid z; the slab reduce folds them in order
    int tps;      // pixel tiles per split (the last split may hold fewer)
    int ntiles;   // N x ceil(H / 8) x ceil(W / 8)
    int bxy;      // (ci, co) blocks = grid x
    int tiles_h, tiles_w;
};

static bool conv2d_bwd_weight_ok(int N, int Ci, int Co, int H, int W) { return c2_supported(N, Ci, Co, H, W); }

// (channel blocks) x splits fills the part once with two workgroups per CU; a launch with few channel blocks (64 -> 64 channels on a
// 512 x 512 map: one) takes nearly all of its parallelism from the split
static Conv2dBwdWeightPlan conv2d_bwd_weight_plan(int N, int Ci, int Co, int H, int W) {
    Conv2dBwdWeightPlan p = {0, 0, 0, 0, 0, 0, 0};
    if (!conv2d_bwd_weight_ok(N, Ci, Co, H, W)) return p;
    p.tiles_h = (H + B2_TH - 1) / B2_TH;
    p.tiles_w = (W + B2_TW - 1) / B2_TW;
    const long ntiles = (long)N * p.tiles_h * p.tiles_w;   // <= N * H * W < 2^31
    p.bxy = ((Ci + B2_CI - 1) / B2_CI) * ((Co + B2_CO - 1) / B2_CO);
    long sp = p.bxy >= B2_TARGET_WGS ? 1 : B2_TARGET_WGS / p.bxy;
    if (sp > ntiles) sp = ntiles;
    p.kernel = W % 8 == 0 ? 1 : 2;
    p.ntiles = (int)ntiles;
    p.tps = (int)((ntiles + sp - 1) / sp);
    p.splits = (int)((ntiles + p.tps - 1) / p.tps);
    return p;
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_bwd_weight_supported(int N, int Ci, int Co, int H, int W) { return conv2d_bwd_weight_ok(N, Ci, Co, H, W) ? 1 : 0; }

extern "C" size_t mphip_conv2d_bwd_weight_workspace_bytes(int N, int Ci, int Co, int H, int W) {
    const Conv2dBwdWeightPlan p = conv2d_bwd_weight_plan(N, Ci, Co, H, W);
    return p.kernel ? B2_WS_HEAD + (size_t)p.splits * Co * Ci * 9 * sizeof(float) : 0;
}

extern "C" int mphip_debug_conv2d_bwd_weight_plan(int N, int Ci, int Co, int H, int W, int out[4]) {
    if (!out) return 0;
    const Conv2dBwdWeightPlan p = conv2d_bwd_weight_plan(N, Ci, Co, H, W);
    out[0] = p.kernel, out[1] = p.splits, out[2] = p.tps, out[3] = p.ntiles;
    return 1;
}

extern "C" int mphip_conv2d_bwd_weight(const float *x, const float *x_range, const float *dy, const float *dy_scale, float *dw, int N, int Ci,
                                       int Co, int H, int W, void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(x && dy && dy_scale && dw, "conv2d_bwd_weight: null pointer");
    const Conv2dBwdWeightPlan p = conv2d_bwd_weight_plan(N, Ci, Co, H, W);
    MPHIP_REQUIRE(p.kernel != 0,
                  "conv2d_bwd_weight: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d (Ci %% 16 == 0, Co %% 32 == 0, N, H, W >= 1, fewer than 2^31 "
                  "elements per tensor)", N, Ci, Co, H, W);
    const size_t need = mphip_conv2d_bwd_weight_workspace_bytes(N, Ci, Co, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("conv2d_bwd_weight: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    MPHIP_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw | (uintptr_t)dy_scale | (uintptr_t)x_range | (uintptr_t)workspace) & 3) == 0,
                  "conv2d_bwd_weight: x, x_range, dy, dy_scale, dw and the workspace must be 4-byte aligned");
    MPHIP_REQUIRE(p.kernel != 1 || (((uintptr_t)x | (uintptr_t)dy) & 15) == 0,
                  "conv2d_bwd_weight: x and dy must be 16-byte aligned when W %% 8 == 0 (the kernel reads rows with 16-byte loads)");
    hipStream_t s = (hipStream_t)stream;
    float *slot = (float *)workspace;
    float *unscale = (float *)((char *)workspace + (size_t)MPHIP_RANGE_FLOATS * sizeof(float));
    float *slabs = (float *)((char *)workspace + B2_WS_HEAD);
    if (!x_range) {   // the library-computed descriptor of x, as in the forward
        conv2d_range_launch(x, (size_t)N * Ci * H * W, slot, s);
        x_range = slot;
    }
    const dim3 grid(p.bxy, 1, p.splits);
    if (p.kernel == 1)
        hipLaunchKernelGGL(conv2d_bwd_weight_f16x3_kernel<true>, grid, dim3(B2_NTHR), 0, s, x, dy, dy_scale, x_range, slabs, unscale, N, Ci, Co, H,
                           W, p.tiles_h, p.tiles_w, p.tps);
    else
        hipLaunchKernelGGL(conv2d_bwd_weight_f16x3_kernel<false>, grid, dim3(B2_NTHR), 0, s, x, dy, dy_scale, x_range, slabs, unscale, N, Ci, Co, H,
                           W, p.tiles_h, p.tiles_w, p.tps);
    const size_t ncc = (size_t)Co * Ci;
    hipLaunchKernelGGL(conv2d_bwd_slab_reduce_kernel, dim3(cdiv(ncc, 64)), dim3(256), 0, s, (const float *)slabs, (const float *)unscale, dw, ncc,
                       p.splits);
    return check_launch("conv2d_bwd_weight");
}
