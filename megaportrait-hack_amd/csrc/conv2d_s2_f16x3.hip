// Conv2d 3x3 at stride 2 (padding 1) on the f16 matrix cores: the f16x3 arithmetic of conv2d_f16x3.hip on a tile of its own, for the first
// conv of a down-sampling BasicBlock of Emtn's ResNet-18s (BatchNorm folded into weights and bias by the caller):
//     y[n,co,i,j] = act( sum w[co,ci,dy,dx] * x[n,ci,2i+dy-1,2j+dx-1] + bias[co] (+ residual[n,co,i,j]) ),   Ho = (H+1)/2, Wo = (W+1)/2
//
// Arithmetic: conv2d_f16x3.hip's, term by term.  The operand scales are the pack header's and the range descriptor's powers of two, x is
// split v*S = hi + lo while it is staged, an accumulator takes Wlo*Xhi, Whi*Xhi, Whi*Xlo per tap in that order, chunk-major over taps
// 0..8, on v_mfma_f32_32x32x16_f16; unscale, bias, residual and ReLU are fp32.  One output element therefore sees the MFMA sequence and
// operands of the stride-1 kernel's element (2i, 2j): with the same x, descriptor, pack and bias this launch writes the bits of
// mphip_conv2d_fwd's output at the even rows and columns (tests/test_gpu_conv2d_s2.py).  The pack is the ordinary one.
//
// Tile: a workgroup of 4 waves computes 64 output channels x (8 rows x 16 columns); a wave owns all 64 channels of 2 rows = 2 x 1 MFMA
// tiles (32 accumulator registers): one tap costs 6 fragment reads for 6 MFMAs.  Per 16-channel chunk the workgroup stages
//   the 17 x 33 input halo as four parity planes (row parity x column parity) of 9 x 17 pixels:
//                                                    [part][kg][plane][pixel][8] f16 = 39168 B   (zero padding lives in the masked loads)
//   the chunk's packed 9-tap weight slab:            [part][tap][kg][co][8] f16 = 36864 B
// = 76032 B of LDS, single buffered: two workgroups share a CU.  Tap (dy, dx) of output pixel (i, j) is halo pixel (2i+dy, 2j+dx) = plane
// (dy&1, dx&1), position (i + (dy>>1), j + (dx>>1)): inside a plane the 16 pixels of an output row are contiguous, so a 16-lane
// ds_read_b128 group reads 256 contiguous bytes exactly as in the stride-1 kernel (same lane -> pixel slot permutation).  Positions a
// plane does not have (row 8 of the odd-row planes, column 16 of the odd-column planes) are neither written nor read.
#include "conv2d_f16x3_tile.h"   // C2_KC, C2_COT, C2_SLAB_HALFS, c2_cots: the pack's constants

namespace mphip {

__device__ unsigned long long g_conv2d_s2_saturated;

constexpr int S2_HH = 2 * C2S2_TH + 1, S2_HW = 2 * C2S2_TW + 1;   // 17 x 33 input halo
constexpr int S2_XV = S2_HH * S2_HW;                              // 561 halo pixels
constexpr int S2_PW = C2S2_TW + 1;                                // 17: a plane's row length
constexpr int S2_PV = (C2S2_TH + 1) * S2_PW;                      // 153 pixels per plane
constexpr int S2_KGV = 4 * S2_PV;                                 // 612 pixels per k group
constexpr int S2_X_PART = 2 * S2_KGV * 8;                         // halfs per part (hi or lo): [kg][plane][pixel][8]

bool c2_s2_supported(int N, int Ci, int Co, int H, int W) {
    if (N < 1 || Ci < C2_KC || Co < 32 || H < 1 || W < 1 || Ci % C2_KC || Co % 32) return false;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return false;
    const unsigned long long howo = (unsigned long long)((H + 1) / 2) * (unsigned long long)((W + 1) / 2);
    if ((unsigned long long)N * Ci * hw >= (1ull << 31) || (unsigned long long)N * Co * howo >= (1ull << 31)) return false;
    return c2_cots(Co) <= 65535;
}

__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3s2_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                         const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                         float *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int relu, int tiles_w,
                         int tiles_h, unsigned nslots) {
    __shared__ __attribute__((aligned(16))) _Float16 smem[C2_SLAB_HALFS + 2 * S2_X_PART];
    __shared__ unsigned red[4];
    _Float16 *const Ws = smem;                   // [part][tap][kg][co][8]
    _Float16 *const Xs = smem + C2_SLAB_HALFS;   // [part][kg][plane][pixel][8]

    float x_scale, x_unscale;
    range_scale_block(x_range, x_scale, x_unscale);   // (folds the producer's partial maxima; barriers inside)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kg = lane >> 5;
    int bid = blockIdx.x;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h;
    const int n = bid / tiles_h;
    const int cot = blockIdx.y;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int h0 = th * C2S2_TH, w0 = tw * C2S2_TW;   // of the output tile; its halo starts at input (2 h0 - 1, 2 w0 - 1)
    const int nchunks = Ci / C2_KC;
    const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;
    const unsigned HWu = (unsigned)HW;   // (a chunk's 16 channels hold fewer than 2^31 elements: 32-bit element offsets)
    const float *const xn = x + (size_t)n * Ci * HW;

    // X staging: an item is (channel pair p, halo pixel r), as in the stride-1 kernel; the halo pixel's parity picks its plane
    constexpr int NX = 8 * S2_XV;                        // items per chunk
    constexpr int XI = (NX + C2_NTHR - 1) / C2_NTHR;     // 18 per thread
    constexpr int WI = C2_SLAB_HALFS * 2 / 16 / C2_NTHR; // 9 16-byte pieces of the slab per thread
    static_assert(C2_SLAB_HALFS * 2 % (16 * C2_NTHR) == 0, "weight slab / thread count");
    static_assert(XI <= 32, "one mask bit per item");
    float xa[XI], xb[XI];
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 wq[WI];
    unsigned sat = 0, okm = 0;
#define S2_LOAD_CHUNK(c_)                                                                              \
    {                                                                                                  \
        const float *const xc_ = xn + (size_t)(c_) * C2_KC * HW;                                       \
        int tid_ = tid;                                                                                \
        asm volatile("" : "+v"(tid_)); /* opaque: keeps the per-item offsets out of registers across the K loop */ \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                               \
            const int e_ = i * C2_NTHR + tid_, ec_ = min(e_, NX - 1);                                  \
            const int rest_ = ec_ >> 2;                                                                \
            const int p_ = (rest_ / S2_XV) * 4 + (ec_ & 3), r_ = rest_ % S2_XV;                        \
            const int gh_ = 2 * h0 - 1 + r_ / S2_HW, gw_ = 2 * w0 - 1 + r_ % S2_HW;                    \
            const bool ok_ = e_ < NX && (unsigned)gh_ < (unsigned)H && (unsigned)gw_ < (unsigned)W;    \
            /* unconditional loads from a clamped (always valid) address, a select later: no branch per load */ \
            const unsigned off_ = (unsigned)(2 * p_) * HWu + (unsigned)min(max(gh_, 0), H - 1) * W + min(max(gw_, 0), W - 1); \
            xa[i] = xc_[off_];                                                                         \
            xb[i] = xc_[off_ + HWu];                                                                   \
            okm = ok_ ? okm | (1u << i) : okm & ~(1u << i);                                            \
        }                                                                                              \
        const u32x4 *const ws_ = reinterpret_cast<const u32x4 *>(wslabs + ((size_t)cot * nchunks + (c_)) * C2_SLAB_HALFS); \
        _Pragma("unroll") for (int i = 0; i < WI; ++i) wq[i] = ws_[i * C2_NTHR + tid_];               \
    }
#define S2_WRITE_CHUNK()                                                                               \
    {                                                                                                  \
        int tid_ = tid;                                                                                \
        asm volatile("" : "+v"(tid_));                                                                 \
        _Pragma("unroll") for (int i = 0; i < XI; ++i) {                                               \
            const int e_ = i * C2_NTHR + tid_;                                                         \
            if (e_ < NX) {                                                                             \
                const int rest_ = e_ >> 2;                                                             \
                const int kgi_ = rest_ / S2_XV, r_ = rest_ % S2_XV;                                    \
                const int hr_ = r_ / S2_HW, hc_ = r_ % S2_HW;                                          \
                const int pix_ = kgi_ * S2_KGV + ((hr_ & 1) * 2 + (hc_ & 1)) * S2_PV + (hr_ >> 1) * S2_PW + (hc_ >> 1); \
                const int dst_ = pix_ * 8 + (e_ & 3) * 2;                                              \
                const bool ok_ = (okm >> i) & 1u;                                                      \
                const float v0_ = ok_ ? xa[i] * x_scale : 0.0f, v1_ = ok_ ? xb[i] * x_scale : 0.0f;    \
                sat += !(fabsf(v0_) <= F16_CLAMP) + !(fabsf(v1_) <= F16_CLAMP);   /* NaN counts */     \
                _Float16 hA_, lA_, hB_, lB_;                                                           \
                split_f16(v0_, hA_, lA_);                                                              \
                split_f16(v1_, hB_, lB_);                                                              \
                const half2v hv_ = {hA_, hB_}, lv_ = {lA_, lB_};                                       \
                *reinterpret_cast<half2v *>(Xs + dst_) = hv_;                                          \
                *reinterpret_cast<half2v *>(Xs + S2_X_PART + dst_) = lv_;                              \
            }                                                                                          \
        }                                                                                              \
        _Pragma("unroll") for (int i = 0; i < WI; ++i) reinterpret_cast<u32x4 *>(Ws)[i * C2_NTHR + tid_] = wq[i]; \
    }

    // the stride-1 kernel's slot permutation: each 16-lane ds_read_b128 group reads one whole 16-pixel row of a plane
    const int jg = ((j >> 2) & 1) ^ ((j >> 3) & 1) ^ ((j >> 4) & 1);
    const int jpos = j < 4 ? j : j < 12 ? j - 4 : j < 20 ? j - 8 : j < 28 ? j - 12 : j - 16;
    const int jv = jg * 16 + jpos;
    const int prow = wave * 2 + (jv >> 4), pcol = jv & 15;       // this lane's output pixel in the tile
    const int a_base = (kg * C2_COT + j) * 8;                    // + ((part*9 + tap)*2*64 + m*32)*8
    const int b_base = (kg * S2_KGV + prow * S2_PW + pcol) * 8;  // + the tap's plane and offset

    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;

    S2_LOAD_CHUNK(0)
    S2_WRITE_CHUNK()
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        if (more) S2_LOAD_CHUNK(c + 1)   // in flight during this chunk's MFMAs
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            const int toff = (((dy & 1) * 2 + (dx & 1)) * S2_PV + (dy >> 1) * S2_PW + (dx >> 1)) * 8;
            half8 ah[2], al[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                ah[m] = *reinterpret_cast<const half8 *>(Ws + a_base + (tap * 2 * C2_COT + m * 32) * 8);
                al[m] = *reinterpret_cast<const half8 *>(Ws + C2_SLAB_HALFS / 2 + a_base + (tap * 2 * C2_COT + m * 32) * 8);
            }
            const half8 bh = *reinterpret_cast<const half8 *>(Xs + b_base + toff);
            const half8 bl = *reinterpret_cast<const half8 *>(Xs + S2_X_PART + b_base + toff);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[m], bh, acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bh, acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bl, acc[m], 0, 0, 0);
        }
        if (more) {
            __syncthreads();   // every wave is past its last fragment read of this chunk
            S2_WRITE_CHUNK()
            __syncthreads();
        }
    }

#undef S2_LOAD_CHUNK
#undef S2_WRITE_CHUNK

    // epilogue (the stride-1 kernel's): unscale (two powers of two, one after the other), bias, residual, ReLU in fp32; stores masked at the
    // ragged edge and past Co
    const Unscale u = {whdr[0], x_unscale};
    unsigned ymax = 0;
    const int gh = h0 + prow, gw = w0 + pcol;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int co0 = cot * C2_COT + m * 32;
        if (co0 < Co && gh < Ho && gw < Wo) {   // (Co % 32 == 0: a row tile is whole or absent)
            const size_t o = ((size_t)n * Co + co0 + 4 * kg) * HWo + (size_t)gh * Wo + gw;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = (reg & 3) + 8 * (reg >> 2);
                const size_t oi = o + (size_t)row * HWo;
                float v = unscaled(acc[m][reg], u, bias[co0 + 4 * kg + row]);
                if (residual) v += residual[oi];
                if (relu) v = v < 0.0f ? 0.0f : v;   // (keeps NaN, like torch's relu)
                y[oi] = v;
                ymax = max(ymax, range_bits(v));
            }
        }
    }
    if (out_range) {   // workgroup-uniform
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
        if (lane == 0) atomicAdd(&g_conv2d_s2_saturated, (unsigned long long)tot);
    }
}

void conv2d_s2_launch(const C2Call &c, const C2Grid &g) {
    hipLaunchKernelGGL(conv2d_k3s2_f16x3_kernel, g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range,
                       (const _Float16 *)((const char *)c.w_packed + 16), (const float *)c.w_packed, c.bias, (const float *)c.residual,
                       (float *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.relu, g.tiles_w, g.tiles_h, g.nslots);
}

int conv2d_s2_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_s2_saturated, count, reset); }

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_s2_supported(int N, int Ci, int Co, int H, int W) { return c2_s2_supported(N, Ci, Co, H, W) ? 1 : 0; }

extern "C" size_t mphip_conv2d_s2_workspace_bytes(int N, int Ci, int Co, int H, int W) {
    return c2_s2_supported(N, Ci, Co, H, W) ? c2_workspace_bytes(1) : 0;   // the library-computed descriptor of x (x_range == NULL)
}

extern "C" int mphip_conv2d_s2_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, const float *residual,
                                   float *y, float *out_range, int N, int Ci, int Co, int H, int W, int relu, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return conv2d_run(c2_call_f32("conv2d_s2_fwd", C2_S2, x, x_range, w_packed, bias, residual, y, out_range, N, Ci, Co, H, W, relu, workspace,
                                  workspace_bytes, stream));
}
