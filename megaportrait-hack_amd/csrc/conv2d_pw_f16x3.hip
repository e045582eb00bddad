// Conv2d 1x1 (pointwise) at stride 1 or 2 on the f16 matrix cores: the f16x3 arithmetic of conv2d_f16x3.hip on a tile of its own, for the
// three 1x1 convs of a torchvision-layout ResNet bottleneck (BatchNorm folded into weights and bias by the caller):
//     y[n,co,i,j] = act( sum_ci w[co,ci] * x[n,ci,s*i,s*j] + bias[co] (+ residual[n,co,i,j]) ),   Ho = (H+s-1)/s, Wo = (W+s-1)/s
//
// Arithmetic: conv2d_f16x3.hip's, term by term.  The operand scales are the pack header's and the range descriptor's powers of two, x is
// split v*S = hi + lo while it is staged, an accumulator (started at +0) takes Wlo*Xhi, Whi*Xhi, Whi*Xlo per 16-channel chunk in that
// order, chunks ascending, on v_mfma_f32_32x32x16_f16 with the 3x3 kernels' operand layout (A = weights, B = pixels, lane l holds channels
// 8*(l>>5)..+7 of the chunk); unscale, bias, residual and ReLU are fp32.  One output element therefore sees the MFMA sequence and operands
// that the 3x3 kernel's element sees from its centre tap: with a 3x3 weight that is zero but for w3[:,:,1,1] = w (the same max|w|, so the
// same pack scale) and the same x, descriptor and bias, this launch writes the bits of mphip_conv2d_fwd (stride 2: of
// mphip_conv2d_s2_fwd), the other taps adding +-0 to an accumulator that is never -0 (tests/test_gpu_conv2d_pw.py).
//
// Tile: per image the conv is Y[Co, Ho*Wo] = W[Co, Ci] * X[Ci, .], and the pixel axis of y is flat at either stride.  A workgroup of 4
// waves computes 64 output channels x 256 consecutive output pixels of one image; a wave owns all 64 channels of 64 pixels = 2 x 2 MFMA
// tiles (64 accumulator registers): a chunk costs 8 fragment reads for 12 MFMAs.  Per 16-channel chunk the workgroup stages
//   the 256 pixels, split while staging:   [part][kg][pixel][8] f16 = 16384 B
//   the chunk's packed weight slab:        [part][kg][co][8] f16    =  4096 B
// = 20480 B of LDS, single buffered; the next chunk's global loads are issued before this chunk's MFMAs and written to LDS after them.
// Fragment reads are 16-byte and conflict-free (lane j of a half-wave reads pixel j: 512 contiguous bytes, each 16-lane service group of
// ds_read_b128 covers every bank once).
//
// Staging, two instantiations with equal bits:
//   VEC   stride 1, H*W % 4 == 0 and x 16-byte aligned: a thread loads two float4 (channels 2p and 2p+1 of four consecutive pixels) per k
//         group.  Its four b32 writes per part go out rotated by (lane >> 4) & 3, so that the 64 lanes of a write hit 64 banks.
//   else  4-byte loads of (channel pair, pixel) items like the 3x3 kernels'; at stride 2 the sub-sample is the load address
//         (2i * W + 2j): no sub-sampled copy exists.  An unaligned or H*W % 4 != 0 stride-1 map takes this path too.
// A ragged last pixel tile is a mask on loads (clamped address, zero staged) and stores; a channel tile past Co is zeros in the pack and
// a mask on the stores.  Stores (and the residual's loads) are 4 bytes per lane: the accumulator layout gives a lane ONE pixel column, and
// the 32 lanes of a half-wave write the 32 consecutive pixels of a channel, one whole 128-byte line per instruction at either alignment.
//
// Grid: one dimension, channel tile fastest: the Co/64 workgroups that read the same 256 pixels of x are neighbours in launch order, so x
// comes from HBM once and from L2 for the rest.
#include "conv2d_f16x3_tile.h"   // C2_KC, C2_COT, C2_NTHR, c2_cots, the helper launches

namespace mphip {

__device__ unsigned long long g_conv2d_pw_saturated;

constexpr int PW_PIX = C2PW_PIX;                      // output pixels per workgroup
constexpr int PW_SLAB_HALFS = 2 * 2 * C2_COT * 8;     // [part][kg][co][8] = 2048 halfs = 4096 B per (co tile, chunk)
constexpr int PW_X_PART = 2 * PW_PIX * 8;             // halfs per part (hi or lo): [kg][pixel][8]

static inline int pw_out(int e, int stride) { return (e + stride - 1) / stride; }

bool c2_pw_supported(int N, int Ci, int Co, int H, int W, int stride) {
    if (stride != 1 && stride != 2) return false;
    if (N < 1 || Ci < C2_KC || Co < 32 || H < 1 || W < 1 || Ci % C2_KC || Co % 32) return false;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return false;
    const unsigned long long howo = (unsigned long long)pw_out(H, stride) * (unsigned long long)pw_out(W, stride);
    if ((unsigned long long)N * Ci * hw >= (1ull << 31) || (unsigned long long)N * Co * howo >= (1ull << 31)) return false;
    return c2_cots(Co) <= 65535;
}

// ---- weight packing: the header of mphip_pack_conv2d_weight (same function of max|w|), then the slabs ------------------------------
__global__ void __launch_bounds__(256) conv2d_pw_absmax_kernel(const float *__restrict__ w, size_t n, unsigned *__restrict__ hdr) {
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
    unsigned b = wave_umax(__float_as_uint(m));   // (non-negative floats order like their bits)
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        b = max(max(red[0], red[1]), max(red[2], red[3]));
        if (b) atomicMax(hdr + 2, b);
    }
}

// one thread = one 16-byte fragment (8 consecutive ci of one co), hi and lo; output channels past Co are zeros
__global__ void __launch_bounds__(256)
conv2d_pw_pack_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, const unsigned *__restrict__ hdr_in, float *__restrict__ hdr_out,
                      int Co, int Ci, int total) {
    const float scale = weight_scale(hdr_in[2]);
    const int nchunks = Ci / C2_KC;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        const int co = i % C2_COT;
        int r = i / C2_COT;
        const int kg = r % 2; r /= 2;
        const int chunk = r % nchunks;
        const int cot = r / nchunks;
        const int cog = cot * C2_COT + co;
        half8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = chunk * C2_KC + kg * 8 + e;
            const float v = cog < Co ? w[(size_t)cog * Ci + ci] : 0.0f;
            _Float16 h, l;
            split_f16(v * scale, h, l);
            hi[e] = h; lo[e] = l;
        }
        const size_t slab = (size_t)cot * nchunks + chunk;
        const size_t inner = ((size_t)kg * C2_COT + co) * 8;
        *reinterpret_cast<half8 *>(out + slab * PW_SLAB_HALFS + inner) = hi;
        *reinterpret_cast<half8 *>(out + slab * PW_SLAB_HALFS + PW_SLAB_HALFS / 2 + inner) = lo;
    }
    if (i == 0) {
        hdr_out[0] = 1.0f / scale;
        hdr_out[1] = scale;
    }
}

// ---- the conv kernel ----------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(3)))
conv2d_pw_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                       const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                       float *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int stride, int relu, int ptiles,
                       int cots, unsigned nslots) {
    __shared__ __attribute__((aligned(16))) _Float16 smem[PW_SLAB_HALFS + 2 * PW_X_PART];
    __shared__ unsigned red[4];
    _Float16 *const Ws = smem;                   // [part][kg][co][8]
    _Float16 *const Xs = smem + PW_SLAB_HALFS;   // [part][kg][pixel][8]

    float x_scale, x_unscale;
    range_scale_block(x_range, x_scale, x_unscale);   // (folds the producer's partial maxima; barriers inside)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kg = lane >> 5;
    unsigned bid = blockIdx.x;
    const int cot = bid % (unsigned)cots; bid /= (unsigned)cots;
    const int pt = bid % (unsigned)ptiles;
    const int n = bid / (unsigned)ptiles;
    const int Wo = VEC ? W : (W + stride - 1) / stride;
    const size_t HW = (size_t)H * W;
    const size_t HWo = VEC ? HW : (size_t)((H + stride - 1) / stride) * Wo;
    const unsigned HWu = (unsigned)HW;   // (a chunk's 16 channels hold fewer than 2^31 elements: 32-bit element offsets)
    const int p0 = pt * PW_PIX;          // first output pixel of the tile (flat index in the image)
    const int nchunks = Ci / C2_KC;
    const float *const xn = x + (size_t)n * Ci * HW;

    // X staging.  The thread's channel pair inside a k group is pp = tid & 3 in both forms, and its pixels do not depend on the chunk:
    //   VEC   the quad of pixels 4q .. 4q+3, q = tid >> 2; item i = k group i
    //   else  the pixels i * 64 + (tid >> 2), i = 0..3; item (i, k group)
    // Loads are unconditional from a clamped (always valid) address, the mask is applied when the values are written to LDS.
    const int pp = tid & 3, q = tid >> 2;
    unsigned off[VEC ? 1 : 4];   // element offset of the thread's pixel(s) inside a channel of x
    unsigned okm = 0;
    if constexpr (VEC) {
        const unsigned P = (unsigned)p0 + 4u * q;
        okm = P < HWu ? 1u : 0u;                 // (H*W % 4 == 0: a quad is whole or absent)
        off[0] = okm ? P : HWu - 4u;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned P = (unsigned)p0 + i * 64 + q;
            const bool ok = P < (unsigned)HWo;
            const unsigned Pc = ok ? P : (unsigned)HWo - 1u;
            off[i] = stride == 1 ? Pc : (Pc / (unsigned)Wo) * 2u * W + (Pc % (unsigned)Wo) * 2u;
            okm |= ok ? 1u << i : 0u;
        }
    }
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    f32x4 xa4[VEC ? 2 : 1], xb4[VEC ? 2 : 1];   // VEC: [k group]
    float xa[VEC ? 1 : 8], xb[VEC ? 1 : 8];     // else: [k group * 4 + i]
    u32x4 wq;
    unsigned sat = 0;
    static_assert(PW_SLAB_HALFS * 2 == 16 * C2_NTHR, "one 16-byte piece of the weight slab per thread");
#define PW_LOAD_CHUNK(c_)                                                                              \
    {                                                                                                  \
        const float *const xc_ = xn + (size_t)(c_) * C2_KC * HW;                                       \
        if constexpr (VEC) {                                                                           \
            _Pragma("unroll") for (int k_ = 0; k_ < 2; ++k_) {                                         \
                const unsigned o_ = (unsigned)(2 * (k_ * 4 + pp)) * HWu + off[0];                      \
                xa4[k_] = *reinterpret_cast<const f32x4 *>(xc_ + o_);                                  \
                xb4[k_] = *reinterpret_cast<const f32x4 *>(xc_ + o_ + HWu);                            \
            }                                                                                          \
        } else {                                                                                       \
            _Pragma("unroll") for (int k_ = 0; k_ < 2; ++k_)                                           \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                        \
                    const unsigned o_ = (unsigned)(2 * (k_ * 4 + pp)) * HWu + off[i];                  \
                    xa[k_ * 4 + i] = xc_[o_];                                                          \
                    xb[k_ * 4 + i] = xc_[o_ + HWu];                                                    \
                }                                                                                      \
        }                                                                                              \
        wq = reinterpret_cast<const u32x4 *>(wslabs + ((size_t)cot * nchunks + (c_)) * PW_SLAB_HALFS)[tid]; \
    }
    // one (channel pair, pixel) value pair -> scale, count, split, one b32 write of hi and one of lo
#define PW_STAGE(a_, b_, ok_, pix_, k_)                                                                \
    {                                                                                                  \
        const float v0_ = (ok_) ? (a_) * x_scale : 0.0f, v1_ = (ok_) ? (b_) * x_scale : 0.0f;          \
        sat += !(fabsf(v0_) <= F16_CLAMP) + !(fabsf(v1_) <= F16_CLAMP);   /* NaN counts */             \
        _Float16 hA_, lA_, hB_, lB_;                                                                   \
        split_f16(v0_, hA_, lA_);                                                                      \
        split_f16(v1_, hB_, lB_);                                                                      \
        const half2v hv_ = {hA_, hB_}, lv_ = {lA_, lB_};                                               \
        const int dst_ = ((k_) * PW_PIX + (pix_)) * 8 + pp * 2;                                        \
        *reinterpret_cast<half2v *>(Xs + dst_) = hv_;                                                  \
        *reinterpret_cast<half2v *>(Xs + PW_X_PART + dst_) = lv_;                                      \
    }
#define PW_WRITE_CHUNK()                                                                               \
    {                                                                                                  \
        if constexpr (VEC) {                                                                           \
            const int rot_ = (tid >> 4) & 3;                                                           \
            _Pragma("unroll") for (int k_ = 0; k_ < 2; ++k_)                                           \
                _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                     \
                    const int rr_ = (r_ + rot_) & 3;                                                   \
                    const float a_ = rr_ == 0 ? xa4[k_][0] : rr_ == 1 ? xa4[k_][1] : rr_ == 2 ? xa4[k_][2] : xa4[k_][3]; \
                    const float b_ = rr_ == 0 ? xb4[k_][0] : rr_ == 1 ? xb4[k_][1] : rr_ == 2 ? xb4[k_][2] : xb4[k_][3]; \
                    PW_STAGE(a_, b_, okm != 0, 4 * q + rr_, k_)                                        \
                }                                                                                      \
        } else {                                                                                       \
            _Pragma("unroll") for (int k_ = 0; k_ < 2; ++k_)                                           \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                          \
                    PW_STAGE(xa[k_ * 4 + i], xb[k_ * 4 + i], (okm >> i) & 1u, i * 64 + q, k_)          \
        }                                                                                              \
        reinterpret_cast<u32x4 *>(Ws)[tid] = wq;                                                       \
    }

    const int a_base = (kg * C2_COT + j) * 8;                  // + (part * 2 * 64 + m * 32) * 8
    const int b_base = (kg * PW_PIX + wave * 64 + j) * 8;      // + t * 32 * 8: this lane's pixel in column tile t is wave * 64 + t * 32 + j

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;

    PW_LOAD_CHUNK(0)
    PW_WRITE_CHUNK()
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        if (more) PW_LOAD_CHUNK(c + 1)   // in flight during this chunk's MFMAs
        half8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            ah[m] = *reinterpret_cast<const half8 *>(Ws + a_base + m * 32 * 8);
            al[m] = *reinterpret_cast<const half8 *>(Ws + PW_SLAB_HALFS / 2 + a_base + m * 32 * 8);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bh[t] = *reinterpret_cast<const half8 *>(Xs + b_base + t * 32 * 8);
            bl[t] = *reinterpret_cast<const half8 *>(Xs + PW_X_PART + b_base + t * 32 * 8);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[m], bh[t], acc[m][t], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bh[t], acc[m][t], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bl[t], acc[m][t], 0, 0, 0);
        if (more) {
            __syncthreads();   // every wave is past its fragment reads of this chunk
            PW_WRITE_CHUNK()
            __syncthreads();
        }
    }

#undef PW_LOAD_CHUNK
#undef PW_STAGE
#undef PW_WRITE_CHUNK

    // epilogue (the 3x3 kernels'): unscale (two powers of two, one after the other), bias, residual, ReLU in fp32; stores masked past the
    // image's last pixel and past Co
    const Unscale u = {whdr[0], x_unscale};
    unsigned ymax = 0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int co0 = cot * C2_COT + m * 32;
        if (co0 < Co) {   // (Co % 32 == 0: a row tile is whole or absent; workgroup-uniform)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned P = (unsigned)p0 + wave * 64 + t * 32 + j;
                if (P < (unsigned)HWo) {
                    const size_t o = ((size_t)n * Co + co0 + 4 * kg) * HWo + P;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = (reg & 3) + 8 * (reg >> 2);
                        const size_t oi = o + (size_t)row * HWo;
                        float v = unscaled(acc[m][t][reg], u, bias[co0 + 4 * kg + row]);
                        if (residual) v += residual[oi];
                        if (relu) v = v < 0.0f ? 0.0f : v;   // (keeps NaN, like torch's relu)
                        y[oi] = v;
                        ymax = max(ymax, range_bits(v));
                    }
                }
            }
        }
    }
    if (out_range) {   // workgroup-uniform
        ymax = wave_umax(ymax);
        if (lane == 0) red[wave] = ymax;
        __syncthreads();
        if (tid == 0) {
            const unsigned mx = max(max(red[0], red[1]), max(red[2], red[3]));
            const unsigned slot = blockIdx.x % nslots;
            if (mx) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + slot, mx);
        }
    }
    if (__builtin_amdgcn_ballot_w64(sat != 0) != 0) {  // never taken in normal operation
        unsigned tot = sat;
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) tot += __shfl_xor(tot, sft, 64);
        if (lane == 0) atomicAdd(&g_conv2d_pw_saturated, (unsigned long long)tot);
    }
}

void conv2d_pw_launch(const C2Call &c, const C2Grid &g) {
    // g.tiles_w: 256-pixel tiles per image (the form is flat: tiles_h == 1); g.grid = (N * tiles_w, channel tiles)
    const unsigned blocks = g.grid.x * g.grid.y;   // (fewer than the elements of y: below 2^31)
    const bool vec = c.stride == 1 && ((size_t)c.H * c.W) % 4 == 0 && ((uintptr_t)c.x1 & 15) == 0;
    auto kern = vec ? conv2d_pw_f16x3_kernel<true> : conv2d_pw_f16x3_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range,
                       (const _Float16 *)((const char *)c.w_packed + 16), (const float *)c.w_packed, c.bias, (const float *)c.residual,
                       (float *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.stride, c.relu, g.tiles_w, (int)g.grid.y, g.nslots);
}

int conv2d_pw_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_pw_saturated, count, reset); }

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_pw_supported(int N, int Ci, int Co, int H, int W, int stride) {
    return c2_pw_supported(N, Ci, Co, H, W, stride) ? 1 : 0;
}

extern "C" size_t mphip_conv2d_pw_packed_weight_bytes(int Co, int Ci) {
    if (Ci < C2_KC || Co < 32 || Ci % C2_KC || Co % 32) return 0;
    return 16 + (size_t)c2_cots(Co) * (Ci / C2_KC) * PW_SLAB_HALFS * 2;
}

extern "C" int mphip_pack_conv2d_pw_weight(const float *w, void *w_packed, int Co, int Ci, void *stream) {
    MPHIP_REQUIRE(w && w_packed, "pack_conv2d_pw_weight: null pointer");
    MPHIP_REQUIRE(Ci >= C2_KC && Co >= 32 && Ci % C2_KC == 0 && Co % 32 == 0 && c2_cots(Co) <= 65535,
                  "pack_conv2d_pw_weight: Co = %d, Ci = %d: Ci must be a multiple of 16 and Co a multiple of 32", Co, Ci);
    MPHIP_REQUIRE(((uintptr_t)w_packed & 15) == 0, "pack_conv2d_pw_weight: w_packed must be 16-byte aligned");
    const long long total = (long long)c2_cots(Co) * (Ci / C2_KC) * 2 * C2_COT;
    MPHIP_REQUIRE(total < (1ll << 31) - 256, "pack_conv2d_pw_weight: Co = %d, Ci = %d is too large", Co, Ci);
    hipStream_t s = (hipStream_t)stream;
    zero_fill(w_packed, 16, s);   // header: the absmax kernel accumulates with atomicMax
    const size_t n = (size_t)Co * Ci;
    hipLaunchKernelGGL(conv2d_pw_absmax_kernel, dim3((unsigned)std::min<size_t>(1024, (n + 2047) / 2048)), dim3(256), 0, s, w, n,
                       (unsigned *)w_packed);
    hipLaunchKernelGGL(conv2d_pw_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, (_Float16 *)((char *)w_packed + 16),
                       (const unsigned *)w_packed, (float *)w_packed, Co, Ci, (int)total);
    return check_launch("pack_conv2d_pw_weight");
}

extern "C" size_t mphip_conv2d_pw_workspace_bytes(int N, int Ci, int Co, int H, int W, int stride) {
    return c2_pw_supported(N, Ci, Co, H, W, stride) ? c2_workspace_bytes(1) : 0;   // the library-computed descriptor of x (x_range == NULL)
}

extern "C" int mphip_conv2d_pw_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, const float *residual,
                                   float *y, float *out_range, int N, int Ci, int Co, int H, int W, int stride, int relu, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    C2Call c = c2_call_f32("conv2d_pw_fwd", C2_PW, x, x_range, w_packed, bias, residual, y, out_range, N, Ci, Co, H, W, relu, workspace,
                           workspace_bytes, stream);
    c.stride = stride;
    return conv2d_run(c);
}
