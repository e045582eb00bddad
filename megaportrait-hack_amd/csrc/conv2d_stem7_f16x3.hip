// Conv2d 7x7 from a 3-channel image at stride 1 or 2 on the f16 matrix cores, for Eapp's two stems: Conv2d(3, 64, 7, padding=3) with a bias, and
// Conv2d(3, 64, 7, stride=2, padding=3) -> folded BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) in ONE launch.
//     c[n,co,i,j] = sum_{ci,dy,dx} w[co,ci,dy,dx] * x[n,ci,s*i+dy-3,s*j+dx-3]        zero padding 3, Ci = 3, Ho = (H+s-1)/s, Wo = (W+s-1)/s
//     v           = c + bias[co];   relu: v = ReLU(v)
//     pool == 0 : y = v                                                              [N,Co,Ho,Wo]
//     pool != 0 : y[n,co,p,q] = max of v over (2p+a-1, 2q+b-1), a, b in {0,1,2}, inside the Ho x Wo map      [N,Co,(Ho+1)/2,(Wo+1)/2]
//
// Arithmetic: conv2d_f16x3.hip's, term by term.  The operand scales are the pack header's and the range descriptor's powers of two, x is split
// v*S = hi + lo while it is staged, an accumulator (started at +0) takes Wlo*Xhi, Whi*Xhi, Whi*Xlo per 16-wide K chunk in that order, chunks
// ascending, on v_mfma_f32_32x32x16_f16 (A = weights, B = pixels, lane l holds K slots 8*(l>>5)..+7 of the chunk); unscale, bias, ReLU and the
// max are fp32.  The pool follows conv2d_stem.hip: conv positions outside the map enter the max as -inf, NaN wins the ReLU and the max, ReLU
// maps negatives and zeros to +0.
//
// K slots.  K is ordered as rows r = ci * 7 + dy of 8 slots dx = 0..7; the weight of dx = 7 is zero.  21 rows and one all-zero row are 176
// slots = 11 chunks; chunk c holds rows 2c (k group 0) and 2c + 1 (k group 1).  The 8-value MFMA fragment of output column j in row (ci, dy) is
// then x[ci][s*i+dy-3][s*j-3 .. s*j+4], the same for all seven dy that touch that input row.  The mapping is the pack's: it does not depend
// on the pixel, the tile position, the stride or the pool flag, so a pixel's MFMA operands are a function of its 7x7 window alone.  That is
// why the stride-2 output is the even sub-sample of the stride-1 output bit for bit, and why a translated image gives translated bits.
//
// Tile.  A workgroup of 4 waves computes all (up to 64) output channels of a 16 x 16 tile of conv positions; a wave owns 4 rows x 16 columns
// = 2 MFMA column tiles of (2 rows x 16 columns), times 2 row tiles of 32 channels: 64 accumulator registers.  LDS holds
//   the whole pack:                 [chunk][part][kg][co 64][8] f16                                  = 45056 B
//   the fragments of the tile:      [part][ci][input row][16 columns][8] f16, S*15+7 rows per ci     = 33792 B (stride 1), 56832 B (stride 2)
//   one zero fragment per part (the B operand of the all-zero K row)                                 =    32 B
// all staged ONCE, before a single barrier; the K loop is 11 chunks x 12 MFMAs with 16-byte fragment reads at 16-byte aligned addresses and
// no barrier.  A fragment's slot 7 is staged as 0: no value outside the window is ever multiplied.  Staging: one thread per fragment,
// seven 4-byte loads from clamped (always valid) addresses, the padding selected afterwards.
//
// Pool.  The conv tile of a pooled workgroup starts at conv position (14 P - 1, 14 Q - 1): its 16 x 16 conv values cover the windows of 7 x 7
// pooled outputs (the last conv row and column are not used), so a conv value is computed (16/14)^2 = 1.31 times.  After the K loop the
// waves park v (biased, ReLU'd, -inf outside the map) in LDS, [co][16][16] fp32 = 65536 B over the dead pack and fragments, and every
// thread takes the max of 9 for its share of the 64 x 49 outputs.
//
// out_range: one partial maximum per workgroup folded into `nslots` slots by an integer atomicMax after an init launch, like every 2-D conv.
#include "conv2d_f16x3_tile.h"   // the helper launches (range scan, out_range init), mphip_f16x3.h

namespace mphip {

__device__ unsigned long long g_conv2d_stem7_saturated;

constexpr int S7_CI = 3, S7_K = 7;
constexpr int S7_ROWS = S7_CI * S7_K;                  // 21 K rows of 8 slots
constexpr int S7_CHUNKS = (S7_ROWS + 1) / 2;           // 11 chunks of 2 rows
constexpr int S7_COT = 64;                             // output channels of a workgroup (the pack is padded to it)
constexpr int S7_T = 16;                               // conv tile: 16 x 16 positions
constexpr int S7_PT = 7;                               // pooled tile: 7 x 7 outputs
constexpr int S7_NTHR = 256;
constexpr int S7_W_HALFS = S7_CHUNKS * 2 * 2 * S7_COT * 8;   // [chunk][part][kg][co][8] = 22528 halfs = 45056 B
constexpr int S7_W_PART = 2 * S7_COT * 8;                    // halfs per (chunk, part)
constexpr size_t S7_PACK_BYTES = 16 + (size_t)S7_W_HALFS * 2;
constexpr int S7_E_FLOATS = S7_COT * S7_T * S7_T;            // the pool's exchange buffer

constexpr int s7_xrows(int S) { return S * (S7_T - 1) + S7_K; }                  // input rows of a tile per channel
constexpr int s7_xfrags(int S) { return S7_CI * s7_xrows(S) * S7_T; }            // fragments per part (the zero fragment follows them)
constexpr int s7_lds_halfs(int S) { return S7_W_HALFS + 2 * (s7_xfrags(S) + 1) * 8; }
static_assert(s7_lds_halfs(1) * 2 >= S7_E_FLOATS * 4 && s7_lds_halfs(2) * 2 >= S7_E_FLOATS * 4, "the exchange buffer reuses the staged LDS");
static_assert(S7_W_HALFS * 2 % (16 * S7_NTHR) == 0, "whole 16-byte pieces of the pack per thread");

static inline int s7_out(int e, int stride) { return (e + stride - 1) / stride; }

static bool stem7_shape_ok(int N, int Ci, int Co, int H, int W, int stride, int pool) {
    if (stride != 1 && stride != 2) return false;
    if (Ci != S7_CI || Co < 16 || Co > S7_COT || Co % 16 != 0 || N < 1 || H < 1 || W < 1) return false;
    const unsigned long long lim = 1ull << 31, hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= lim || (unsigned long long)N * S7_CI * hw >= lim) return false;
    unsigned long long ho = (unsigned long long)s7_out(H, stride), wo = (unsigned long long)s7_out(W, stride);
    if (pool) ho = (ho + 1) / 2, wo = (wo + 1) / 2;
    return (unsigned long long)N * ho * wo < lim && (unsigned long long)N * ho * wo * Co < lim;
}

static bool stem7_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

// ---- weight packing: the header of mphip_pack_conv2d_weight (same function of max|w|), then the slabs ------------------------------
__global__ void __launch_bounds__(256) conv2d_stem7_absmax_kernel(const float *__restrict__ w, size_t n, unsigned *__restrict__ hdr) {
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

// one thread = one 16-byte fragment (K row r = 2 * chunk + kg of one co), hi and lo; row 21, slot 7 and the channels past Co are zeros
__global__ void __launch_bounds__(256)
conv2d_stem7_pack_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, const unsigned *__restrict__ hdr_in, float *__restrict__ hdr_out,
                         int Co) {
    const float scale = weight_scale(hdr_in[2]);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < S7_CHUNKS * 2 * S7_COT) {
        const int co = i % S7_COT;
        const int kg = (i / S7_COT) % 2;
        const int chunk = i / (2 * S7_COT);
        const int r = 2 * chunk + kg;
        half8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = co < Co && r < S7_ROWS && e < S7_K ? w[((size_t)co * S7_ROWS + r) * S7_K + e] : 0.0f;
            _Float16 h, l;
            split_f16(v * scale, h, l);
            hi[e] = h; lo[e] = l;
        }
        const int inner = (kg * S7_COT + co) * 8;
        *reinterpret_cast<half8 *>(out + (chunk * 2 + 0) * S7_W_PART + inner) = hi;
        *reinterpret_cast<half8 *>(out + (chunk * 2 + 1) * S7_W_PART + inner) = lo;
    }
    if (i == 0) {
        hdr_out[0] = 1.0f / scale;
        hdr_out[1] = scale;
    }
}

struct Stem7Args {
    int Co, H, W, Ho, Wo, Hy, Wy;   // Ho x Wo: the conv map; Hy x Wy: y's map (the pooled one with POOL)
    int relu, tiles_h, tiles_w;
    unsigned nslots;
};

__device__ __forceinline__ float stem7_relu(float v) { return v <= 0.0f ? 0.0f : v; }   // (NaN stays; -0 and negatives become +0)

// ---- the conv kernel ----------------------------------------------------------------------------------------------------------------
template <int S, bool POOL>
__global__ void __launch_bounds__(S7_NTHR)
conv2d_stem7_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wpack,
                          const float *__restrict__ whdr, const float *__restrict__ bias, float *__restrict__ y, float *__restrict__ out_range,
                          const Stem7Args p) {
    constexpr int XR = s7_xrows(S);          // input rows per channel
    constexpr int NFRAG = s7_xfrags(S);      // fragments per part
    constexpr int X_PART = (NFRAG + 1) * 8;  // halfs per part, the zero fragment last
    __shared__ __attribute__((aligned(16))) _Float16 smem[s7_lds_halfs(S)];
    __shared__ unsigned red[4];
    _Float16 *const Ws = smem;               // [chunk][part][kg][co][8]
    _Float16 *const Xs = smem + S7_W_HALFS;  // [part][ci][row][col][8], then the zero fragment

    float x_scale, x_unscale;
    range_scale_block(x_range, x_scale, x_unscale);   // (folds the producer's partial maxima; barriers inside)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kg = lane >> 5;
    const int H = p.H, W = p.W, Co = p.Co;
    unsigned bid = blockIdx.x;
    const int tw = bid % (unsigned)p.tiles_w; bid /= (unsigned)p.tiles_w;
    const int th = bid % (unsigned)p.tiles_h;
    const int n = bid / (unsigned)p.tiles_h;
    // first conv position of the tile (-1 with POOL: the row above / column left of the first pooled window)
    const int crow0 = POOL ? 2 * S7_PT * th - 1 : S7_T * th;
    const int ccol0 = POOL ? 2 * S7_PT * tw - 1 : S7_T * tw;
    const size_t HW = (size_t)H * W;
    const float *const xn = x + (size_t)n * S7_CI * HW;

    // the pack: 11 16-byte pieces per thread, copied as they are
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    {
        constexpr int WI = S7_W_HALFS * 2 / 16 / S7_NTHR;
        u32x4 wq[WI];
#pragma unroll
        for (int i = 0; i < WI; ++i) wq[i] = reinterpret_cast<const u32x4 *>(wpack)[i * S7_NTHR + tid];
#pragma unroll
        for (int i = 0; i < WI; ++i) reinterpret_cast<u32x4 *>(Ws)[i * S7_NTHR + tid] = wq[i];
    }
    // the fragments: fragment f = (ci * XR + row) * 16 + col holds x[ci][S*crow0 - 3 + row][S*(ccol0 + col) - 3 .. + 6] and a zero
    unsigned sat = 0;
    const int gy0 = S * crow0 - 3, gx0 = S * ccol0 - 3;
    for (int f = tid; f < NFRAG; f += S7_NTHR) {
        const int col = f % S7_T;
        const int rr = f / S7_T;
        const int ci = rr / XR, row = rr - ci * XR;
        const int gy = gy0 + row, gx = gx0 + S * col;
        const bool yin = gy >= 0 && gy < H;
        const float *const xr = xn + (size_t)ci * HW + (size_t)min(max(gy, 0), H - 1) * W;
        float v[S7_K];
#pragma unroll
        for (int e = 0; e < S7_K; ++e) v[e] = xr[min(max(gx + e, 0), W - 1)];
        half8 hi, lo;
#pragma unroll
        for (int e = 0; e < S7_K; ++e) {
            const float vs = yin && gx + e >= 0 && gx + e < W ? v[e] * x_scale : 0.0f;
            sat += !(fabsf(vs) <= F16_CLAMP);   // NaN counts
            _Float16 h, l;
            split_f16(vs, h, l);
            hi[e] = h; lo[e] = l;
        }
        hi[7] = (_Float16)0.0f; lo[7] = (_Float16)0.0f;
        *reinterpret_cast<half8 *>(Xs + f * 8) = hi;
        *reinterpret_cast<half8 *>(Xs + X_PART + f * 8) = lo;
    }
    if (tid < 2) {
        half8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.0f;
        *reinterpret_cast<half8 *>(Xs + tid * X_PART + NFRAG * 8) = z;
    }
    __syncthreads();

    // this lane's pixel in column tile t: tile row wave * 4 + t * 2 + (j >> 4), tile column j & 15
    const int lcol = j & 15;
    const int lrow0 = wave * 4 + (j >> 4);
    const int a_base = (kg * S7_COT + j) * 8;   // + ((chunk * 2 + part) * 2 * 64 + m * 32) * 8

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;

#pragma unroll
    for (int c = 0; c < S7_CHUNKS; ++c) {
        // K row of this lane's k group: r = 2c + kg -> (ci, dy); the all-zero row 21 reads the zero fragment
        const int r = 2 * c + kg;
        const int ci = r / S7_K, dy = r - ci * S7_K;
        half8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            ah[m] = *reinterpret_cast<const half8 *>(Ws + (c * 2 + 0) * S7_W_PART + a_base + m * 32 * 8);
            al[m] = *reinterpret_cast<const half8 *>(Ws + (c * 2 + 1) * S7_W_PART + a_base + m * 32 * 8);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int frag = r < S7_ROWS ? (ci * XR + S * (lrow0 + t * 2) + dy) * S7_T + lcol : NFRAG;
            bh[t] = *reinterpret_cast<const half8 *>(Xs + frag * 8);
            bl[t] = *reinterpret_cast<const half8 *>(Xs + X_PART + frag * 8);
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
    }

    // epilogue: unscale (two powers of two, one after the other), bias, ReLU in fp32
    const Unscale u = {whdr[0], x_unscale};
    unsigned ymax = 0;
    if constexpr (POOL) {
        float *const E = reinterpret_cast<float *>(smem);   // [co][16][16]
        __syncthreads();   // every wave is past its fragment reads
        const float ninf = -__builtin_inff();
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int lrow = lrow0 + t * 2;
                const bool in = crow0 + lrow >= 0 && crow0 + lrow < p.Ho && ccol0 + lcol >= 0 && ccol0 + lcol < p.Wo;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int co = m * 32 + 4 * kg + (reg & 3) + 8 * (reg >> 2);
                    float v = unscaled(acc[m][t][reg], u, bias[min(co, Co - 1)]);
                    if (p.relu) v = stem7_relu(v);
                    E[(co * S7_T + lrow) * S7_T + lcol] = in ? v : ninf;
                }
            }
        __syncthreads();
        const int pr0 = S7_PT * th, pc0 = S7_PT * tw;
        for (int o = tid; o < Co * S7_PT * S7_PT; o += S7_NTHR) {
            const int co = o / (S7_PT * S7_PT), pq = o - co * (S7_PT * S7_PT);
            const int pr = pq / S7_PT, pc = pq - pr * S7_PT;
            if (pr0 + pr < p.Hy && pc0 + pc < p.Wy) {
                const float *const e = E + (co * S7_T + 2 * pr) * S7_T + 2 * pc;
                float mx = ninf;
                bool nan = false;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        const float v = e[a * S7_T + b];
                        mx = fmaxf(mx, v);
                        nan |= v != v;
                    }
                if (nan) mx = __builtin_nanf("");
                y[(((size_t)n * Co + co) * p.Hy + pr0 + pr) * p.Wy + pc0 + pc] = mx;
                ymax = max(ymax, range_bits(mx));
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int gi = crow0 + lrow0 + t * 2, gj = ccol0 + lcol;
                if (gi < p.Ho && gj < p.Wo) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int co = m * 32 + 4 * kg + (reg & 3) + 8 * (reg >> 2);
                        if (co < Co) {
                            float v = unscaled(acc[m][t][reg], u, bias[co]);
                            if (p.relu) v = stem7_relu(v);
                            y[(((size_t)n * Co + co) * p.Ho + gi) * p.Wo + gj] = v;
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
            if (mx) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + blockIdx.x % p.nslots, mx);
        }
    }
    if (__builtin_amdgcn_ballot_w64(sat != 0) != 0) {  // never taken in normal operation
        unsigned tot = sat;
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) tot += __shfl_xor(tot, sft, 64);
        if (lane == 0) atomicAdd(&g_conv2d_stem7_saturated, (unsigned long long)tot);
    }
}

int conv2d_stem7_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_stem7_saturated, count, reset); }

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_stem7_supported(int N, int Ci, int Co, int H, int W, int stride, int pool) {
    return stem7_shape_ok(N, Ci, Co, H, W, stride, pool) ? 1 : 0;
}

extern "C" size_t mphip_conv2d_stem7_packed_weight_bytes(int Co) {
    return Co >= 16 && Co <= S7_COT && Co % 16 == 0 ? S7_PACK_BYTES : 0;
}

extern "C" int mphip_pack_conv2d_stem7_weight(const float *w_oihw, void *w_packed, int Co, void *stream) {
    MPHIP_REQUIRE(w_oihw && w_packed, "pack_conv2d_stem7_weight: null pointer");
    MPHIP_REQUIRE(Co >= 16 && Co <= S7_COT && Co % 16 == 0, "pack_conv2d_stem7_weight: Co = %d: a multiple of 16, at most %d", Co, S7_COT);
    MPHIP_REQUIRE(((uintptr_t)w_oihw & 3) == 0 && ((uintptr_t)w_packed & 15) == 0,
                  "pack_conv2d_stem7_weight: w must be 4-byte aligned, w_packed 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    zero_fill(w_packed, 16, s);   // header: the absmax kernel accumulates with atomicMax
    const size_t n = (size_t)Co * S7_ROWS * S7_K;
    hipLaunchKernelGGL(conv2d_stem7_absmax_kernel, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, s, w_oihw, n, (unsigned *)w_packed);
    hipLaunchKernelGGL(conv2d_stem7_pack_kernel, dim3(cdiv(S7_CHUNKS * 2 * S7_COT, 256)), dim3(256), 0, s, w_oihw,
                       (_Float16 *)((char *)w_packed + 16), (const unsigned *)w_packed, (float *)w_packed, Co);
    return check_launch("pack_conv2d_stem7_weight");
}

extern "C" size_t mphip_conv2d_stem7_workspace_bytes(int N, int Ci, int Co, int H, int W, int stride, int pool) {
    return stem7_shape_ok(N, Ci, Co, H, W, stride, pool) ? c2_workspace_bytes(1) : 0;   // the library-computed descriptor of x (x_range == NULL)
}

extern "C" int mphip_conv2d_stem7_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, float *y, float *out_range,
                                      int N, int Ci, int Co, int H, int W, int stride, int relu, int pool, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(x && w_packed && bias && y, "conv2d_stem7_fwd: null pointer");
    MPHIP_REQUIRE(stem7_shape_ok(N, Ci, Co, H, W, stride, pool),
                  "conv2d_stem7_fwd: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d stride=%d pool=%d (Ci == 3, Co %% 16 == 0, Co <= 64, N, H, W >= 1, "
                  "stride 1 or 2, fewer than 2^31 elements per tensor)", N, Ci, Co, H, W, stride, pool);
    MPHIP_REQUIRE(((uintptr_t)w_packed & 15) == 0 &&
                      (((uintptr_t)x | (uintptr_t)x_range | (uintptr_t)bias | (uintptr_t)y | (uintptr_t)out_range) & 3) == 0,
                  "conv2d_stem7_fwd: w_packed must be 16-byte aligned, x, x_range, bias, y and out_range 4-byte aligned");
    Stem7Args p;
    p.Ho = s7_out(H, stride), p.Wo = s7_out(W, stride);
    p.Hy = pool ? (p.Ho + 1) / 2 : p.Ho, p.Wy = pool ? (p.Wo + 1) / 2 : p.Wo;
    const size_t nx = (size_t)N * S7_CI * H * W, ny = (size_t)N * Co * p.Hy * p.Wy;
    MPHIP_REQUIRE(!stem7_overlap(y, ny * sizeof(float), x, nx * sizeof(float)),
                  "conv2d_stem7_fwd: y must not alias x (a workgroup reads the halo of tiles other workgroups write)");
    hipStream_t s = (hipStream_t)stream;
    if (!x_range) {   // the library's own descriptor of x: one pass over a 3-channel image
        const size_t need = c2_workspace_bytes(1);
        if (!workspace || workspace_bytes < need) {
            set_error("conv2d_stem7_fwd: workspace %zu bytes < required %zu", workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        MPHIP_REQUIRE(((uintptr_t)workspace & 3) == 0, "conv2d_stem7_fwd: the workspace must be 4-byte aligned");
        conv2d_range_launch(x, nx, (float *)workspace, s);
        x_range = (const float *)workspace;
    }
    p.Co = Co, p.H = H, p.W = W, p.relu = relu ? 1 : 0;
    p.tiles_h = pool ? cdiv(p.Hy, S7_PT) : cdiv(p.Ho, S7_T);
    p.tiles_w = pool ? cdiv(p.Wy, S7_PT) : cdiv(p.Wo, S7_T);
    const long long tiles = (long long)N * p.tiles_h * p.tiles_w;   // (<= the elements of one channel of y: below 2^31)
    p.nslots = (unsigned)std::min<long long>(tiles, (long long)RANGE_MAX_PARTS);
    if (out_range) conv2d_out_range_init_launch(out_range, p.nslots, s);
    auto kern = stride == 1 ? (pool ? conv2d_stem7_f16x3_kernel<1, true> : conv2d_stem7_f16x3_kernel<1, false>)
                            : (pool ? conv2d_stem7_f16x3_kernel<2, true> : conv2d_stem7_f16x3_kernel<2, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(S7_NTHR), 0, s, x, x_range, (const _Float16 *)((const char *)w_packed + 16),
                       (const float *)w_packed, bias, y, out_range, p);
    return check_launch("conv2d_stem7_fwd");
}
