// K12 — the ResNet-18 stem of Emtn's two nets: Conv2d(3, Co, 3, padding=1) (+ folded BatchNorm) -> ReLU -> MaxPool2d(3, 2, 1) in ONE launch.
//     c[n,co,r,s] = sum_{ci,dy,dx} w[co,ci,dy,dx] * x[n,ci,r+dy-1,s+dx-1]          zero padding 1, Ci = 3
//     v           = c + bias[co];   relu: v = ReLU(v)
//     pool == 0 : y[n,co,r,s] = v
//     pool != 0 : y[n,co,i,j] = max of v over the positions (2i+a-1, 2j+b-1), a, b in {0,1,2}, inside the map;  Ho = (H+1)/2, Wo = (W+1)/2
// Exact fp32 with a contract that leaves no freedom (include/mphip.h): acc = +0, fmaf(w, x, acc) over ci, dy, dx in that nesting, one
// rounded + bias; padded taps are multiplied by a staged 0; ReLU maps negative values and zeros to +0; NaN wins the ReLU and the max.
//
// Schedule.  No LDS tile: Ci = 3 makes the whole input window of a thread small enough for registers, and the 27 weights of an output
// channel are wave-uniform (scalar loads, one SGPR operand per FMA).  A thread owns two conv columns (2j, 2j+1) and
//   pool: the five conv rows 2i-1 .. 2i+3 of two pooled rows i, i+1: 7 x 4 x 3 = 84 input registers, loaded once, then the loop over Co;
//   flat: four conv rows: 6 x 4 x 3 = 72 input registers.
// The pooled window of column j is the conv columns 2j-1, 2j, 2j+1: 2j-1 is the left neighbour LANE's second column and arrives by one
// cross-lane move per conv row (no LDS, no barrier).  Lane 0 of a wave has no such neighbour: it computes pooled column j0 - 1 only to feed
// lane 1 and stores nothing, so a wave covers 63 pooled columns (2 pooled rows) and a conv value is computed 5/4 * 64/63 = 1.27 times.
// max commutes with the order, so neither the tiling nor that recomputation shows in the result.  ReLU is applied after the max
// (ReLU(max v) == max ReLU(v) bit for bit, NaN included); conv positions outside the map enter the max as -inf and never as NaN.
// The sign of a zero maximum is unspecified without ReLU (a window holding -0 and +0: -0 arises only from a -0 bias or an underflow).
// A workgroup is four waves stacked along H; when a map has few tiles the output channels are split over workgroups (blockIdx.y).
// out_range: one partial maximum per workgroup folded into `nslots` slots with an integer atomicMax after an init launch, the way
// conv2d_f16x3_tile.h's epilogue does (exact, order-independent: bitwise reproducible).
#include "mphip_common.h"

namespace mphip {

constexpr int ST_CI = 3;
constexpr int ST_WAVES = 4;              // waves of a workgroup, stacked along H
constexpr int ST_POOL_COLS = 63;         // pooled columns a wave stores (lane 0 feeds lane 1)
constexpr int ST_POOL_ROWS = 2;          // pooled rows of a wave
constexpr int ST_FLAT_COLS = 128;        // conv columns of a wave without the pool
constexpr int ST_FLAT_ROWS = 4;          // conv rows of a wave without the pool
constexpr int ST_SPLIT_WGS = 1024;       // the channels are split over workgroups while the grid stays within this (4 per CU)

struct StemArgs {
    int Co, H, W, Ho, Wo, relu, tiles_w, tiles_h;
    int co_per_wg;   // output channels of one workgroup (blockIdx.y picks the group): few tiles are spread over more workgroups
    unsigned nslots;
};

__global__ void __launch_bounds__(256) stem_range_init_kernel(float *__restrict__ range, unsigned nslots) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    unsigned *r = reinterpret_cast<unsigned *>(range);
    if (i < 4) r[i] = i == 3 ? nslots : 0u;   // derive mode
    if (i < nslots) r[4 + i] = 0u;
}

__device__ __forceinline__ float stem_relu(float v) { return v <= 0.0f ? 0.0f : v; }   // (NaN stays; -0 and negatives become +0)

template <bool POOL>
__global__ void __launch_bounds__(256)
conv2d_stem_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ y,
                   float *__restrict__ out_range, const StemArgs p) {
    constexpr int NR = POOL ? 2 * ST_POOL_ROWS + 1 : ST_FLAT_ROWS;   // conv rows of a thread
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = p.H, W = p.W, Co = p.Co;
    unsigned t = blockIdx.x;
    const int tw = t % p.tiles_w;
    t /= p.tiles_w;
    const int th = t % p.tiles_h, n = t / p.tiles_h;
    // first conv row and first conv column of this thread
    const int pi0 = (th * ST_WAVES + wave) * ST_POOL_ROWS;            // (pool) first pooled row
    const int pj = tw * ST_POOL_COLS + lane - 1;                      // (pool) pooled column; -1 and lane 0: the feeder
    const int r0 = POOL ? 2 * pi0 - 1 : (th * ST_WAVES + wave) * ST_FLAT_ROWS;
    const int c0 = POOL ? 2 * pj : tw * ST_FLAT_COLS + 2 * lane;

    float xin[ST_CI][NR + 2][4];
    const size_t HW = (size_t)H * W;
    const float *xn = x + (size_t)n * ST_CI * HW;
#pragma unroll
    for (int ci = 0; ci < ST_CI; ++ci)
#pragma unroll
        for (int r = 0; r < NR + 2; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // (every load is issued, from an address clamped into the map, and the padding selected afterwards: a load under its
                // own branch would wait for the one before it)
                const int gy = r0 - 1 + r, gx = c0 - 1 + c;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
                const float v = xn[(size_t)ci * HW + (size_t)cy * W + cx];
                xin[ci][r][c] = in ? v : 0.0f;
            }
    bool rok[NR], cok[2];
#pragma unroll
    for (int r = 0; r < NR; ++r) rok[r] = r0 + r >= 0 && r0 + r < H;
#pragma unroll
    for (int c = 0; c < 2; ++c) cok[c] = c0 + c >= 0 && c0 + c < W;

    unsigned ymax = 0;
    const float ninf = -__builtin_inff();
    const int co_begin = blockIdx.y * p.co_per_wg;
    for (int co = co_begin; co < co_begin + p.co_per_wg; ++co) {
        const float *wc = w + (size_t)co * (ST_CI * 9);   // wave-uniform: scalar loads
        const float b = bias[co];
        float acc[NR][2];
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r][0] = acc[r][1] = 0.0f;
#pragma unroll
        for (int ci = 0; ci < ST_CI; ++ci)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float wv = wc[(ci * 3 + dy) * 3 + dx];
#pragma unroll
                    for (int r = 0; r < NR; ++r)
#pragma unroll
                        for (int c = 0; c < 2; ++c) acc[r][c] = fmaf(wv, xin[ci][r + dy][c + dx], acc[r][c]);
                }
        if constexpr (POOL) {
            float h[NR];
            bool nan[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float v0 = rok[r] && cok[0] ? acc[r][0] + b : ninf;
                const float v1 = rok[r] && cok[1] ? acc[r][1] + b : ninf;
                const float left = __shfl_up(v1, 1, 64);   // conv column 2j-1 (lane 0 gets its own value back: it stores nothing)
                h[r] = fmaxf(fmaxf(left, v0), v1);
                nan[r] = __builtin_isunordered(v0, v1) || left != left;
            }
#pragma unroll
            for (int q = 0; q < ST_POOL_ROWS; ++q) {
                float m = fmaxf(fmaxf(h[2 * q], h[2 * q + 1]), h[2 * q + 2]);
                if (p.relu) m = stem_relu(m);
                if (nan[2 * q] || nan[2 * q + 1] || nan[2 * q + 2]) m = __builtin_nanf("");
                const int i = pi0 + q;
                if (lane != 0 && i < p.Ho && pj < p.Wo) {
                    y[(((size_t)n * Co + co) * p.Ho + i) * p.Wo + pj] = m;
                    ymax = max(ymax, range_bits(m));
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    float v = acc[r][c] + b;
                    if (p.relu) v = stem_relu(v);
                    if (rok[r] && cok[c]) {
                        y[(((size_t)n * Co + co) * H + (r0 + r)) * W + (c0 + c)] = v;
                        ymax = max(ymax, range_bits(v));
                    }
                }
        }
    }
    if (out_range) {   // workgroup-uniform
        __shared__ unsigned red[ST_WAVES];
        ymax = wave_umax(ymax);
        if (lane == 0) red[wave] = ymax;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned mx = max(max(red[0], red[1]), max(red[2], red[3]));
            if (mx) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + (blockIdx.x + gridDim.x * blockIdx.y) % p.nslots, mx);
        }
    }
}

static bool stem_shape_ok(int N, int Ci, int Co, int H, int W, int pool) {
    if (Ci != ST_CI || Co < 16 || Co % 16 != 0 || N < 1 || H < 1 || W < 1) return false;
    const unsigned long long lim = 1ull << 31, hw = (unsigned long long)H * W;
    if (hw >= lim || (unsigned long long)N * ST_CI * hw >= lim) return false;
    const unsigned long long howo = pool ? (unsigned long long)((H + 1) / 2) * ((W + 1) / 2) : hw;
    return (unsigned long long)N * howo < lim && (unsigned long long)N * howo * Co < lim;
}

static bool stem_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_stem_supported(int N, int Ci, int Co, int H, int W, int pool) { return stem_shape_ok(N, Ci, Co, H, W, pool) ? 1 : 0; }

extern "C" int mphip_conv2d_stem_fwd(const float *x, const float *w_oihw, const float *bias, float *y, float *out_range, int N, int Ci, int Co,
                                     int H, int W, int relu, int pool, void *stream) {
    MPHIP_REQUIRE(x && w_oihw && bias && y, "conv2d_stem_fwd: null pointer");
    MPHIP_REQUIRE(stem_shape_ok(N, Ci, Co, H, W, pool),
                  "conv2d_stem_fwd: unsupported shape N=%d Ci=%d Co=%d H=%d W=%d pool=%d (Ci == 3, Co %% 16 == 0, N, H, W >= 1, fewer than 2^31 "
                  "elements per tensor)", N, Ci, Co, H, W, pool);
    MPHIP_REQUIRE((((uintptr_t)x | (uintptr_t)w_oihw | (uintptr_t)bias | (uintptr_t)y | (uintptr_t)out_range) & 3) == 0,
                  "conv2d_stem_fwd: x, w, bias, y and out_range must be 4-byte aligned");
    StemArgs p;
    p.Ho = pool ? (H + 1) / 2 : H, p.Wo = pool ? (W + 1) / 2 : W;
    const size_t nx = (size_t)N * ST_CI * H * W, ny = (size_t)N * Co * p.Ho * p.Wo;
    MPHIP_REQUIRE(!stem_overlap(y, ny * sizeof(float), x, nx * sizeof(float)),
                  "conv2d_stem_fwd: y must not alias x (a workgroup reads the halo of tiles other workgroups write)");
    p.Co = Co, p.H = H, p.W = W, p.relu = relu ? 1 : 0;
    p.tiles_w = pool ? cdiv(p.Wo, ST_POOL_COLS) : cdiv(W, ST_FLAT_COLS);
    p.tiles_h = pool ? cdiv(p.Ho, ST_WAVES * ST_POOL_ROWS) : cdiv(H, ST_WAVES * ST_FLAT_ROWS);
    const long long tiles = (long long)N * p.tiles_h * p.tiles_w;   // (<= N * H * W < 2^31: they fit grid.x)
    // a small map has few tiles (one 512 x 512 frame: 160 for 256 CUs): the channels are split over up to ST_SPLIT_WGS workgroups, in
    // groups of a multiple of 16 (a workgroup of another group loads the same input window; the result does not depend on the split)
    int groups = 1;
    for (int d = Co / 16; d >= 1; --d)
        if ((Co / 16) % d == 0 && tiles * d <= ST_SPLIT_WGS) {
            groups = d;
            break;
        }
    p.co_per_wg = Co / groups;
    const long long wgs = tiles * groups;
    p.nslots = (unsigned)(wgs < (long long)RANGE_MAX_PARTS ? wgs : (long long)RANGE_MAX_PARTS);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)groups);
    if (out_range) hipLaunchKernelGGL(stem_range_init_kernel, dim3(cdiv(p.nslots + 4, 256)), dim3(256), 0, s, out_range, p.nslots);
    if (pool) hipLaunchKernelGGL(conv2d_stem_kernel<true>, grid, dim3(256), 0, s, x, w_oihw, bias, y, out_range, p);
    else      hipLaunchKernelGGL(conv2d_stem_kernel<false>, grid, dim3(256), 0, s, x, w_oihw, bias, y, out_range, p);
    return check_launch("conv2d_stem_fwd");
}
