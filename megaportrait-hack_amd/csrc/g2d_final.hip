// K11 — G2d's exit: GroupNorm(32, 64) -> ReLU -> Conv2d(64, 3, 3, padding=1) -> Sigmoid on [N, 64, H, W]  (model.py:747-752, 762).
// HBM-bound: the input is the largest activation of the generator (64 MiB per frame in fp32 at 512 x 512) and the result is 3 MiB.
//   forward : gf_stats_partial_kernel  one read of x   -> per-chunk pivoted (sum, sum of squares) in double (norm.hip's numerics)
//             gf_fwd_kernel            one read of x   -> the image.  Every workgroup folds the partial sums of its own frame in its prologue
//                                      (32 groups x <= 32 chunks), stages a = max((x - mean) * rstd * gamma + beta, 0) of its tile + halo into
//                                      LDS four channels at a time, and keeps 3 x 4 fp32 accumulators per thread.
//   backward: gf_bwd_kernel            recomputes a the same way, writes a and da = conv^T(dv) (dv = dy * y * (1 - y)) to scratch and one
//                                      partial (dW, db) per workgroup; gf_fold_kernel adds the partials in a fixed order; the ReLU mask and
//                                      the GroupNorm backward are mphip_groupnorm_bwd (act = ReLU) on (x, a, da).
// The conv's zero padding is applied in the ACTIVATED domain: a halo pixel outside the image is staged as 0, never as act(norm(0)).
// The 1 728 weights are read through uniform (scalar-cache) loads: their index depends on loop counters only.
#include "mphip_common.h"

namespace mphip {

constexpr int GF_C = 64, GF_G = 32, GF_CO = 3, GF_CPG = GF_C / GF_G;
constexpr int GF_TW = 64, GF_TH = 16;   // output pixels of one workgroup: 256 threads x (1 row x 4 columns)
constexpr int GF_CH = 4;                // channels staged per step
constexpr int GF_LH = GF_TH + 2;        // LDS rows: the tile and one halo row above and below
constexpr int GF_LW = 72;               // LDS row: [3] left halo, [4 .. 67] the tile (16-byte aligned), [68] right halo
constexpr int GF_CHUNK = 16384;         // elements of one statistics partial (norm.hip's GN_CHUNK)
constexpr int GF_NW = GF_CO * GF_C * 9; // 1728 weights
constexpr int GF_PART = GF_NW + 4;      // floats of one workgroup's (dW, db) partial (db at [1728 .. 1730])

template <int DT>
struct alignas(sizeof(dtype_t<DT>) * 4) vec4_of {
    dtype_t<DT> v[4];
};

__device__ __forceinline__ double gf_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ float gf_wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// ---- statistics, stage 1: per (frame, group) span of cnt contiguous elements -> per-chunk (sum, sum of squares) of x - K in double,
// K = the span's first element (norm.hip: the pivot keeps the variance of a group whose |mean| is large against its spread).  Every
// thread adds groups of four consecutive elements whether they arrive as one vector load or four scalar ones, so the sums do not
// depend on the alignment of x — a half tensor and its widened fp32 copy give the same bits.
template <int DT>
__global__ void __launch_bounds__(256)
gf_stats_partial_kernel(const dtype_t<DT> *__restrict__ x, double *__restrict__ partial, size_t cnt, int chunks, int vec) {
    const int grp = blockIdx.y, chunk = blockIdx.x;
    const dtype_t<DT> *p = x + (size_t)grp * cnt;
    const size_t begin = (size_t)chunk * GF_CHUNK;
    const size_t end = begin + GF_CHUNK < cnt ? begin + GF_CHUNK : cnt;
    const float k = widen(p[0]);
    float s = 0.0f, ss = 0.0f;
#pragma unroll 4
    for (size_t i = begin + (size_t)threadIdx.x * 4; i < end; i += 1024) {
        float v[4];
        if (vec && i + 4 <= end) {
            const vec4_of<DT> t = *reinterpret_cast<const vec4_of<DT> *>(p + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = widen(t.v[j]) - k;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = i + j < end ? widen(p[i + j]) - k : 0.0f;
        }
        s += (v[0] + v[1]) + (v[2] + v[3]);
        ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const double ds = gf_wave_sum((double)s), dss = gf_wave_sum((double)ss);
    __shared__ double red[8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[wave * 2] = ds;
        red[wave * 2 + 1] = dss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[((size_t)grp * chunks + chunk) * 2] = (red[0] + red[2]) + (red[4] + red[6]);
        partial[((size_t)grp * chunks + chunk) * 2 + 1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
}

// One channel's folded normalisation: a = max(fma((x - mean_hi) - mean_lo, scale, beta), 0), scale = rstd * gamma.
// mean_hi + mean_lo is the double mean split in two floats: x - mean_hi is exact for x near the mean, so an input with a large DC keeps
// the accuracy of its spread.  (The backward gets the saved fp32 mean: mean_lo = 0.)
__device__ __forceinline__ float gf_act(float x, const float4 t) { return fmaxf(fmaf((x - t.x) - t.y, t.z, t.w), 0.0f); }

// Stages a of channels [c0, c0 + GF_CH) of the tile at (ty0, tx0) plus its one-pixel halo; outside the image: 0 (the conv pads a, not x).
template <int DT>
__device__ __forceinline__ void gf_stage(const dtype_t<DT> *__restrict__ xn, int c0, int H, int W, int ty0, int tx0, bool vec,
                                         const float4 *__restrict__ tab, float (*__restrict__ s_a)[GF_LH][GF_LW]) {
    const size_t HW = (size_t)H * W;
    if (vec) {   // (W % 4 == 0: a group of four columns is inside the image or outside it)
#pragma unroll
        for (int it = threadIdx.x; it < GF_CH * GF_LH * (GF_TW / 4); it += 256) {
            const int q = it & 15, r = (it >> 4) % GF_LH, cc = it / (16 * GF_LH);
            const int gy = ty0 + r - 1, gx = tx0 + q * 4;
            float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gy >= 0 && gy < H && gx < W) {
                const vec4_of<DT> t = *reinterpret_cast<const vec4_of<DT> *>(xn + (size_t)(c0 + cc) * HW + (size_t)gy * W + gx);
                const float4 f = tab[c0 + cc];
                o = make_float4(gf_act(widen(t.v[0]), f), gf_act(widen(t.v[1]), f), gf_act(widen(t.v[2]), f), gf_act(widen(t.v[3]), f));
            }
            *reinterpret_cast<float4 *>(&s_a[cc][r][4 + q * 4]) = o;
        }
        if (threadIdx.x < GF_CH * GF_LH * 2) {
            const int it = threadIdx.x, side = it & 1, r = (it >> 1) % GF_LH, cc = it / (2 * GF_LH);
            const int gy = ty0 + r - 1, gx = side ? tx0 + GF_TW : tx0 - 1;
            float o = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) o = gf_act(widen(xn[(size_t)(c0 + cc) * HW + (size_t)gy * W + gx]), tab[c0 + cc]);
            s_a[cc][r][side ? 4 + GF_TW : 3] = o;
        }
    } else {
        for (int it = threadIdx.x; it < GF_CH * GF_LH * (GF_TW + 2); it += 256) {
            const int q = it % (GF_TW + 2), r = (it / (GF_TW + 2)) % GF_LH, cc = it / ((GF_TW + 2) * GF_LH);
            const int gy = ty0 + r - 1, gx = tx0 + q - 1;
            float o = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) o = gf_act(widen(xn[(size_t)(c0 + cc) * HW + (size_t)gy * W + gx]), tab[c0 + cc]);
            s_a[cc][r][3 + q] = o;
        }
    }
}

// the 3 x 6 window of one channel a thread's four pixels read: rows ty .. ty + 2 of the staged tile, columns 4 tx - 1 .. 4 tx + 4
__device__ __forceinline__ void gf_window(const float (*__restrict__ s)[GF_LW], int ty, int tx, float v[3][6]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float4 m = *reinterpret_cast<const float4 *>(&s[ty + r][4 + tx * 4]);
        v[r][0] = s[ty + r][3 + tx * 4];
        v[r][1] = m.x;
        v[r][2] = m.y;
        v[r][3] = m.z;
        v[r][4] = m.w;
        v[r][5] = s[ty + r][8 + tx * 4];
    }
}

template <int DTX, int DTY>
struct GfFwd {
    const dtype_t<DTX> *x;
    const double *partial;
    const float *gamma, *beta, *bias;
    dtype_t<DTY> *y;
    float *stats_out;
    int H, W, chunks, vec_x, vec_y;
    float eps;
};

template <int DTX, int DTY>
__global__ void __launch_bounds__(256) gf_fwd_kernel(const GfFwd<DTX, DTY> p, const float *__restrict__ w) {
    __shared__ __attribute__((aligned(16))) float s_a[GF_CH][GF_LH][GF_LW];
    __shared__ float4 s_tab[GF_C];
    const int n = blockIdx.z, ty0 = blockIdx.y * GF_TH, tx0 = blockIdx.x * GF_TW;
    const int H = p.H, W = p.W;
    const size_t HW = (size_t)H * W;
    const dtype_t<DTX> *xn = p.x + (size_t)n * GF_C * HW;

    if (threadIdx.x < GF_G) {   // statistics, stage 2: this frame's 32 (mean, rstd) from the chunk partials, in double
        const int g = threadIdx.x;
        const size_t grp = (size_t)n * GF_G + g;
        double a = 0.0, b = 0.0;
        for (int c = 0; c < p.chunks; ++c) {
            a += p.partial[(grp * p.chunks + c) * 2];
            b += p.partial[(grp * p.chunks + c) * 2 + 1];
        }
        const double cnt = (double)GF_CPG * (double)HW, k = (double)widen(xn[(size_t)g * GF_CPG * HW]);
        const double d = a / cnt, mean = k + d;
        double var = b / cnt - d * d;
        if (var < 0.0) var = 0.0;
        const float mean_hi = (float)mean, mean_lo = (float)(mean - (double)mean_hi), rstd = (float)(1.0 / sqrt(var + (double)p.eps));
#pragma unroll
        for (int j = 0; j < GF_CPG; ++j) {
            const int c = g * GF_CPG + j;
            s_tab[c] = make_float4(mean_hi, mean_lo, rstd * p.gamma[c], p.beta[c]);
        }
        if (p.stats_out && blockIdx.x == 0 && blockIdx.y == 0) {
            p.stats_out[grp * 2] = mean_hi;
            p.stats_out[grp * 2 + 1] = rstd;
        }
    }

    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[GF_CO][4];
#pragma unroll
    for (int o = 0; o < GF_CO; ++o) {
        const float b = p.bias[o];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = b;
    }
    for (int c0 = 0; c0 < GF_C; c0 += GF_CH) {
        __syncthreads();   // (s_tab is written; the previous step's reads of s_a are done)
        gf_stage<DTX>(xn, c0, H, W, ty0, tx0, p.vec_x != 0, s_tab, s_a);
        __syncthreads();
#pragma nounroll   // (one channel's 27 weights in scalar registers at a time: four channels' 108 spill them)
        for (int cc = 0; cc < GF_CH; ++cc) {
            float v[3][6];
            gf_window(s_a[cc], ty, tx, v);
            const float *wc = w + (c0 + cc) * 9;
#pragma unroll
            for (int o = 0; o < GF_CO; ++o)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const float wv = wc[o * GF_C * 9 + r * 3 + t];
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(v[r][j + t], wv, acc[o][j]);
                    }
        }
    }

    const int gy = ty0 + ty, gx = tx0 + tx * 4;
    if (gy >= H || gx >= W) return;
    dtype_t<DTY> *yn = p.y + (size_t)n * GF_CO * HW + (size_t)gy * W + gx;
#pragma unroll
    for (int o = 0; o < GF_CO; ++o) {
        vec4_of<DTY> out;
#pragma unroll
        for (int j = 0; j < 4; ++j) out.v[j] = narrow<DTY>(1.0f / (1.0f + expf(-acc[o][j])));
        if (p.vec_y) {
            *reinterpret_cast<vec4_of<DTY> *>(yn + (size_t)o * HW) = out;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (gx + j < W) yn[(size_t)o * HW + j] = out.v[j];
        }
    }
}

struct GfBwd {
    const float *x, *y, *dy, *stats, *gamma, *beta;
    float *a, *da, *part;
    int H, W, vec;
};

// DW: also this workgroup's partial of dW and db (false when neither is wanted)
template <bool DW>
__global__ void __launch_bounds__(256) gf_bwd_kernel(const GfBwd p, const float *__restrict__ w) {
    __shared__ __attribute__((aligned(16))) float s_a[GF_CH][GF_LH][GF_LW];
    __shared__ __attribute__((aligned(16))) float s_dv[GF_CO][GF_LH][GF_LW];
    __shared__ float4 s_tab[GF_C];
    __shared__ float s_red[4][GF_CH * 27 + 4];
    const int n = blockIdx.z, ty0 = blockIdx.y * GF_TH, tx0 = blockIdx.x * GF_TW;
    const int H = p.H, W = p.W;
    const size_t HW = (size_t)H * W;
    const float *xn = p.x + (size_t)n * GF_C * HW;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *part = p.part + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * GF_PART;

    if (threadIdx.x < GF_C) {
        const int c = threadIdx.x;
        const size_t grp = (size_t)n * GF_G + c / GF_CPG;
        s_tab[c] = make_float4(p.stats[grp * 2], 0.0f, p.stats[grp * 2 + 1] * p.gamma[c], p.beta[c]);
    }
    // dv = dy * y * (1 - y) of the tile + halo, 0 outside the image
    for (int it = threadIdx.x; it < GF_CO * GF_LH * (GF_TW + 2); it += 256) {
        const int q = it % (GF_TW + 2), r = (it / (GF_TW + 2)) % GF_LH, o = it / ((GF_TW + 2) * GF_LH);
        const int gy = ty0 + r - 1, gx = tx0 + q - 1;
        float v = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t i = ((size_t)n * GF_CO + o) * HW + (size_t)gy * W + gx;
            const float yv = p.y[i];
            v = p.dy[i] * yv * (1.0f - yv);
        }
        s_dv[o][r][3 + q] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float dv[GF_CO][3][6];
#pragma unroll
    for (int o = 0; o < GF_CO; ++o) gf_window(s_dv[o], ty, tx, dv[o]);
    if (DW) {   // db: this tile's sum of dv
#pragma unroll
        for (int o = 0; o < GF_CO; ++o) {
            const float s = gf_wave_sum((dv[o][1][1] + dv[o][1][2]) + (dv[o][1][3] + dv[o][1][4]));
            if (lane == 0) s_red[wave][GF_CH * 27 + o] = s;
        }
        __syncthreads();
        if (threadIdx.x < GF_CO) {
            const int o = threadIdx.x;
            part[GF_NW + o] = (s_red[0][GF_CH * 27 + o] + s_red[1][GF_CH * 27 + o]) + (s_red[2][GF_CH * 27 + o] + s_red[3][GF_CH * 27 + o]);
        }
    }

    const int gy = ty0 + ty, gx = tx0 + tx * 4;
    const bool inside = gy < H && gx < W;
    for (int c0 = 0; c0 < GF_C; c0 += GF_CH) {
        __syncthreads();
        gf_stage<MPHIP_DTYPE_F32>(xn, c0, H, W, ty0, tx0, p.vec != 0, s_tab, s_a);
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < GF_CH; ++cc) {
            float v[3][6];
            gf_window(s_a[cc], ty, tx, v);
            const float *wc = w + (c0 + cc) * 9;
            // da[c, p] = sum_{o, tap} dv[o, p - tap] * W[o, c, tap]
            float da[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int o = 0; o < GF_CO; ++o)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const float wv = wc[o * GF_C * 9 + r * 3 + t];
#pragma unroll
                        for (int j = 0; j < 4; ++j) da[j] = fmaf(dv[o][2 - r][j + 2 - t], wv, da[j]);
                    }
            if (inside) {
                const size_t i = ((size_t)n * GF_C + c0 + cc) * HW + (size_t)gy * W + gx;
                if (p.vec) {
                    *reinterpret_cast<float4 *>(p.a + i) = make_float4(v[1][1], v[1][2], v[1][3], v[1][4]);
                    *reinterpret_cast<float4 *>(p.da + i) = make_float4(da[0], da[1], da[2], da[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (gx + j < W) {
                            p.a[i + j] = v[1][1 + j];
                            p.da[i + j] = da[j];
                        }
                }
            }
            if (DW) {   // dW[o, c, tap] = sum_p dv[o, p] * a[c, p + tap]  (dv is 0 at the pixels of the tile that are outside the image)
#pragma unroll
                for (int o = 0; o < GF_CO; ++o)
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int t = 0; t < 3; ++t) {
                            float s = 0.0f;
#pragma unroll
                            for (int j = 0; j < 4; ++j) s = fmaf(dv[o][1][1 + j], v[r][j + t], s);
                            s = gf_wave_sum(s);
                            if (lane == 0) s_red[wave][cc * 27 + o * 9 + r * 3 + t] = s;
                        }
            }
        }
        if (DW) {
            __syncthreads();
            if (threadIdx.x < GF_CH * 27) {
                const int i = threadIdx.x, cc = i / 27, o = (i % 27) / 9, tap = i % 9;
                part[(o * GF_C + c0 + cc) * 9 + tap] = (s_red[0][i] + s_red[1][i]) + (s_red[2][i] + s_red[3][i]);
            }
        }
    }
}

// (dW, db) = the workgroups' partials added in a fixed order: 16 slices of consecutive workgroups per output, then the 16 slice sums
__global__ void __launch_bounds__(256) gf_fold_kernel(const float *__restrict__ part, int nwg, float *__restrict__ dw, float *__restrict__ db) {
    __shared__ float red[16][16];
    const int col = threadIdx.x & 15, slice = threadIdx.x >> 4, i = blockIdx.x * 16 + col;
    const int per = (nwg + 15) / 16, b = slice * per, e = b + per < nwg ? b + per : nwg;
    float s = 0.0f;
    if (i < GF_NW + GF_CO) {
#pragma unroll 8
        for (int k = b; k < e; ++k) s += part[(size_t)k * GF_PART + i];
    }
    red[slice][col] = s;
    __syncthreads();
    if (slice == 0 && i < GF_NW + GF_CO) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][col];
        if (i < GF_NW) {
            if (dw) dw[i] = t;
        } else if (db) {
            db[i - GF_NW] = t;
        }
    }
}

static inline size_t gf_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int gf_chunks(int H, int W) { return (int)(((size_t)GF_CPG * H * W + GF_CHUNK - 1) / GF_CHUNK); }
inline size_t gf_tiles(int N, int H, int W) { return (size_t)N * cdiv(H, GF_TH) * cdiv(W, GF_TW); }
inline size_t gf_fwd_bytes(int N, int H, int W) { return gf_align((size_t)N * GF_G * gf_chunks(H, W) * 2 * sizeof(double)); }
inline size_t gf_plane_bytes(int N, int H, int W) { return gf_align((size_t)N * GF_C * H * W * sizeof(float)); }
inline size_t gf_part_bytes(int N, int H, int W) { return gf_align(gf_tiles(N, H, W) * GF_PART * sizeof(float)); }

static bool gf_shape_ok(const char *what, int N, int C, int Co, int H, int W, int G) {
    if (C != GF_C || G != GF_G || Co != GF_CO) {
        set_error("%s: only C=64, G=32, Co=3 is covered (C=%d G=%d Co=%d)", what, C, G, Co);
        return false;
    }
    if (N < 1 || N > 65535 || H < 1 || W < 1 || cdiv(H, GF_TH) > 65535 || (size_t)H * W > ((size_t)1 << 40)) {
        set_error("%s: bad dims (N=%d H=%d W=%d)", what, N, H, W);
        return false;
    }
    return true;
}

template <int DTX, int DTY>
int gf_fwd_launch(const void *x, const float *gamma, const float *beta, const float *w, const float *bias, void *y, float *stats_out, int N,
                  int H, int W, float eps, void *workspace, hipStream_t s) {
    const int chunks = gf_chunks(H, W);
    const size_t cnt = (size_t)GF_CPG * H * W;
    const int vec_x = W % 4 == 0 && ((uintptr_t)x & (sizeof(dtype_t<DTX>) * 4 - 1)) == 0;
    const int vec_y = W % 4 == 0 && ((uintptr_t)y & (sizeof(dtype_t<DTY>) * 4 - 1)) == 0;
    hipLaunchKernelGGL(gf_stats_partial_kernel<DTX>, dim3(chunks, N * GF_G), dim3(256), 0, s, (const dtype_t<DTX> *)x, (double *)workspace, cnt,
                       chunks, vec_x && cnt % 4 == 0);
    GfFwd<DTX, DTY> p;
    p.x = (const dtype_t<DTX> *)x;
    p.partial = (const double *)workspace;
    p.gamma = gamma;
    p.beta = beta;
    p.bias = bias;
    p.y = (dtype_t<DTY> *)y;
    p.stats_out = stats_out;
    p.H = H;
    p.W = W;
    p.chunks = chunks;
    p.vec_x = vec_x;
    p.vec_y = vec_y;
    p.eps = eps;
    hipLaunchKernelGGL((gf_fwd_kernel<DTX, DTY>), dim3(cdiv(W, GF_TW), cdiv(H, GF_TH), N), dim3(256), 0, s, p, w);
    return check_launch("g2d_final_fwd");
}

}  // namespace mphip

using namespace mphip;

extern "C" size_t mphip_g2d_final_workspace_bytes(int N, int C, int H, int W, int G, int backward) {
    if (C != GF_C || G != GF_G || N < 1 || H < 1 || W < 1) return 0;
    if (!backward) return gf_fwd_bytes(N, H, W);
    return 2 * gf_plane_bytes(N, H, W) + gf_part_bytes(N, H, W) + gf_align(mphip_groupnorm_bwd_workspace_bytes(N, C, H * W));
}

extern "C" int mphip_g2d_final_fwd(const void *x, int x_dtype, const float *gamma, const float *beta, const float *w, const float *bias,
                                   void *y, int y_dtype, float *stats_out, int N, int C, int Co, int H, int W, int G, float eps,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(x && gamma && beta && w && bias && y, "g2d_final_fwd: null pointer");
    if (!gf_shape_ok("g2d_final_fwd", N, C, Co, H, W, G)) return MPHIP_EINVAL;
    const size_t need = gf_fwd_bytes(N, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("g2d_final_fwd: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    return dispatch_dtype(x_dtype, "g2d_final_fwd: unknown input dtype", [&](auto dx) {
        return dispatch_dtype(y_dtype, "g2d_final_fwd: unknown output dtype", [&](auto dy) {
            return gf_fwd_launch<decltype(dx)::value, decltype(dy)::value>(x, gamma, beta, w, bias, y, stats_out, N, H, W, eps, workspace, s);
        });
    });
}

extern "C" int mphip_g2d_final_bwd(const float *x, const float *y, const float *dy, const float *stats, const float *gamma,
                                   const float *beta, const float *w, float *dx, float *dgamma, float *dbeta, float *dw, float *db, int N,
                                   int C, int Co, int H, int W, int G, void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(x && y && dy && stats && gamma && beta && w && dx && dgamma && dbeta, "g2d_final_bwd: null pointer");
    if (!gf_shape_ok("g2d_final_bwd", N, C, Co, H, W, G)) return MPHIP_EINVAL;
    MPHIP_REQUIRE((size_t)H * W <= 0x7fffffffu, "g2d_final_bwd: H*W = %zu does not fit the GroupNorm backward", (size_t)H * W);
    const size_t need = mphip_g2d_final_workspace_bytes(N, C, H, W, G, 1);
    if (!workspace || workspace_bytes < need) {
        set_error("g2d_final_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    GfBwd p;
    p.x = x;
    p.y = y;
    p.dy = dy;
    p.stats = stats;
    p.gamma = gamma;
    p.beta = beta;
    p.a = (float *)ws;
    p.da = (float *)(ws + gf_plane_bytes(N, H, W));
    p.part = (float *)(ws + 2 * gf_plane_bytes(N, H, W));
    void *gn_ws = ws + 2 * gf_plane_bytes(N, H, W) + gf_part_bytes(N, H, W);
    p.H = H;
    p.W = W;
    p.vec = W % 4 == 0 && ((uintptr_t)x & 15) == 0;   // (a and da start 256-byte aligned in the workspace)
    MPHIP_REQUIRE(((uintptr_t)workspace & 15) == 0, "g2d_final_bwd: the workspace must be 16-byte aligned");
    const dim3 grid(cdiv(W, GF_TW), cdiv(H, GF_TH), N);
    if (dw || db) {
        hipLaunchKernelGGL(gf_bwd_kernel<true>, grid, dim3(256), 0, s, p, w);
        hipLaunchKernelGGL(gf_fold_kernel, dim3(cdiv(GF_NW + GF_CO, 16)), dim3(256), 0, s, (const float *)p.part, (int)gf_tiles(N, H, W), dw, db);
    } else {
        hipLaunchKernelGGL(gf_bwd_kernel<false>, grid, dim3(256), 0, s, p, w);
    }
    const int rc = check_launch("g2d_final_bwd");
    if (rc != MPHIP_OK) return rc;
    return mphip_groupnorm_bwd(x, p.a, p.da, stats, gamma, beta, nullptr, dx, nullptr, dgamma, dbeta, nullptr, nullptr, N, C, H * W, G, 1, gn_ws,
                               mphip_groupnorm_bwd_workspace_bytes(N, C, H * W), stream);
}
