// K13 — what lies between the convs of a VGG19 perceptual loss (losses.py: VGG19FeatureLoss), forward and backward to the predicted
// image.  The thirteen 3x3 convs are ops.conv2d / ops.conv2d_bwd_data and the first one ops.conv2d_stem; this unit holds the rest:
//     maxpool2_fwd             nn.MaxPool2d(2, 2), floor mode, with the range descriptor of its output
//     feature_l1               coeff * sum |y_pred - y_target| of one tap, fp64 partial sums in a fixed order
//     feature_grad_assemble    g = (upstream + coeff * sgn(y_pred - y_target)) * (y_pred > 0) and g's operand scale, in one pass;
//                              upstream: nothing, a same-size dx, or a half-size gradient routed through the 2x2 max-pool
//     conv2d_stem_bwd_data     dx [N,3,H,W] of nn.Conv2d(3, Co, 3, padding=1), exact fp32 in a fixed FMA order
// All maps are NCHW fp32.  These are streaming passes: rows are read with 16-byte loads when W % 4 == 0 and the maps lie on 16-byte
// boundaries, element by element with masks otherwise (the same values; feature_l1's two forms add in a different, equally fixed
// order).  No atomics and no memset: a workgroup leaves its partial (a maximum, a sum) in its own slot with a plain store and a second
// small launch folds the slots in index order, so two calls give the same bits and every call can be captured.
// The max-pool's rule is ATen's: the window is scanned in (row, column) order from -inf and an element replaces the maximum when
// `val > max || isnan(val)`: the FIRST of equal maxima wins, NaN wins.  An odd last row or column belongs to no window.
#include "mphip_common.h"

namespace mphip {

constexpr unsigned FL_MAX_BLOCKS = RANGE_MAX_PARTS;   // workgroups of the grid-stride passes: one descriptor / workspace slot each
constexpr unsigned FL_L1_BLOCKS = 1024;               // workgroups (fp64 partial sums) of feature_l1

__device__ __forceinline__ bool pool_takes(float v, float m) { return v > m || v != v; }

// ---------------------------------------------------------------------------------------------------------------- max-pool 2x2
// VEC: a thread owns two windows (two float4 of x, one float2 of y); else one window, four 4-byte loads.
template <bool VEC>
__global__ void __launch_bounds__(256)
maxpool2_kernel(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ out_range, int H, int W, int Ho, int Wo,
                unsigned long long items) {
    const int wq = VEC ? Wo / 2 : Wo;
    unsigned bits = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < items; i += stride) {
        const int j = (int)(i % wq);
        const unsigned long long t = i / wq;
        const int r = (int)(t % Ho);
        const size_t plane = (size_t)(t / Ho);
        const float *r0 = x + (plane * H + 2 * r) * W, *r1 = r0 + W;
        float *o = y + (plane * Ho + r) * Wo;
        if constexpr (VEC) {
            const float4 a = *reinterpret_cast<const float4 *>(r0 + 4 * j), b = *reinterpret_cast<const float4 *>(r1 + 4 * j);
            float m0 = -__builtin_inff(), m1 = m0;
            m0 = pool_takes(a.x, m0) ? a.x : m0, m0 = pool_takes(a.y, m0) ? a.y : m0;
            m0 = pool_takes(b.x, m0) ? b.x : m0, m0 = pool_takes(b.y, m0) ? b.y : m0;
            m1 = pool_takes(a.z, m1) ? a.z : m1, m1 = pool_takes(a.w, m1) ? a.w : m1;
            m1 = pool_takes(b.z, m1) ? b.z : m1, m1 = pool_takes(b.w, m1) ? b.w : m1;
            *reinterpret_cast<float2 *>(o + 2 * j) = make_float2(m0, m1);
            bits = max(bits, max(range_bits(m0), range_bits(m1)));
        } else {
            const float v00 = r0[2 * j], v01 = r0[2 * j + 1], v10 = r1[2 * j], v11 = r1[2 * j + 1];
            float m = -__builtin_inff();
            m = pool_takes(v00, m) ? v00 : m, m = pool_takes(v01, m) ? v01 : m;
            m = pool_takes(v10, m) ? v10 : m, m = pool_takes(v11, m) ? v11 : m;
            o[j] = m;
            bits = max(bits, range_bits(m));
        }
    }
    if (out_range) range_note_block(bits, out_range, blockIdx.x, gridDim.x);   // (kernel-uniform branch; a barrier inside)
}

static bool maxpool2_shape_ok(int NC, int H, int W) {
    return NC >= 1 && H >= 2 && W >= 2 && (unsigned long long)NC * H * W < (1ull << 31);
}

// ---------------------------------------------------------------------------------------------------------------- the L1 tap
// y holds 2N samples of M floats: predicted first, then target.  T = N * M differences.
template <bool VEC>
__global__ void __launch_bounds__(256)
feature_l1_partial_kernel(const float *__restrict__ y, double *__restrict__ partial, size_t T) {
    const float *p = y, *t = y + T;
    double acc = 0.0;
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {   // T % 4 == 0 and y 16-byte aligned: the target half starts on a 16-byte boundary too
        for (size_t i = first; i < T / 4; i += stride) {
            const float4 a = reinterpret_cast<const float4 *>(p)[i], b = reinterpret_cast<const float4 *>(t)[i];
            acc += (double)fabsf(a.x - b.x);
            acc += (double)fabsf(a.y - b.y);
            acc += (double)fabsf(a.z - b.z);
            acc += (double)fabsf(a.w - b.w);
        }
    } else {
        for (size_t i = first; i < T; i += stride) acc += (double)fabsf(p[i] - t[i]);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(256)
feature_l1_finish_kernel(const double *__restrict__ partial, unsigned n, double coeff, float *__restrict__ loss_out) {
    __shared__ double part[FL_L1_BLOCKS];
    for (unsigned i = threadIdx.x; i < n; i += 256) part[i] = partial[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (unsigned i = 0; i < n; ++i) s += part[i];   // index order
        loss_out[0] = (float)(s * coeff);                // the one rounding to fp32
    }
}

static bool feature_l1_shape_ok(int N, int M) { return N >= 1 && M >= 1 && 2ull * (unsigned long long)N * M < (1ull << 31); }

static unsigned feature_l1_blocks(int N, int M) {
    const unsigned long long want = ((unsigned long long)N * M + 1023) / 1024;   // (a thread of the 16-byte form: one float4 pair)
    return (unsigned)(want < FL_L1_BLOCKS ? want : FL_L1_BLOCKS);
}

// ---------------------------------------------------------------------------------------------------------------- gradient assembly
struct FgaArgs {
    int H, W, Hp, Wp;          // the map; the pooled map (kind 2): H / 2, W / 2
    int ph, pw;                // patches of a plane: 2 rows x CW columns each
    int kind;                  // upstream: 0 none, 1 dx [N,C,H,W], 2 dpool [N,C,Hp,Wp]
    unsigned long long items;  // N * C * ph * pw
    size_t half;               // N * C * H * W: the target half of y starts there
};

// CW == 4: rows by 16-byte accesses (W % 4 == 0, y / g / dx on 16-byte boundaries); CW == 2: masked elements.  A thread owns the rows
// 2i, 2i+1 and CW columns of one predicted plane: whole pool windows, so the routing needs no neighbour.
template <int CW>
__global__ void __launch_bounds__(256)
feature_grad_assemble_kernel(const float *__restrict__ y, const float *__restrict__ up, const float *__restrict__ coeff,
                             float *__restrict__ g, float *__restrict__ partial, const FgaArgs a) {
    const bool tap = coeff != nullptr;
    const float cf = tap ? coeff[0] : 0.0f;
    const int H = a.H, W = a.W;
    float mx = 0.0f;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < a.items; i += stride) {
        const int pj = (int)(i % a.pw);
        const unsigned long long t = i / a.pw;
        const int pi = (int)(t % a.ph);
        const size_t plane = (size_t)(t / a.ph);
        const int c0 = CW * pj;
        float yp[2][CW], yt[2][CW], u[2][CW];
        bool ok[2][CW];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = 2 * pi + r;
            const size_t o = (plane * H + min(row, H - 1)) * W + c0;
            if constexpr (CW == 4) {
                const float4 vp = *reinterpret_cast<const float4 *>(y + o), vt = *reinterpret_cast<const float4 *>(y + a.half + o);
                yp[r][0] = vp.x, yp[r][1] = vp.y, yp[r][2] = vp.z, yp[r][3] = vp.w;
                yt[r][0] = vt.x, yt[r][1] = vt.y, yt[r][2] = vt.z, yt[r][3] = vt.w;
                float4 vu = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (a.kind == 1) vu = *reinterpret_cast<const float4 *>(up + o);
                u[r][0] = vu.x, u[r][1] = vu.y, u[r][2] = vu.z, u[r][3] = vu.w;
#pragma unroll
                for (int k = 0; k < CW; ++k) ok[r][k] = row < H;
            } else {
#pragma unroll
                for (int k = 0; k < CW; ++k) {
                    ok[r][k] = row < H && c0 + k < W;
                    const size_t e = o - c0 + min(c0 + k, W - 1);   // (clamped into the plane: the value is dropped when !ok)
                    yp[r][k] = y[e];
                    yt[r][k] = y[a.half + e];
                    u[r][k] = a.kind == 1 ? up[e] : 0.0f;
                }
            }
        }
        if (a.kind == 2) {   // route the pooled gradient to the first maximum of its window; no window: 0
#pragma unroll
            for (int q = 0; q < CW / 2; ++q) {
                const int wj = c0 / 2 + q;
                const bool in = pi < a.Hp && wj < a.Wp;   // (then the window's four elements are inside the map)
                const float d = in ? up[(plane * a.Hp + min(pi, a.Hp - 1)) * a.Wp + min(wj, a.Wp - 1)] : 0.0f;
                float m = -__builtin_inff();
                int at = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = yp[e >> 1][2 * q + (e & 1)];
                    if (pool_takes(v, m)) m = v, at = e;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e >> 1][2 * q + (e & 1)] = in && at == e ? d : 0.0f;
            }
        }
        float gv[2][CW];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < CW; ++k) {
                float v = u[r][k];
                if (tap) {
                    const float s = yp[r][k] - yt[r][k];
                    v = v + (s > 0.0f ? cf : s < 0.0f ? -cf : 0.0f);   // the one rounding when both terms exist; sgn(0) = sgn(NaN) = 0
                }
                gv[r][k] = yp[r][k] > 0.0f ? v : 0.0f;
                if (ok[r][k]) mx = fmaxf(mx, fabsf(gv[r][k]));
            }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = 2 * pi + r;
            const size_t o = (plane * H + min(row, H - 1)) * W + c0;
            if constexpr (CW == 4) {
                if (row < H) *reinterpret_cast<float4 *>(g + o) = make_float4(gv[r][0], gv[r][1], gv[r][2], gv[r][3]);
            } else {
#pragma unroll
                for (int k = 0; k < CW; ++k)
                    if (ok[r][k]) g[o + k] = gv[r][k];
            }
        }
    }
    // max|g| of the workgroup, the way grad_prep_partial_kernel takes it (fmaxf: a NaN does not enter the maximum)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    __shared__ float redm[4];
    if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
}

// scale[0..2] = (s, 1 / s, max|g|) by grad_prep_finalize_kernel's rule (scale_from_bits); scale[3] = 0
__global__ void __launch_bounds__(256)
feature_grad_scale_kernel(const float *__restrict__ partial, unsigned n, float *__restrict__ scale) {
    float m = 0.0f;
    for (unsigned i = threadIdx.x; i < n; i += 256) m = fmaxf(m, partial[i]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    __shared__ float redm[4];
    if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
        float sc, inv;
        scale_from_bits(range_bits(m), sc, inv);
        scale[0] = sc;
        scale[1] = inv;
        scale[2] = m;
        scale[3] = 0.0f;
    }
}

static bool fga_shape_ok(int N, int C, int H, int W, int kind) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || kind < 0 || kind > 2) return false;
    if (kind == 2 && (H < 2 || W < 2)) return false;
    return 2ull * (unsigned long long)N * C * (unsigned long long)H * W < (1ull << 31);
}

static unsigned fga_blocks(int N, int C, int H, int W, int cw) {
    const unsigned long long items = (unsigned long long)N * C * ((H + 1) / 2) * ((W + cw - 1) / cw), want = (items + 255) / 256;
    return (unsigned)(want < FL_MAX_BLOCKS ? want : FL_MAX_BLOCKS);
}

// ---------------------------------------------------------------------------------------------------------------- stem backward-data
//     dx[n,ci,h,w] = sum_{co,kh,kw} w[co,ci,kh,kw] * dy[n,co,h+1-kh,w+1-kw]            (dy is zero outside the map)
// acc = +0, then fmaf(w, dy, acc) over co = 0 .. Co-1, kh = 0..2, kw = 0..2 in that nesting.  As in the forward stem the 27 weights of an
// output channel are wave-uniform (scalar loads) and a thread keeps a 2 x 2 pixel patch of all three input channels in registers: a
// 4 x 4 window of dy per output channel feeds 108 FMAs.  A workgroup is 32 x 8 patches: 64 columns x 16 rows of one image.
constexpr int SB_PW = 32, SB_PH = 8;

__global__ void __launch_bounds__(256)
conv2d_stem_bwd_data_kernel(const float *__restrict__ dy, const float *__restrict__ w, float *__restrict__ dx, int Co, int H, int W,
                            int tiles_w, int tiles_h) {
    unsigned t = blockIdx.x;
    const int tw = t % tiles_w;
    t /= tiles_w;
    const int th = t % tiles_h, n = t / tiles_h;
    const int r0 = (th * SB_PH + (int)(threadIdx.x >> 5)) * 2, c0 = (tw * SB_PW + (int)(threadIdx.x & 31)) * 2;
    const size_t HW = (size_t)H * W;
    const float *dyn = dy + (size_t)n * Co * HW;
    size_t off[4][4];
    bool in[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // (every load is issued, from an address clamped into the map, and the zero selected afterwards: conv2d_stem.hip)
            const int gy = r0 - 1 + r, gx = c0 - 1 + c;
            in[r][c] = gy >= 0 && gy < H && gx >= 0 && gx < W;
            off[r][c] = (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
        }
    float acc[3][2][2];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) acc[ci][0][0] = acc[ci][0][1] = acc[ci][1][0] = acc[ci][1][1] = 0.0f;
    for (int co = 0; co < Co; ++co) {
        const float *wc = w + (size_t)co * 27;   // wave-uniform
        const float *dc = dyn + (size_t)co * HW;
        float d[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float v = dc[off[r][c]];
                d[r][c] = in[r][c] ? v : 0.0f;
            }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float wv = wc[(ci * 3 + kh) * 3 + kw];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int c = 0; c < 2; ++c) acc[ci][r][c] = fmaf(wv, d[r + 2 - kh][c + 2 - kw], acc[ci][r][c]);
                }
    }
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (r0 + r < H && c0 + c < W) dx[((size_t)n * 3 + ci) * HW + (size_t)(r0 + r) * W + (c0 + c)] = acc[ci][r][c];
}

static bool stem_bwd_shape_ok(int N, int Co, int H, int W) {
    if (N < 1 || Co < 16 || Co % 16 != 0 || H < 1 || W < 1) return false;
    return (unsigned long long)N * Co * (unsigned long long)H * W < (1ull << 31);   // (dx is the smaller map)
}

static bool fl_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_maxpool2_supported(int NC, int H, int W) { return maxpool2_shape_ok(NC, H, W) ? 1 : 0; }

extern "C" int mphip_maxpool2_fwd(const float *x, float *y, float *out_range, int NC, int H, int W, void *stream) {
    MPHIP_REQUIRE(x && y, "maxpool2_fwd: null pointer");
    MPHIP_REQUIRE(maxpool2_shape_ok(NC, H, W), "maxpool2_fwd: unsupported shape NC=%d H=%d W=%d (NC >= 1, H, W >= 2, fewer than 2^31 elements)",
                  NC, H, W);
    MPHIP_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)out_range) & 3) == 0, "maxpool2_fwd: x, y and out_range must be 4-byte aligned");
    const int Ho = H / 2, Wo = W / 2;
    MPHIP_REQUIRE(!fl_overlap(y, (size_t)NC * Ho * Wo * sizeof(float), x, (size_t)NC * H * W * sizeof(float)), "maxpool2_fwd: y must not alias x");
    const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const unsigned long long items = (unsigned long long)NC * Ho * (vec ? Wo / 2 : Wo), want = (items + 255) / 256;
    const unsigned blocks = (unsigned)(want < FL_MAX_BLOCKS ? want : FL_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(maxpool2_kernel<true>, dim3(blocks), dim3(256), 0, s, x, y, out_range, H, W, Ho, Wo, items);
    else     hipLaunchKernelGGL(maxpool2_kernel<false>, dim3(blocks), dim3(256), 0, s, x, y, out_range, H, W, Ho, Wo, items);
    return check_launch("maxpool2_fwd");
}

extern "C" int mphip_feature_l1_supported(int N, int M) { return feature_l1_shape_ok(N, M) ? 1 : 0; }

extern "C" size_t mphip_feature_l1_workspace_bytes(int N, int M) {
    return feature_l1_shape_ok(N, M) ? (size_t)feature_l1_blocks(N, M) * sizeof(double) : 0;
}

extern "C" int mphip_feature_l1(const float *y, int N, int M, double coeff, float *loss_out, void *workspace, size_t workspace_bytes,
                                void *stream) {
    MPHIP_REQUIRE(y && loss_out, "feature_l1: null pointer");
    MPHIP_REQUIRE(feature_l1_shape_ok(N, M), "feature_l1: unsupported shape N=%d M=%d (N, M >= 1, fewer than 2^31 elements in the 2N samples)", N, M);
    MPHIP_REQUIRE((((uintptr_t)y | (uintptr_t)loss_out) & 3) == 0, "feature_l1: y and loss_out must be 4-byte aligned");
    const size_t need = mphip_feature_l1_workspace_bytes(N, M);
    if (!workspace || workspace_bytes < need) {
        set_error("feature_l1: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    MPHIP_REQUIRE(((uintptr_t)workspace & 15) == 0, "feature_l1: workspace must be 16-byte aligned");
    const size_t T = (size_t)N * M;
    const unsigned blocks = feature_l1_blocks(N, M);
    hipStream_t s = (hipStream_t)stream;
    if (T % 4 == 0 && ((uintptr_t)y & 15) == 0)
        hipLaunchKernelGGL(feature_l1_partial_kernel<true>, dim3(blocks), dim3(256), 0, s, y, (double *)workspace, T);
    else
        hipLaunchKernelGGL(feature_l1_partial_kernel<false>, dim3(blocks), dim3(256), 0, s, y, (double *)workspace, T);
    hipLaunchKernelGGL(feature_l1_finish_kernel, dim3(1), dim3(256), 0, s, (const double *)workspace, blocks, coeff, loss_out);
    return check_launch("feature_l1");
}

extern "C" int mphip_feature_grad_assemble_supported(int N, int C, int H, int W, int upstream) { return fga_shape_ok(N, C, H, W, upstream) ? 1 : 0; }

extern "C" size_t mphip_feature_grad_assemble_workspace_bytes(int N, int C, int H, int W) {
    return fga_shape_ok(N, C, H, W, 0) ? (size_t)fga_blocks(N, C, H, W, 2) * sizeof(float) : 0;   // (the element form starts the most workgroups)
}

extern "C" int mphip_feature_grad_assemble(const float *y, const float *upstream_grad, int upstream, const float *coeff, float *g, float *scale,
                                           int N, int C, int H, int W, void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(y && g && scale && (upstream == 0 || upstream_grad), "feature_grad_assemble: null pointer");
    MPHIP_REQUIRE(fga_shape_ok(N, C, H, W, upstream),
                  "feature_grad_assemble: unsupported shape N=%d C=%d H=%d W=%d upstream=%d (N, C, H, W >= 1, upstream 0, 1 or 2, H, W >= 2 with a "
                  "pooled upstream, fewer than 2^31 elements in the 2N samples)", N, C, H, W, upstream);
    MPHIP_REQUIRE(upstream != 0 || coeff, "feature_grad_assemble: neither an upstream gradient nor a tap");
    MPHIP_REQUIRE((((uintptr_t)y | (uintptr_t)upstream_grad | (uintptr_t)coeff | (uintptr_t)g | (uintptr_t)scale) & 3) == 0,
                  "feature_grad_assemble: y, the upstream gradient, coeff, g and scale must be 4-byte aligned");
    const size_t half = (size_t)N * C * H * W;
    MPHIP_REQUIRE(!fl_overlap(g, half * sizeof(float), y, 2 * half * sizeof(float)), "feature_grad_assemble: g must not alias y");
    const size_t need = mphip_feature_grad_assemble_workspace_bytes(N, C, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("feature_grad_assemble: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    MPHIP_REQUIRE(((uintptr_t)workspace & 15) == 0, "feature_grad_assemble: workspace must be 16-byte aligned");
    const bool vec = W % 4 == 0 && (((uintptr_t)y | (uintptr_t)g | (uintptr_t)(upstream == 1 ? upstream_grad : nullptr)) & 15) == 0;
    const int cw = vec ? 4 : 2;
    FgaArgs a;
    a.H = H, a.W = W, a.Hp = H / 2, a.Wp = W / 2, a.ph = (H + 1) / 2, a.pw = (W + cw - 1) / cw, a.kind = upstream;
    a.items = (unsigned long long)N * C * a.ph * a.pw;
    a.half = half;
    const unsigned blocks = fga_blocks(N, C, H, W, cw);
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(feature_grad_assemble_kernel<4>, dim3(blocks), dim3(256), 0, s, y, upstream_grad, coeff, g, (float *)workspace, a);
    else     hipLaunchKernelGGL(feature_grad_assemble_kernel<2>, dim3(blocks), dim3(256), 0, s, y, upstream_grad, coeff, g, (float *)workspace, a);
    hipLaunchKernelGGL(feature_grad_scale_kernel, dim3(1), dim3(256), 0, s, (const float *)workspace, blocks, scale);
    return check_launch("feature_grad_assemble");
}

extern "C" int mphip_conv2d_stem_bwd_data_supported(int N, int Co, int H, int W) { return stem_bwd_shape_ok(N, Co, H, W) ? 1 : 0; }

extern "C" int mphip_conv2d_stem_bwd_data(const float *dy, const float *w_oihw, float *dx, int N, int Co, int H, int W, void *stream) {
    MPHIP_REQUIRE(dy && w_oihw && dx, "conv2d_stem_bwd_data: null pointer");
    MPHIP_REQUIRE(stem_bwd_shape_ok(N, Co, H, W),
                  "conv2d_stem_bwd_data: unsupported shape N=%d Co=%d H=%d W=%d (Co %% 16 == 0, N, H, W >= 1, fewer than 2^31 elements per tensor)",
                  N, Co, H, W);
    MPHIP_REQUIRE((((uintptr_t)dy | (uintptr_t)w_oihw | (uintptr_t)dx) & 3) == 0, "conv2d_stem_bwd_data: dy, w and dx must be 4-byte aligned");
    MPHIP_REQUIRE(!fl_overlap(dx, (size_t)N * 3 * H * W * sizeof(float), dy, (size_t)N * Co * H * W * sizeof(float)),
                  "conv2d_stem_bwd_data: dx must not alias dy");
    const int tiles_w = cdiv(W, 2 * SB_PW), tiles_h = cdiv(H, 2 * SB_PH);   // (N * tiles <= N * H * W < 2^31: they fit grid.x)
    hipLaunchKernelGGL(conv2d_stem_bwd_data_kernel, dim3((unsigned)((long long)N * tiles_h * tiles_w)), dim3(256), 0, (hipStream_t)stream, dy,
                       w_oihw, dx, Co, H, W, tiles_w, tiles_h);
    return check_launch("conv2d_stem_bwd_data");
}
