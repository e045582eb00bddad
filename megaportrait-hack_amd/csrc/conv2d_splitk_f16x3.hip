// The split-K form of the 2-D 3x3 f16x3 conv (conv2d_f16x3_tile.h, SPLIT = true; plain and with GRP), for the small maps of layer3 and
// layer4 of Emtn's ResNet-18s and of 6DRepNet's RepVGG backbone at B = 1: a 16 x 16-pixel tile leaves those layers 4 to 64 workgroups,
// each walking every K chunk and every packed weight alone.  The reduction over the (Ci / groups) / 16 input-channel chunks is split over
// `splits` workgroups per (tile, channel tile); the weight bytes of a launch do not grow, the workgroup count is multiplied by `splits`.
//
// Two launches, no arrival counters and no floating-point atomics: the bits do not depend on the order workgroups run in.
//   partial   grid (tiles, c2_cots(Co), splits).  Workgroup z runs chunks [z * nchunks / splits, (z + 1) * nchunks / splits) of the K loop
//             (under GRP: of its group's chunks) from accumulators at +0, with the staging, LDS layout, per-chunk MFMA sequence and slab
//             index of the unsplit kernels, and stores its raw fp32 accumulators to part[z][N,Co,H,W], masked at the ragged edge and past
//             Co.  Nothing is unscaled; bias, residual, ReLU and out_range are the finish kernel's.
//   finish    elementwise over N * Co * H * W:  a = part[0];  a = a + part[z] for z = 1 .. splits - 1, in that order;  then the plain
//             epilogue term by term (-ffp-contract=off):  v = (a * 1/scale_w) * 1/scale_x + bias[co]  (unscaled(): two powers of two, one
//             after the other),  v += residual,  ReLU that keeps NaN,  the store.
//             out_range as conv2d_run makes it for every entry: an init launch, then one integer atomicMax per workgroup into
//             min(workgroups, 4096) slots.  A 16-byte path (H * W % 4 == 0 and part, residual, y on 16-byte boundaries) and a scalar one.
// Contract.  Power-of-two scales commute with fp32 rounding away from underflow and overflow, so with one descriptor of x and one header
// scale the launch writes  act(((y_0 + y_1) + ... + y_{splits-1}) + bias (+ residual)),  y_z = mphip_conv2d_fwd of K range z with a zero
// bias, evaluated in fp32 in that order (tests/test_gpu_conv2d_splitk.py).
// fp32 maps, stride 1, one source, three products.  splits == 1 is the plain or the grouped kernel's launch (conv2d_split_launch).
#include "conv2d_f16x3_tile.h"

namespace mphip {

__device__ unsigned long long g_conv2d_split_saturated;

template <bool GRP>
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_split_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                             float *__restrict__ part, size_t part_stride, int Ci, int Co, int H, int W, int tiles_w, int tiles_h, int cig,
                             int cots_per_group) {
    conv2d_k3_tile<false, &g_conv2d_split_saturated, MPHIP_DTYPE_F32, MPHIP_DTYPE_F32, 3, 0, GRP, true>(
        x, x_range, C2CatArgs{}, wslabs, nullptr, nullptr, nullptr, part, nullptr, Ci, Co, H, W, 0, tiles_w, tiles_h, 1u, nullptr, cig,
        cots_per_group, part_stride);
}

constexpr int C2F_NTHR = 256, C2F_PER = 4;   // the finish kernel: elements per thread

__device__ __forceinline__ float c2_finish_one(float a, Unscale u, float b, const float *__restrict__ residual, unsigned i, int relu) {
    float v = unscaled(a, u, b);
    if (residual) v += residual[i];
    if (relu) v = v < 0.0f ? 0.0f : v;   // (keeps NaN, like torch's relu)
    return v;
}

// n = N * Co * HW < 2^31 (the shape rule).  VEC: thread t of workgroup b takes elements 4 * (256 b + t) .. + 3 of one channel (HW % 4 == 0);
// else elements 1024 b + 256 k + t, k < 4.
template <bool VEC>
__global__ void __launch_bounds__(C2F_NTHR)
conv2d_split_finish_kernel(const float *__restrict__ part, size_t part_stride, int splits, const float *__restrict__ x_range,
                           const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                           float *__restrict__ y, float *__restrict__ out_range, unsigned n, unsigned HW, unsigned Co, int relu,
                           unsigned nslots) {
    __shared__ unsigned red[C2F_NTHR / 64];
    float x_scale, x_unscale;
    range_scale_block(x_range, x_scale, x_unscale);   // the descriptor the partial launch staged x with
    const Unscale u = {whdr[0], x_unscale};   // two powers of two, applied one after the other (csrc/mphip_f16x3.h)
    const unsigned tid = threadIdx.x;
    unsigned ymax = 0;
    if constexpr (VEC) {
        const unsigned i = (blockIdx.x * C2F_NTHR + tid) * C2F_PER;
        if (i < n) {
            f32x4 a = *reinterpret_cast<const f32x4 *>(part + i);
            for (int z = 1; z < splits; ++z) {
                const f32x4 p = *reinterpret_cast<const f32x4 *>(part + (size_t)z * part_stride + i);
#pragma unroll
                for (int e = 0; e < C2F_PER; ++e) a[e] = a[e] + p[e];
            }
            const float b = bias[(i / HW) % Co];
            f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
            if (residual) r = *reinterpret_cast<const f32x4 *>(residual + i);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < C2F_PER; ++e) {
                float t = unscaled(a[e], u, b);
                if (residual) t += r[e];
                if (relu) t = t < 0.0f ? 0.0f : t;   // (keeps NaN, like torch's relu)
                v[e] = t;
                ymax = max(ymax, range_bits(t));
            }
            *reinterpret_cast<f32x4 *>(y + i) = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < C2F_PER; ++k) {
            const unsigned i = blockIdx.x * (C2F_NTHR * C2F_PER) + k * C2F_NTHR + tid;
            if (i < n) {
                float a = part[i];
                for (int z = 1; z < splits; ++z) a = a + part[(size_t)z * part_stride + i];
                const float v = c2_finish_one(a, u, bias[(i / HW) % Co], residual, i, relu);
                y[i] = v;
                ymax = max(ymax, range_bits(v));
            }
        }
    }
    if (out_range) {   // workgroup-uniform
        ymax = wave_umax(ymax);
        if ((tid & 63) == 0) red[tid >> 6] = ymax;
        __syncthreads();
        if (tid == 0) {
            const unsigned mx = max(max(red[0], red[1]), max(red[2], red[3]));
            if (mx) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + blockIdx.x % nslots, mx);
        }
    }
}

int conv2d_split_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_split_saturated, count, reset); }

static int c2_split_chunks(int Ci, int groups) { return Ci / groups / C2_KC; }

// splits == 1: the grouped rule (the plain rule at one group).  Else also 2 <= splits <= 16, a divisor of the (Ci / groups) / 16 chunks.
bool c2_split_supported(int N, int Ci, int Co, int H, int W, int groups, int splits) {
    if (!c2_grouped_supported(N, Ci, Co, H, W, groups) || splits < 1 || splits > C2_MAX_SPLITS) return false;
    return c2_split_chunks(Ci, groups) % splits == 0;
}

unsigned c2_split_finish_blocks(size_t ny) { return (unsigned)cdiv(ny, (size_t)(C2F_NTHR * C2F_PER)); }

// grid.z = c.splits; g.part: c.splits maps of N * Co * H * W floats; every range in place, out_range initialised for g.nslots slots
void conv2d_split_launch(const C2Call &c, const C2Grid &g) {
    if (!g.part) return conv2d_grouped_launch(c, g);   // (c.splits == 1)
    float *part = g.part;
    const size_t ny = (size_t)c.N * c.Co * c.H * c.W;
    const _Float16 *slabs = (const _Float16 *)((const char *)c.w_packed + 16);
    const dim3 grid(g.grid.x, g.grid.y, (unsigned)c.splits);
    if (c.groups > 1)
        hipLaunchKernelGGL(conv2d_k3_split_f16x3_kernel<true>, grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range, slabs, part,
                           ny, c.C1, c.Co, c.H, c.W, g.tiles_w, g.tiles_h, c.C1 / c.groups, c.Co / c.groups / C2_COT);
    else
        hipLaunchKernelGGL(conv2d_k3_split_f16x3_kernel<false>, grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range, slabs, part,
                           ny, c.C1, c.Co, c.H, c.W, g.tiles_w, g.tiles_h, 0, 1);
    const unsigned hw = (unsigned)(c.H * c.W);
    const bool vec = hw % C2F_PER == 0 && (((uintptr_t)part | (uintptr_t)c.y | (uintptr_t)c.residual) & 15) == 0;
    const dim3 fgrid(c2_split_finish_blocks(ny));
#define C2F_LAUNCH(VEC)                                                                                                                  \
    hipLaunchKernelGGL(conv2d_split_finish_kernel<VEC>, fgrid, dim3(C2F_NTHR), 0, c.stream, (const float *)part, ny, c.splits, c.x1_range, \
                       (const float *)c.w_packed, c.bias, (const float *)c.residual, (float *)c.y, c.out_range, (unsigned)ny, hw,         \
                       (unsigned)c.Co, c.relu, g.nslots)
    if (vec) C2F_LAUNCH(true);
    else C2F_LAUNCH(false);
#undef C2F_LAUNCH
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_split_supported(int N, int Ci, int Co, int H, int W, int groups, int splits) {
    return c2_split_supported(N, Ci, Co, H, W, groups, splits) ? 1 : 0;
}

// The library's recommendation (1 = do not split): a reduction of fewer than C2_SPLIT_MIN_K chunks (the finish launch costs more than
// the split saves) and a launch of more than C2_SPLIT_MAX_UNSPLIT_WG workgroups (half the CUs have one already) are left whole; else the
// largest power of two S <= C2_SPLIT_MAX_S that divides the chunk count, leaves every workgroup at least C2_SPLIT_MIN_CHUNKS chunks and
// keeps workgroups * S <= C2_SPLIT_MAX_WG.  DESIGN.md section 3.14 has the sweep.
extern "C" int mphip_conv2d_splits(int N, int Ci, int Co, int H, int W, int groups) {
    if (!c2_grouped_supported(N, Ci, Co, H, W, groups)) return 1;
    const int nchunks = c2_split_chunks(Ci, groups);
    if (nchunks < C2_SPLIT_MIN_K) return 1;
    const long long wg = (long long)N * cdiv(H, C2_TH) * cdiv(W, C2_TW) * c2_cots(Co);
    if (wg > C2_SPLIT_MAX_UNSPLIT_WG) return 1;
    for (int s = C2_SPLIT_MAX_S; s >= 2; s >>= 1)
        if (nchunks % s == 0 && nchunks / s >= C2_SPLIT_MIN_CHUNKS && wg * s <= C2_SPLIT_MAX_WG) return s;
    return 1;
}

extern "C" size_t mphip_conv2d_split_workspace_bytes(int N, int Ci, int Co, int H, int W, int groups, int splits) {
    if (!c2_split_supported(N, Ci, Co, H, W, groups, splits)) return 0;
    // the library-computed descriptor of x (x_range == NULL), then the partial maps
    return c2_workspace_bytes(1) + (splits > 1 ? (size_t)splits * N * Co * H * W * sizeof(float) : 0);
}

extern "C" int mphip_conv2d_split_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, const float *residual,
                                      float *y, float *out_range, int N, int Ci, int Co, int H, int W, int groups, int splits, int relu,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    C2Call c = c2_call_f32("conv2d_split_fwd", C2_SPLIT, x, x_range, w_packed, bias, residual, y, out_range, N, Ci, Co, H, W, relu, workspace,
                           workspace_bytes, stream);
    c.groups = groups, c.splits = splits;
    return conv2d_run(c);
}
