// K1/K2/K3 — warp-field composition and the two volumetric warps of the Gbase hot slice.
// HBM-bound kernels: K2 is write-dominated (25 MB out per frame), K3 read-dominated.
// Reference call sites: model.py:965-973/1016-1022 (K1), model.py:1028-1065 (K2),
// model.py:1167-1171 (K3).  Built with -ffp-contract=off: every rounding below is placed where
// ATen's CPU kernels round; the FMAs ATen uses are explicit fmaf().
#include "mphip_ablate.h"
#include "mphip_common.h"
#include "mphip_gn.h"
#include "mphip_resample.h"
#include "mphip_warp.h"

namespace mphip {

// ----------------------------------------------------------------------------------------- K1
// One thread per (b,d,h,w); the three components share the index math.
__global__ void __launch_bounds__(256)
warp_field_compose_kernel(const float *__restrict__ theta, const float *__restrict__ em,
                          const float *__restrict__ base, float *__restrict__ wout, float *__restrict__ rt_out,
                          float *__restrict__ em_out, int B, int eD, int eH, int eW, int G) {
    MPHIP_LATENCY_KERNEL_PRIO();
    const size_t vol = (size_t)G * G * G;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * vol) return;
    int b = (int)(t / vol);
    size_t r = t - (size_t)b * vol;
    int d = (int)(r / ((size_t)G * G));
    int h = (int)((r / G) % G);
    int w = (int)(r % G);
    const float x = base[w], y = base[h], z = base[d];
    const SrcIdx sd = src_index<false>(d, eD, G), sh = src_index<false>(h, eH, G), sw = src_index<false>(w, eW, G);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float *th = theta + ((size_t)b * 3 + j) * 4;
        float acc = x * th[0];
        acc = fmaf(y, th[1], acc);
        acc = fmaf(z, th[2], acc);
        acc = fmaf(1.0f, th[3], acc);
        float e = trilerp(em + ((size_t)b * 3 + j) * eD * eH * eW, eH, eW, sd, sh, sw);
        size_t o = ((size_t)b * 3 + j) * vol + r;
        wout[o] = acc + e;
        if (rt_out) rt_out[o] = acc;
        if (em_out) em_out[o] = e;
    }
}

// ------------------------------------------------------------------------------------ K2 / K3
// Sample coordinate of output voxel (b,d,h,w): the literal op chain of model.py:1036-1058 and
// ATen GridSampler.h:27-36,58-60.  Returns the clipped un-normalised coordinate per axis.
__device__ __forceinline__ float coord_axis(float g, float f, float sz) {
    float p = g + f;         // model.py:1052  grid + warp_field
    float m = 2.0f * p;      // model.py:1058  2.0 * warped_grid
    float q = m / sz;        //                / normalization_factors
    float n = q - 1.0f;      //                - 1.0
    float c = ((n + 1.0f) / 2.0f) * sz;  // grid_sampler_unnormalize, align_corners=True
    return fminf(sz, fmaxf(c, 0.0f));    // clip_coordinates (padding_mode='border')
}

__device__ __forceinline__ Coord3 sample_coord(const float *__restrict__ field, const float *__restrict__ lin_d,
                                               const float *__restrict__ lin_h, const float *__restrict__ lin_w,
                                               int b, int d, int h, int w, int D, int H, int W, int fD, int fH,
                                               int fW) {
    const SrcIdx sd = src_index<true>(d, fD, D), sh = src_index<true>(h, fH, H), sw = src_index<true>(w, fW, W);
    const size_t fvol = (size_t)fD * fH * fW;
    const float *fb = field + (size_t)b * 3 * fvol;
    Coord3 c;
    c.x = coord_axis(lin_w[w], trilerp(fb, fH, fW, sd, sh, sw), (float)(W - 1));
    c.y = coord_axis(lin_h[h], trilerp(fb + fvol, fH, fW, sd, sh, sw), (float)(H - 1));
    c.z = coord_axis(lin_d[d], trilerp(fb + 2 * fvol, fH, fW, sd, sh, sw), (float)(D - 1));
    return c;
}

// K1 + the coordinate pass in one kernel (r03): the warp field [B,3,G,G,G] a generator composes is read exactly once, by the
// coordinate pass of the warp it feeds, which only needs the 2 x D of its G depth planes the align_corners=True resize touches.
// One thread per (b,d,h,w) of the (D,G,G) volume evaluates warp_field_compose_kernel's expression at the two source planes and
// warp_coords_kernel<INPLANE>'s chain on them — the same operations in the same order: bit-identical coordinates, without the
// 2 x 25 MB round trip and one launch less on the latency-bound chain.
__device__ __forceinline__ float compose_value(const float *__restrict__ th /* theta[b][j] */, const float *__restrict__ emj, float x, float y,
                                               float z, int eH, int eW, const SrcIdx &sd, const SrcIdx &sh, const SrcIdx &sw) {
    float acc = x * th[0];
    acc = fmaf(y, th[1], acc);
    acc = fmaf(z, th[2], acc);
    acc = fmaf(1.0f, th[3], acc);
    return acc + trilerp(emj, eH, eW, sd, sh, sw);
}

__global__ void __launch_bounds__(256)
warp_field_coords_kernel(const float *__restrict__ theta, const float *__restrict__ em, const float *__restrict__ base,
                         const float *__restrict__ lin_d, const float *__restrict__ lin_h, const float *__restrict__ lin_w,
                         float *__restrict__ coords, int B, int eD, int eH, int eW, int G, int D) {
    MPHIP_LATENCY_KERNEL_PRIO();
    const size_t n = (size_t)B * D * G * G;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int w = (int)(t % G);
    size_t r = t / G;
    const int h = (int)(r % G);
    r /= G;
    const int d = (int)(r % D);
    const int b = (int)(r / D);
    const SrcIdx sd = src_index<true>(d, G, D);   // the field's depth planes this output slice blends (warp_coords_kernel<true>)
    const float x = base[w], y = base[h];
    const SrcIdx eh = src_index<false>(h, eH, G), ew = src_index<false>(w, eW, G);
    const SrcIdx e0 = src_index<false>(sd.i0, eD, G), e1 = src_index<false>(sd.i1, eD, G);
    const float z0 = base[sd.i0], z1 = base[sd.i1];
    float f[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float *th = theta + ((size_t)b * 3 + j) * 4;
        const float *emj = em + ((size_t)b * 3 + j) * eD * eH * eW;
        const float f0 = compose_value(th, emj, x, y, z0, eH, eW, e0, eh, ew);
        const float f1 = compose_value(th, emj, x, y, z1, eH, eW, e1, eh, ew);
        f[j] = lerp2(sd.l0, f0, sd.l1, f1);
    }
    coords[t * 3] = coord_axis(lin_w[w], f[0], (float)(G - 1));
    coords[t * 3 + 1] = coord_axis(lin_h[h], f[1], (float)(G - 1));
    coords[t * 3 + 2] = coord_axis(lin_d[d], f[2], (float)(D - 1));
}

// ---- coordinate pass -------------------------------------------------------------------------
// One thread per output voxel: coords[B,D,H,W,3] = clipped (x,y,z) sample coordinates (and the
// floor indices for the tests).  12 B per voxel (0.79 MB per 512^2 frame, 3 % of K2's traffic);
// K2/K3 read it back instead of re-deriving the chain per channel slice.
// INPLANE: fH==H && fW==W -> the align_corners=True resize is the identity in H,W (weights exactly
// (1,0)), so only the depth lerp remains — bitwise the same value as the full 8-corner form.
template <bool INPLANE>
__global__ void __launch_bounds__(256)
warp_coords_kernel(const float *__restrict__ field, const float *__restrict__ lin_d, const float *__restrict__ lin_h,
                   const float *__restrict__ lin_w, float *__restrict__ coords, int32_t *__restrict__ idx, int B,
                   int D, int H, int W, int fD, int fH, int fW) {
    const size_t n = (size_t)B * D * H * W;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int w = (int)(t % W);
    size_t r = t / W;
    int h = (int)(r % H);
    r /= H;
    int d = (int)(r % D);
    int b = (int)(r / D);
    Coord3 c;
    if (INPLANE) {
        const SrcIdx sd = src_index<true>(d, fD, D);
        const size_t fvol = (size_t)fD * fH * fW;
        const float *f0 = field + (size_t)b * 3 * fvol + ((size_t)sd.i0 * fH + h) * fW + w;
        const float *f1 = field + (size_t)b * 3 * fvol + ((size_t)sd.i1 * fH + h) * fW + w;
        c.x = coord_axis(lin_w[w], lerp2(sd.l0, f0[0], sd.l1, f1[0]), (float)(W - 1));
        c.y = coord_axis(lin_h[h], lerp2(sd.l0, f0[fvol], sd.l1, f1[fvol]), (float)(H - 1));
        c.z = coord_axis(lin_d[d], lerp2(sd.l0, f0[2 * fvol], sd.l1, f1[2 * fvol]), (float)(D - 1));
    } else {
        c = sample_coord(field, lin_d, lin_h, lin_w, b, d, h, w, D, H, W, fD, fH, fW);
    }
    coords[t * 3] = c.x;
    coords[t * 3 + 1] = c.y;
    coords[t * 3 + 2] = c.z;
    if (idx) {
        idx[t * 3] = (int)floorf(c.x);
        idx[t * 3 + 1] = (int)floorf(c.y);
        idx[t * 3 + 2] = (int)floorf(c.z);
    }
}

// ---- gather pass -----------------------------------------------------------------------------
// The source voxels a tile of output voxels needs form a small box when the warp is smooth (the
// reference's own fields move samples by a few voxels: SURVEY.md §0 quirk 1).  Each workgroup
// finds that bounding box with a wavefront-shuffle + LDS min/max reduction, stages the box for a
// slice of channels into LDS with coalesced row reads, and does the 8-tap trilinear gather from
// LDS (neighbouring lanes hit the same or adjacent words: broadcast, no bank conflicts).  A box
// that does not fit (wild fields) falls back to gathering from global memory.
constexpr int STAGE_FLOATS = 12288;  // 48 KB of LDS for the staged box

__device__ __forceinline__ float gather8_lds(const float *__restrict__ img, const TapOff &o, const float (&w)[8]) {
    const float *p = img + o.base;
    float acc = 0.0f;
    acc += p[0] * w[0];
    acc += p[o.dx] * w[1];
    acc += p[o.dy] * w[2];
    acc += p[o.dy + o.dx] * w[3];
    acc += p[o.dz] * w[4];
    acc += p[o.dz + o.dx] * w[5];
    acc += p[o.dz + o.dy] * w[6];
    acc += p[o.dz + o.dy + o.dx] * w[7];
    return acc;
}

// Four channels per tap with one ds_read_b128 each (LDS image [voxel][channel], 16-byte aligned pitch): every
// channel sees exactly the scalar op sequence of gather8 (acc=0; acc += p*w in tap order), so values stay
// bit-identical, at a quarter of the LDS instructions.
__device__ __forceinline__ void gather8x4(const float *__restrict__ img, const TapOff &t, const float (&tw)[8],
                                          float out[4]) {
    const float *p = img + t.base;
    const float4 q0 = *reinterpret_cast<const float4 *>(p);
    const float4 q1 = *reinterpret_cast<const float4 *>(p + t.dx);
    const float4 q2 = *reinterpret_cast<const float4 *>(p + t.dy);
    const float4 q3 = *reinterpret_cast<const float4 *>(p + t.dy + t.dx);
    const float4 q4 = *reinterpret_cast<const float4 *>(p + t.dz);
    const float4 q5 = *reinterpret_cast<const float4 *>(p + t.dz + t.dx);
    const float4 q6 = *reinterpret_cast<const float4 *>(p + t.dz + t.dy);
    const float4 q7 = *reinterpret_cast<const float4 *>(p + t.dz + t.dy + t.dx);
    // channel pairs on the packed fp32 pipe (v_pk_mul_f32 / v_pk_add_f32: per channel still acc = 0; acc += q_k * w_k in tap order,
    // one rounding per op — the same bits as the scalar sequence at half the instructions; K3 on the reference's fields 52.7 -> 48.4 us, r04)
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    const float4 q[8] = {q0, q1, q2, q3, q4, q5, q6, q7};
    f32x2_ lo = {0.0f, 0.0f}, hi = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const f32x2_ wk = {tw[k], tw[k]};
        lo += f32x2_{q[k].x, q[k].y} * wk;
        hi += f32x2_{q[k].z, q[k].w} * wk;
    }
    out[0] = lo[0]; out[1] = lo[1]; out[2] = hi[0]; out[3] = hi[1];
}

// channel pitch of the staged image: a multiple of 4 floats (16-byte tap reads) whose quarter is odd, so lanes
// that read different voxels fall on different 16-byte bank slots
__device__ __forceinline__ int lds_pitch_for(int channels) {
    int p = (channels + 3) & ~3;
    if (((p >> 2) & 1) == 0) p += 4;
    return p;
}

// K2, tiles whose samples all lie in the volume's LOW CORNER — every tile of the reference's own fields (apply_warping_field hands
// grid_sample coordinates of size ~[-2, 3] as if they were voxel indices).  Any other tile — a field that really
// travels through the volume — is only MARKED here (todo[tile]) and done by warp_gather_columns_kernel / warp_gather_direct_kernel
// below: keeping those paths out of this kernel keeps it lean.
//
// How it got its shape (r04; wall-clock stamps per workgroup, tools/dbg_k2_trace.py, and ablations, tools/k2_ablate.sh, B=8):
//   * r03 (32 x 32 tile, four positions per thread, every workgroup staging its own source box line by line from global memory —
//     1.5 k scattered 128-byte lines, the rows of all 96 planes on the same few L2 channels): 63 us.  Not the stores: without them
//     59 us.  Not the tap arithmetic either: half the VALU instructions (packed fp32), no address arithmetic in the loop, half the
//     dependent chain per wave at four waves per SIMD — each +-0.  The stamps: the gather LOOPS wrote at ~7.7 TB/s, the speed of a
//     plain fill of the same 201 MB, but covered less than half of a workgroup's life; in front of them sat three dependent
//     round trips (coordinates -> box -> staging loads), and a tail of workgroups whose staging loads queued behind the store flood
//     of the others ended at 60 us when the median had ended at 34.
//   * So the corner [0,E)^3 of every frame is copied ONCE per call (warp_corner_image_kernel; the hot slice does it at the start of
//     its step, vs is an input) into a compact image that already has the LDS layout, [frame][channel group][cell][channels + pad],
//     contiguous — all L2 channels serve it — and a workgroup brings its block in by LDS-DMA, issued FIRST THING: it lands under
//     the coordinate loads and the box reduction.  One global round trip in front of the stores instead of three.
//   * More, smaller workgroups (3072 of 256 threads, three resident rounds) gave 50 us: every workgroup pays the coordinate round
//     trip (3.7 us) before it stores for 7 us.  One workgroup per CU and launch does better: 1024 threads own a 32 x 64 tile of one
//     (b,d) plane, two positions per thread, ALL channels (image: 6^3 cells x 98 floats = 85 KB), one prologue, then nothing but
//     tap reads and stores.  Few tiles (B = 1, 2): the channels are split over blockIdx.y so that every CU has work.
//   * The image is [cell][channel], channel pitch = channels + 2 (98): a tap's (c, c+1) pair is ONE 8-byte-aligned ds_read_b64 whose
//     channel is an immediate offset (no address arithmetic in the loop), and lanes that read different cells fall on different
//     bank pairs.  What bounds the loop now is its arithmetic — 16 fp32 multiplies / adds per output value, kept as separate,
//     separately rounded ops for ATen's bits: 20 us of the chip's fp32 pipe at B=8, 34 us with addressing and stores; the packed ops
//     (v_pk_mul_f32 / v_pk_add_f32, half the instructions) measured the same time as scalar ones.
// Values: per channel and position exactly gather8's op sequence (acc = 0; acc += p_k * w_k in tap order, one rounding per op).
constexpr int K2_TH = 32, K2_TW = 64;      // 2048 positions per workgroup, two per thread
constexpr int K2_THREADS = 1024;
constexpr int K2_DIRECT_SPLIT = 4;         // channel groups of the direct gather (warp_gather_direct_body)
constexpr int K2_COLUMNS_MAX_BOX = 16384;  // source-box voxels of a tile up to which the column walk is used
constexpr int K2_CORNER_E = 6;
constexpr int K2_CORNER_CELLS = K2_CORNER_E * K2_CORNER_E * K2_CORNER_E;
constexpr int K2_CG_MAX = 96;              // channels per workgroup at most (LDS: 216 x 98 floats = 84672 B)
constexpr int K2_LDS_FLOATS = K2_CORNER_CELLS * (K2_CG_MAX + 2);
// channels per workgroup (blockIdx.y groups): all of them (<= 96) when the tiles alone fill the chip, else 32 or 16
__host__ __device__ inline int k2_group_channels(size_t tiles, int C) {
    int cg = min(C, K2_CG_MAX);
    if (tiles * (size_t)((C + cg - 1) / cg) < 256 && C > 32) cg = 32;
    if (tiles * (size_t)((C + cg - 1) / cg) < 256 && C > 16) cg = 16;
    return cg;
}
// channel pitch of the image: EVEN (a tap's channel pair is one 8-byte-aligned ds_read_b64: 256 B/clk, twice ds_read2_b32) and = 2 mod 32
// for the channel counts in use (98, 34, 18 -> cell * pitch mod 64 takes 32 different even values: the 32 lanes of a read group that
// hit different cells fall on different bank pairs)
__host__ __device__ inline int k2_pitch(int cg) { return ((cg + 1) & ~1) + 2; }
// image: [frame][group][cell][k2_pitch(cg)] floats, a group's block padded to a multiple of 16 bytes
__host__ __device__ inline size_t k2_block_floats(int cg) { return ((size_t)K2_CORNER_CELLS * k2_pitch(cg) + 3) / 4 * 4; }
// DT: the volume's dtype (model dtypes, include/mphip.h), widened on load: the image is fp32 whatever the source.  A typed K2 always has
// the image: warp_gather_kernel<DT != F32> reads the corner from it and nowhere else.
template <int DT>
__global__ void __launch_bounds__(128)
warp_corner_image_kernel(const dtype_t<DT> *__restrict__ v, float *__restrict__ img, int C, int D, int H, int W, int cg, int groups) {
    const int cell = blockIdx.x, b = blockIdx.y;
    const int z = cell / (K2_CORNER_E * K2_CORNER_E), y = (cell / K2_CORNER_E) % K2_CORNER_E, x = cell % K2_CORNER_E;
    const bool inside = z < D && y < H && x < W;
    const size_t vol = (size_t)D * H * W, blk = k2_block_floats(cg);
    const int cgp = k2_pitch(cg);
    for (int c = threadIdx.x; c < groups * cgp; c += 128) {   // (the pad slot and channels >= C: zeros, the block is copied whole)
        const int g = c / cgp, cl = c - g * cgp, ch = g * cg + cl;
        const bool real = inside && cl < cg && ch < C;
        img[((size_t)b * groups + g) * blk + (size_t)cell * cgp + cl] = real ? widen(v[((size_t)b * C + ch) * vol + ((size_t)z * H + y) * W + x]) : 0.0f;
    }
}
// one block of the corner image -> LDS, as LDS-DMA (16 bytes per lane, 1 KiB per wave and instruction, no registers); issued by hand:
// the compiler would wait for each transfer before the next LDS access.  The caller waits (vmcnt(0)) before its barrier.
template <int THREADS>
__device__ __forceinline__ void k2_dma_image(const float *__restrict__ blk, float *lds, int floats) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)lds;
    const int pieces = (floats + 255) / 256;
    for (int q = wave; q < pieces; q += THREADS / 64) {
        const int f = q * 256 + lane * 4;   // float index of this lane's 16 bytes
        if (f < floats) {
            const float *src = blk + f;
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds0 + (unsigned)q * 1024u) : "memory");
        }
    }
}
// ... and without an image (a caller whose workspace has no room for it): the workgroup collects its block itself
__device__ __forceinline__ void k2_stage_corner(const float *__restrict__ vb, float *lds, int c0, int cs, int cgp, int D, int H, int W) {
    const size_t vol = (size_t)D * H * W;
    for (int i = threadIdx.x; i < K2_CORNER_CELLS * cs; i += K2_THREADS) {
        const int c = i / K2_CORNER_CELLS, cell = i - c * K2_CORNER_CELLS;   // lanes along cells: neighbours share lines
        const int z = cell / (K2_CORNER_E * K2_CORNER_E), y = (cell / K2_CORNER_E) % K2_CORNER_E, x = cell % K2_CORNER_E;
        lds[cell * cgp + c] = (z < D && y < H && x < W) ? vb[(size_t)(c0 + c) * vol + ((size_t)z * H + y) * W + x] : 0.0f;
    }
}

// (the tap arithmetic itself — packed fp32, two channels per instruction — is k2_tap_pairs, mphip_warp.h)
#ifdef MPHIP_K2_TRACE   /* dev: wall-clock (100 MHz) stamps per workgroup: start, box known, image staged, done */
__device__ unsigned long long g_k2_trace[4096 * 4];
#define K2_STAMP(i) if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < 4096) g_k2_trace[(blockIdx.y * gridDim.x + blockIdx.x) * 4 + (i)] = wall_clock64();
#else
#define K2_STAMP(i)
#endif
// DT: the source volume's dtype (model dtypes).  A typed source is never read here: the fp32 image of its corner (warp_corner_image_kernel<DT>)
// is required instead.
template <int DT>
__global__ void __launch_bounds__(K2_THREADS)
warp_gather_kernel(const dtype_t<DT> *__restrict__ v, const float *__restrict__ coords, float *__restrict__ out,
                   float *__restrict__ out_range /* optional range descriptor of `out`: G3d's first conv reads it */,
                   int *__restrict__ todo, int B, int C, int D, int H, int W,
                   const float *__restrict__ img /* optional corner image (warp_corner_image_kernel, same cg) */, int cg /* channels per blockIdx.y */) {
    constexpr bool TYPED = DT != MPHIP_DTYPE_F32;
    if (TYPED && img == nullptr) return;   // (the host refuses a typed K2 without the image)
    __shared__ __attribute__((aligned(16))) float lds[K2_LDS_FLOATS];
    __shared__ int red[(K2_THREADS / 64) * 6];
    K2_STAMP(0)
    const int HW = H * W;
    const int tiles_w = (W + K2_TW - 1) / K2_TW, tiles_h = (H + K2_TH - 1) / K2_TH;
    // XCD-aware order: consecutive logical ids (d fastest, then tile, then frame) run on the same XCD
    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int d = (int)(bid % (unsigned)D);
    const int tile = (int)((bid / (unsigned)D) % (unsigned)(tiles_w * tiles_h));
    const int b = (int)(bid / ((unsigned)D * (unsigned)(tiles_w * tiles_h)));
    const int cg0 = (int)blockIdx.y * cg, Cg = min(C - cg0, cg), cgp = k2_pitch(cg);
    const int h = (tile / tiles_w) * K2_TH + (int)(threadIdx.x / (K2_TW / 2));
    const int w = (tile % tiles_w) * K2_TW + (int)(threadIdx.x % (K2_TW / 2)) * 2;
    const bool active = h < H && w < W;  // W % 4 == 0 -> a thread's 2 positions share validity
    const int p0 = h * W + w;
    const size_t vol = (size_t)D * HW;

    Taps taps[2];
    int x0[2], y0[2], z0[2];
    int lx = INT_MAX, ly = INT_MAX, lz = INT_MAX, hx = 0, hy = 0, hz = 0;
    float cf[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (active) {   // (issued BEFORE the scalar test below is waited for: one round trip for both)
        const float *cp = coords + (((size_t)b * D + d) * HW + p0) * 3;   // (p0 even: 8-byte aligned)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float2 t2 = *reinterpret_cast<const float2 *>(cp + q * 2);
            cf[q * 2] = t2.x; cf[q * 2 + 1] = t2.y;
        }
    }
    // The image is fetched only if the tile's FIRST sample lies in the corner (one scalar load): a field that travels through the volume
    // (not the reference's) would otherwise pay for the transfers for nothing.
    // TYPED: always.  The typed kernel has no fp32 volume to stage from, so it brings the image in for EVERY tile: a tile whose clamped box
    // lies in the corner although its first sample does not (an axis of 6 voxels whose samples clip to its far border) finds its data in
    // LDS too.
    const float *c0p = coords + (((size_t)b * D + d) * HW + (size_t)(tile / tiles_w) * K2_TH * W + (tile % tiles_w) * K2_TW) * 3;
    const float fx = c0p[0], fy = c0p[1], fz = c0p[2];
    const bool maybe = TYPED || (fx >= 0.0f && fx < (float)(K2_CORNER_E - 1) && fy >= 0.0f && fy < (float)(K2_CORNER_E - 1) && fz >= 0.0f && fz < (float)(K2_CORNER_E - 1));
    const bool dma = maybe && img != nullptr;
#ifndef MPHIP_K2_ABL_NOSTAGE   /* dev ablations (timing only, wrong results): tools/k2_ablate.sh */
    if (dma) k2_dma_image<K2_THREADS>(img + ((size_t)b * gridDim.y + blockIdx.y) * k2_block_floats(cg), lds, (int)k2_block_floats(cg));
#endif
    if (active) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            Coord3 c{cf[i * 3], cf[i * 3 + 1], cf[i * 3 + 2]};
            taps[i] = make_taps(c, D, H, W);
            x0[i] = (int)floorf(c.x); y0[i] = (int)floorf(c.y); z0[i] = (int)floorf(c.z);
            lx = min(lx, x0[i]); ly = min(ly, y0[i]); lz = min(lz, z0[i]);
            hx = max(hx, x0[i]); hy = max(hy, y0[i]); hz = max(hz, z0[i]);
        }
    }
    const Box bx = block_box_n<K2_THREADS / 64>(lx, ly, lz, hx, hy, hz, D, H, W, red);
    K2_STAMP(1)
    // block-uniform: every sample of the tile (all eight corners of each) inside the corner the image holds
    const bool in_corner = bx.ox + bx.ex <= K2_CORNER_E && bx.oy + bx.ey <= K2_CORNER_E && bx.oz + bx.ez <= K2_CORNER_E;
    // 0: done here; 1: a box of moderate size = a smooth field that travels -> warp_gather_columns_kernel (plane reuse down the
    // slices); 2: no locality to exploit (a box like the whole volume) -> warp_gather_direct_kernel (most loads in flight)
    if (threadIdx.x == 0 && blockIdx.y == 0) todo[bid] = in_corner ? 0 : (bx.ex * bx.ey * bx.ez <= K2_COLUMNS_MAX_BOX ? 1 : 2);
    unsigned mbits = 0;
    if (dma) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the image have landed
    if (in_corner) {
        float *ob = out + (size_t)b * C * vol + (size_t)d * HW + p0;
#ifndef MPHIP_K2_ABL_NOSTAGE
        if constexpr (!TYPED) {   // (a typed kernel never reads `v`: with the image, `dma` always holds)
            if (!dma) k2_stage_corner(v + (size_t)b * C * vol, lds, cg0, Cg, cgp, D, H, W);
        }
#endif
        __syncthreads();
        K2_STAMP(2)
        if (active) {
            int tb[2][8];   // tap addresses in the image (floats, premultiplied by the pitch)
            const Box cbx{0, 0, 0, K2_CORNER_E, K2_CORNER_E, K2_CORNER_E};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const TapOff o = rebase(taps[i], x0[i], y0[i], z0[i], cbx, cgp);
                tb[i][0] = o.base; tb[i][1] = o.base + o.dx; tb[i][2] = o.base + o.dy; tb[i][3] = o.base + o.dy + o.dx;
                tb[i][4] = o.base + o.dz; tb[i][5] = o.base + o.dz + o.dx; tb[i][6] = o.base + o.dz + o.dy;
                tb[i][7] = o.base + o.dz + o.dy + o.dx;
            }
            k2_f2 wp[2][4];   // the taps' weights in pairs
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) wp[i][j] = k2_f2{taps[i].w[2 * j], taps[i].w[2 * j + 1]};
            auto two_channels = [&](const float *src, int c) {
                k2_f2 acc[2];
                k2_tap_pairs<2>(src, tb, wp, acc);
#ifdef MPHIP_K2_ABL_NOSTORE
                if (acc[0][0] == 1.2345e30f)
#endif
                {
                    *reinterpret_cast<float2 *>(ob + (size_t)(cg0 + c) * vol) = make_float2(acc[0][0], acc[1][0]);
                    *reinterpret_cast<float2 *>(ob + (size_t)(cg0 + c + 1) * vol) = make_float2(acc[0][1], acc[1][1]);
                }
                mbits = max(max(mbits, range_bits(acc[0][0])), max(range_bits(acc[0][1]), max(range_bits(acc[1][0]), range_bits(acc[1][1]))));
                __builtin_amdgcn_sched_barrier(0);   // one channel pair at a time (hoisting the next pairs' reads spills)
            };
            int c = 0;
#ifndef MPHIP_K2_ABL_NOLOOP
            for (; c + 8 <= Cg; c += 8) {   // (eight channels per trip: their offsets are immediates of the tap reads)
                const float *src = lds + c;
#pragma unroll
                for (int u = 0; u < 8; u += 2) two_channels(src + u, c + u);
            }
            for (; c + 2 <= Cg; c += 2) two_channels(lds + c, c);
            if (c < Cg) {   // odd tail
                float r[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    r[i] = 0.0f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) r[i] += lds[c + tb[i][k]] * taps[i].w[k];
                }
                *reinterpret_cast<float2 *>(ob + (size_t)(cg0 + c) * vol) = make_float2(r[0], r[1]);
                mbits = max(mbits, max(range_bits(r[0]), range_bits(r[1])));
            }
#endif
        }
    }
    // (slot = group * tiles + tile: the follow-up kernels fold into group 0's slots)
    if (out_range) range_note_block(mbits, out_range, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    K2_STAMP(3)
}

// GroupNorm apply + residual + ReLU + AvgPool3d(2) of the block K2's output enters (G3d's first ResBlock3D, identity shortcut), with the
// residual REBUILT instead of fetched: the residual is K2's output, and wherever K2 served a tile from the corner image (todo == 0: every
// tile of the reference's own fields) each of its values is k2_tap_reads + k2_tap_chain on 85 KB that are still in the workspace.  gn_apply_pool_kernel<2>
// streams conv2's output AND the residual (2 x 201 MB at B = 8) to write 25 MB; this kernel streams conv2's output only and does the tap
// arithmetic K2 did (20 us of the chip's fp32 pipe) underneath.
// Organised like K2: a thread owns positions and walks the channels, so a sample's taps are built once.  A workgroup of 512 threads takes a
// 32 x 64 (h, w) tile of one frame and the slice PAIR (2 od, 2 od + 1), in two passes of 16 rows; per pass a thread holds four samples — two
// along w (its own pooling pair), times the two slices.  The h-partner of a cell is the other half of the wave (lanes 0-31: an even row,
// lanes 32-63: the row below): per channel pair (c, c+1) one v_permlane32_swap per value hands the lower half all eight values of channel c
// and the upper half those of c+1, which each adds in gn_apply_pool_kernel's order (d outer, then h, then w, from 0.0f, then / 8.0f) and
// stores: 128 contiguous bytes per half wave.  blockIdx.y = (K2's channel group, i.e. block of the image) x csub parts of it: few tiles ->
// more parts, so that the chip has a workgroup per CU.
// A pair with a slice K2 did NOT serve from the corner (travelling fields) loads the residual from p.residual, as the plain kernel does.
// Values: gn_value on the bits K2 stored (same make_taps / rebase / k2_tap_reads / k2_tap_chain), summed in that order: bitwise gn_apply_pool_kernel.
// Schedule: nothing in the channel walk waits for memory it has just asked for — the channels' parameters sit in LDS, a pair's
// tap reads go out a pair ahead of their chain, conv2's output a trip ahead.
constexpr int GPW_THREADS = 512;
constexpr int GPW_ROWS = GPW_THREADS / (K2_TW / 2);   // rows of the tile per pass
constexpr int GPW_TRIP = 8;                              // channels per trip of the walk (their offsets: immediates of the tap reads)
static_assert(K2_TH % GPW_ROWS == 0 && GPW_ROWS % 2 == 0, "whole passes of row pairs");
__global__ void __launch_bounds__(GPW_THREADS)
gn_apply_pool_warp_kernel(GnParams p, const float *__restrict__ coords, const int *__restrict__ todo, const float *__restrict__ img, int D, int H,
                          int W, int cg /* channels per block of the image (K2's) */, int csub /* workgroups per block */) {
    __shared__ __attribute__((aligned(16))) float lds[K2_LDS_FLOATS];
    __shared__ float4 chn[K2_CG_MAX];   // (mean, rstd, gamma, beta) of this workgroup's channels
    const int C = p.C, HW = H * W, oD = D / 2, oH = H / 2, oW = W / 2;
    const int tiles_w = (W + K2_TW - 1) / K2_TW, tiles = tiles_w * ((H + K2_TH - 1) / K2_TH);
    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);   // (slice pair fastest, then tile, then frame: K2's order)
    const int od = (int)(bid % (unsigned)oD);
    const int tile = (int)((bid / (unsigned)oD) % (unsigned)tiles);
    const int b = (int)(bid / ((unsigned)oD * (unsigned)tiles));
    const int grp = (int)blockIdx.y / csub, sub = (int)blockIdx.y % csub, groups = (int)gridDim.y / csub;
    const int cg0 = grp * cg, Cg = min(C - cg0, cg), cgp = k2_pitch(cg);
    const int cs = ((Cg / GPW_TRIP + csub - 1) / csub) * GPW_TRIP;   // channels per part: whole trips (C % GPW_TRIP == 0)
    const int c_lo = sub * cs, c_hi = min(Cg, c_lo + cs);           // this workgroup's channels of the block
    const size_t vol = (size_t)D * HW;
    const int *mk = todo + ((size_t)b * tiles + tile) * D + 2 * od;   // K2's marks of the two slices
    const bool rebuild = mk[0] == 0 && mk[1] == 0;                     // block-uniform
    const int row = (int)(threadIdx.x / (K2_TW / 2));
    const int h0 = (tile / tiles_w) * K2_TH + row;
    const int w = (tile % tiles_w) * K2_TW + (int)(threadIdx.x % (K2_TW / 2)) * 2;
    // a pass's coordinates: 2 slices x (x, y, z) of 2 positions; the first pass's are asked for ahead of the image, the second's ahead of the
    // first's channel walk: one round trip in front of the stream
    auto load_coords = [&](int h, float (&cf)[2][6]) {
        if (h < H && w < W) {   // W % 4 == 0 -> a thread's 2 positions share validity
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float *cp = coords + (((size_t)b * D + 2 * od + s) * HW + h * W + w) * 3;   // (w even: 8-byte aligned)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float2 t2 = *reinterpret_cast<const float2 *>(cp + q * 2);
                    cf[s][q * 2] = t2.x; cf[s][q * 2 + 1] = t2.y;
                }
            }
        }
    };
    float cf[2][6] = {}, cfn[2][6] = {};
    if (rebuild) load_coords(h0, cf);
    if ((int)threadIdx.x < c_hi - c_lo) {   // (the channel walk reads these from LDS: a load from memory in it would wait for the whole stream)
        const int c = cg0 + c_lo + (int)threadIdx.x, gi = b * (C / p.cpg) + c / p.cpg;
        chn[threadIdx.x] = make_float4(p.stats[gi * 2], p.stats[gi * 2 + 1], p.gamma[c], p.beta[c]);
    }
    if (rebuild) {
        k2_dma_image<GPW_THREADS>(img + ((size_t)b * groups + grp) * k2_block_floats(cg), lds, (int)k2_block_floats(cg));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the image have landed
    }
    __syncthreads();
    // what the block asks of gn_value, as constants: no second affine, residual, ReLU, no tanh (the launcher passes nothing else)
    GnParams q = p;
    q.relu = 1;
    q.tanh_ = 0;
    const int half = (int)(threadIdx.x & 63) >> 5;   // 0: even row, channel c of a pair; 1: odd row, channel c + 1
    unsigned mbits = 0;
    // one pass: GPW_ROWS rows of the tile.  RB: the residual is rebuilt (else loaded); a compile-time copy of `rebuild`, so that the walk
    // has no branch in it (the compiler counts the loads in flight only within straight-line code)
    auto pass = [&](auto RB, int h) {
        constexpr bool REBUILD = decltype(RB)::value;
        int tb[2][2][8];      // [slice][position]: tap addresses in the image
        k2_f2 wp[2][2][4];    // ... and weights in pairs
        if constexpr (REBUILD) {
            const Box cbx{0, 0, 0, K2_CORNER_E, K2_CORNER_E, K2_CORNER_E};
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const Coord3 c{cf[s][i * 3], cf[s][i * 3 + 1], cf[s][i * 3 + 2]};
                    const Taps t = make_taps(c, D, H, W);
                    k2_tap_setup(rebase(t, (int)floorf(c.x), (int)floorf(c.y), (int)floorf(c.z), cbx, cgp), t, tb[s][i], wp[s][i]);
                }
        }
        // addresses: a workgroup-uniform base (frame, slice 2 od, channel 0) + the thread's byte offset in the plane, 32 bits (vol < 2^30) —
        // one register per thread for all the loads, not a 64-bit pointer each
        const size_t in0 = (size_t)b * C * vol + (size_t)(2 * od) * HW;
        const float *xb = p.x + in0, *rb = p.residual + in0;
        const unsigned toff = (unsigned)(h * W + w) * 4u;
        float *ob = p.y + ((size_t)b * C * oD + od) * (oH * oW);
        const unsigned ooff = (unsigned)(half * oD * (oH * oW) + (h / 2) * oW + w / 2) * 4u;   // (lanes 32-63 store the pair's second channel)
        // conv2's output (and a residual that is loaded) of a channel pair: two slices x two positions each; asked for a trip ahead, into
        // the registers the pair before it in the same place of the trip has just left
        auto load_pair = [&](const float *src, int c, float2 (&yv)[GPW_TRIP][2], int u) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    yv[u + k][s] = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(src + (size_t)(cg0 + c + k) * vol + s * HW) + toff);
        };
        // the tap values of a channel pair, per slice: read a pair ahead of their chain (two waves per SIMD do not hide an LDS round trip
        // per four taps).  The walk's last pair asks for the pair behind its channels: the next part's, or the pitch's two pad floats.
        k2_f2 pv0[2][8], pv1[2][8];
        if constexpr (REBUILD) {
            k2_tap_reads<2>(lds + c_lo, tb[0], pv0);
            k2_tap_reads<2>(lds + c_lo, tb[1], pv1);
        }
        auto do_trip = [&](int cl, int cn, float2 (&yv)[GPW_TRIP][2], float2 (&rv)[GPW_TRIP][2]) {
            const float *src = lds + cl;   // (the pair's offset in the trip: an immediate of the tap reads)
#pragma unroll
            for (int u = 0; u < GPW_TRIP; u += 2) {
                k2_f2 res[2][2];   // [slice][position] = residual of channels (u, u + 1) of the trip
                // (asked for ahead of the next pair's tap reads: LDS answers in order, behind them it would wait for all of them)
                const float4 n2[2] = {chn[cl - c_lo + u], chn[cl - c_lo + u + 1]};
                if constexpr (REBUILD) {
                    k2_tap_chain<2>(pv0, wp[0], res[0]);
                    k2_tap_reads<2>(src + u + 2, tb[0], pv0);
                    __builtin_amdgcn_sched_barrier(0);
                    k2_tap_chain<2>(pv1, wp[1], res[1]);
                    k2_tap_reads<2>(src + u + 2, tb[1], pv1);
                    __builtin_amdgcn_sched_barrier(0);
                } else {
#pragma unroll
                    for (int k = 0; k < 2; ++k)
#pragma unroll
                        for (int s = 0; s < 2; ++s) { res[s][0][k] = rv[u + k][s].x; res[s][1][k] = rv[u + k][s].y; }
                }
                float v[2][2][2];   // [channel of the pair][slice][position]
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float4 n = n2[k];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        v[k][s][0] = gn_value(q, yv[u + k][s].x, n.x, n.y, n.z, n.w, 1.0f, 0.0f, false, res[s][0][k], true);
                        v[k][s][1] = gn_value(q, yv[u + k][s].y, n.x, n.y, n.z, n.w, 1.0f, 0.0f, false, res[s][1][k], true);
                    }
                }
                // lanes 0-31 keep channel u and receive the odd row's values of it, lanes 32-63 the reverse with u + 1
                float sum = 0.0f;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const auto e0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[0][s][0]), __float_as_uint(v[1][s][0]), false, false);
                    const auto e1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[0][s][1]), __float_as_uint(v[1][s][1]), false, false);
                    sum += __uint_as_float(e0[0]);   // even row, w
                    sum += __uint_as_float(e1[0]);   // even row, w + 1
                    sum += __uint_as_float(e0[1]);   // odd row, w
                    sum += __uint_as_float(e1[1]);   // odd row, w + 1
                }
                load_pair(xb, cn + u, yv, u);
                if constexpr (!REBUILD) load_pair(rb, cn + u, rv, u);
                const float o = sum / 8.0f;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(ob + (size_t)(cg0 + cl + u) * oD * (oH * oW)) + ooff) = o;
                mbits = max(mbits, range_bits(o));
                __builtin_amdgcn_sched_barrier(0);   // one channel pair at a time (hoisting more of the next pairs' tap reads spills)
            }
        };
        float2 ya[GPW_TRIP][2], ra[GPW_TRIP][2] = {};
#pragma unroll
        for (int u = 0; u < GPW_TRIP; u += 2) {
            load_pair(xb, c_lo + u, ya, u);
            if constexpr (!REBUILD) load_pair(rb, c_lo + u, ra, u);
            __builtin_amdgcn_sched_barrier(0);   // (in the walk's order: the compiler's count of loads in flight at the top of a trip is the
                                                 //  smaller of this path's and the loop's; out of order it drains them all, once per trip)
        }
#pragma unroll 1
        for (int cl = c_lo; cl < c_hi; cl += GPW_TRIP)
            do_trip(cl, min(cl + GPW_TRIP, c_hi - GPW_TRIP), ya, ra);   // (the last trip asks for itself again: no branch in the walk)
    };
    if (c_lo < c_hi) {
#pragma unroll 1
        for (int r = 0; r < K2_TH / GPW_ROWS; ++r) {
            const int h = h0 + r * GPW_ROWS;
            if (!(h < H && w < W)) break;   // (H even: both rows of a pair, i.e. both halves of the wave, stay or leave; later passes lie lower still)
            if (rebuild) {
                if (r + 1 < K2_TH / GPW_ROWS) load_coords(h + GPW_ROWS, cfn);
                pass(std::true_type{}, h);
            } else {
                pass(std::false_type{}, h);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < 6; ++i) cf[s][i] = cfn[s][i];
        }
    }
    if (p.range) range_note_block(mbits, p.range, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
}

// The tiles warp_gather_kernel marked: one position per lane, lanes running along w, so for a smooth field every tap load of
// a wave covers one or two contiguous row segments (the per-CU L1 serves the overlap between taps and rows) and the stores
// are contiguous 128-byte rows; the x-neighbour taps come in pairs (gather8_pairs).  Workgroups of unmarked tiles exit.
template <typename TV>
__device__ __forceinline__ void
warp_gather_direct_body(const TV *__restrict__ v, const float *__restrict__ coords, float *__restrict__ out,
                        float *__restrict__ out_range, const int *__restrict__ todo, int B, int C, int D, int H, int W,
                        unsigned blk_x, unsigned grid_x, unsigned blk_y, unsigned grid_y) {
    unsigned mbits = 0;
    const unsigned bid = xcd_remap(blk_x, grid_x);  // same logical order as warp_gather_kernel
    if (todo[bid] == 2) {  // block-uniform
        const int HW = H * W;
        const int tiles_w = (W + K2_TW - 1) / K2_TW, tiles_h = (H + K2_TH - 1) / K2_TH;
        const int d = (int)(bid % (unsigned)D);
        const int tile = (int)((bid / (unsigned)D) % (unsigned)(tiles_w * tiles_h));
        const int b = (int)(bid / ((unsigned)D * (unsigned)(tiles_w * tiles_h)));
        const size_t vol = (size_t)D * HW;
        // a workgroup takes four passes of 256 positions (RPP rows each): blk_y = (row part of the tile) * K2_DIRECT_SPLIT + channel group
        constexpr int RPP = 256 / K2_TW, NP = 4;
        static_assert(K2_TH % (NP * RPP) == 0, "tile rows");
        const int part = (int)blk_y / K2_DIRECT_SPLIT;
        blk_y %= K2_DIRECT_SPLIT; grid_y = K2_DIRECT_SPLIT;
        const int w = (tile % tiles_w) * K2_TW + (int)(threadIdx.x % K2_TW);
        const int hb = (tile / tiles_w) * K2_TH + part * NP * RPP + (int)(threadIdx.x / K2_TW);  // rows hb, hb+RPP, ...
        Taps t[NP];
        bool act[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int h = hb + RPP * i;
            act[i] = h < H && w < W;
            if (act[i]) {
                const float *cq = coords + (((size_t)b * D + d) * HW + h * W + w) * 3;
                t[i] = make_taps(Coord3{cq[0], cq[1], cq[2]}, D, H, W);
            }
        }
        const TV *vb = v + (size_t)b * C * vol;
        float *ob = out + (size_t)b * C * vol + (size_t)d * HW + hb * W + w;
        // channels are split over grid_y workgroups: this path is latency-bound (L2-hit gathers), it needs every wave slot
        const int cpg = (C + (int)grid_y - 1) / (int)grid_y;
        const int c_end = min(C, ((int)blk_y + 1) * cpg);
#pragma unroll 2
        for (int c = (int)blk_y * cpg; c < c_end; ++c) {
            const TV *src = vb + (size_t)c * vol;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                if (act[i]) {
                    const float r = W >= 2 ? gather8_pairs(src, t[i]) : gather8(src, t[i]);
                    ob[(size_t)c * vol + RPP * i * W] = r;
                    mbits = max(mbits, range_bits(r));
                }
            }
        }
    }
    // the rare path folds its maximum into the slot warp_gather_kernel wrote for this tile (one atomic per wave that did work;
    // idle workgroups leave without touching the descriptor)
    if (out_range && todo[bid] == 2) {
        mbits = wave_umax(mbits);
        if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + bid, mbits);
    }
}

// The same marked tiles, walked like K3 walks them: a workgroup owns a 16 x 16 tile of (h,w) positions, ALL D output slices and
// K2C_CPB channels; every thread runs down the slices of its position (taps once per slice, channels innermost).  Consecutive
// output slices of a smooth field sample neighbouring source planes, so the plane a slice fetched is still in the L1 / L2 when
// the next slice needs it — the direct gather, one workgroup per (tile, slice), re-fetches it from another CU.
#ifndef MPHIP_K2C_CPB
#define MPHIP_K2C_CPB 16
#endif
constexpr int K2C_CPB = MPHIP_K2C_CPB;
template <typename TV>
__device__ __forceinline__ void
warp_gather_columns_body(const TV *__restrict__ v, const float *__restrict__ coords, float *__restrict__ out,
                         float *__restrict__ out_range, const int *__restrict__ todo, int B, int C, int D, int H, int W,
                         unsigned blk, unsigned nblk) {
    const int HW = H * W;
    const int tiles_w = (W + 15) / 16, tiles_h = (H + 15) / 16, ntile = tiles_w * tiles_h;
    const int tiles32_w = (W + K2_TW - 1) / K2_TW, ntile32 = tiles32_w * ((H + K2_TH - 1) / K2_TH);
    unsigned bid = xcd_remap(blk, nblk);  // the tiles of one (frame, channel slice) under one L2 (as K3)
    const int tile = (int)(bid % ntile); bid /= ntile;
    const int slices = (C + K2C_CPB - 1) / K2C_CPB;
    const int slice = (int)(bid % slices), b = (int)(bid / slices);
    const int h = (tile / tiles_w) * 16 + (int)(threadIdx.x >> 4);
    const int w = (tile % tiles_w) * 16 + (int)(threadIdx.x & 15);
    const bool active = h < H && w < W;
    const int p = h * W + w;
    const size_t vol = (size_t)D * HW;
    const int c0 = slice * K2C_CPB, cs = min(K2C_CPB, C - c0);
    // the 16 x 16 tile lies inside one 32 x 32 tile of warp_gather_kernel: its marks, one per slice (block-uniform)
    const int t32 = ((tile / tiles_w) * 16 / K2_TH) * tiles32_w + (tile % tiles_w) * 16 / K2_TW;
    const int *marks = todo + ((size_t)b * ntile32 + t32) * D;
    const TV *vb = v + ((size_t)b * C + c0) * vol;
    float *ob = out + ((size_t)b * C + c0) * vol + p;
    unsigned mbits = 0;
    // nothing marked for this column (every launch on the reference's own fields): leave after ONE round of loads
    int mine = 0;
    for (int d = threadIdx.x; d < D; d += 256) mine |= marks[d] == 1;
    if (!__syncthreads_or(mine)) return;
    for (int d = 0; d < D; ++d) {
        if (marks[d] != 1 || !active) continue;
        const float *q = coords + (((size_t)b * D + d) * HW + p) * 3;
        const Taps t = make_taps(Coord3{q[0], q[1], q[2]}, D, H, W);
#pragma unroll
        for (int c = 0; c < K2C_CPB; ++c)
            if (c < cs) {
                const float r = gather8_pairs(vb + (size_t)c * vol, t);
                ob[(size_t)c * vol + (size_t)d * HW] = r;
                mbits = max(mbits, range_bits(r));
            }
    }
    if (out_range) {  // into the slot warp_gather_kernel wrote for (frame, 32 x 32 tile, slice 0)
        mbits = wave_umax(mbits);
        if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned *>(out_range) + 4 + ((size_t)b * ntile32 + t32) * D, mbits);
    }
}

// The kernels of the two walks.  Their code stays in the *_body functions above: written straight into the kernels, hipcc allocates the fp32
// instantiations' registers differently (same resources, another instruction stream than the recorded one).
// Two launches, not one kernel with two roles: merged, the column walk inherits the direct gather's 223 registers (two waves
// per SIMD) and loses what it gained (smooth field 223 -> 325 us); the second, mostly idle launch costs the reference-field path ~4 us.
template <int DT>
__global__ void __launch_bounds__(256)
warp_gather_columns_kernel(const dtype_t<DT> *__restrict__ v, const float *__restrict__ coords, float *__restrict__ out,
                           float *__restrict__ out_range, const int *__restrict__ todo, int B, int C, int D, int H, int W) {
    warp_gather_columns_body(v, coords, out, out_range, todo, B, C, D, H, W, blockIdx.x, gridDim.x);
}
template <int DT>
__global__ void __launch_bounds__(256)
warp_gather_direct_kernel(const dtype_t<DT> *__restrict__ v, const float *__restrict__ coords, float *__restrict__ out,
                          float *__restrict__ out_range, const int *__restrict__ todo, int B, int C, int D, int H, int W) {
    warp_gather_direct_body(v, coords, out, out_range, todo, B, C, D, H, W, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);
}

// K3: a workgroup owns a compact 16 x 16 tile of (h,w) positions of one frame and CPB channels; every thread walks the D
// output slices of its position accumulating the depth projection in registers (d ascending, like torch.sum(dim=2) on
// the warped volume, which is never written).  If the source box of ALL D slices fits the LDS image (the reference's own
// fields: a 4^3 corner) it is staged once, [voxel][channel] with 16-byte tap reads; otherwise the taps are gathered from
// global memory through the L1 (lanes along w, x-neighbours in pairs).
#ifndef MPHIP_K3_TH
#define MPHIP_K3_TH 16
#endif
constexpr int K3_TH = MPHIP_K3_TH, K3_TW = 256 / MPHIP_K3_TH;
template <int CPB, int DTO>
__global__ void __launch_bounds__(256)
warp_gather_dsum_kernel(const float *__restrict__ v, const float *__restrict__ coords, dtype_t<DTO> *__restrict__ out,
                        int B, int C, int D, int H, int W, size_t v_frame_stride /* floats; 0 = one shared source volume */) {
    __shared__ __attribute__((aligned(16))) float lds[STAGE_FLOATS];
    __shared__ int red[24];
    const int HW = H * W;
    const int tiles_w = (W + K3_TW - 1) / K3_TW, tiles_h = (H + K3_TH - 1) / K3_TH, ntile = tiles_w * tiles_h;
    // XCD-aware order: the tiles of one (frame, channel slice) are consecutive logical ids, i.e. they run on ONE XCD at about the
    // same time — w-neighbours share every 128-byte line of a source row, h-neighbours the halo rows, and with the hardware's
    // round-robin (tile t -> XCD t % 8) each of those lines was fetched into up to four different L2s (travelling fields: 5x the
    // algorithmic bytes crossed the fabric, at 6.9 TB/s — the kernel's limit)
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = (int)(bid % ntile); bid /= ntile;
    const int slices = (C + CPB - 1) / CPB;
    const int slice = (int)(bid % slices), b = (int)(bid / slices);
    static_assert(K3_TH * K3_TW == 256, "one thread per position of the tile");
    const int h = (tile / tiles_w) * K3_TH + (int)(threadIdx.x / K3_TW);
    const int w = (tile % tiles_w) * K3_TW + (int)(threadIdx.x % K3_TW);
    const bool active = h < H && w < W;
    const int p = h * W + w;
    const size_t vol = (size_t)D * HW;
    const int c0 = slice * CPB;
    const int cs = min(CPB, C - c0);
    const int cs_pad = lds_pitch_for(cs);
    const float *cp = coords + ((size_t)b * D * HW + (active ? p : 0)) * 3;
    const float *vb = v + (size_t)b * v_frame_stride;

    float acc[CPB];
#pragma unroll
    for (int c = 0; c < CPB; ++c) acc[c] = 0.0f;

    int lx = INT_MAX, ly = INT_MAX, lz = INT_MAX, hx = 0, hy = 0, hz = 0;
    if (active) {
        for (int d = 0; d < D; ++d) {
            const float *q = cp + (size_t)d * HW * 3;
            int x = (int)floorf(q[0]), y = (int)floorf(q[1]), z = (int)floorf(q[2]);
            lx = min(lx, x); ly = min(ly, y); lz = min(lz, z);
            hx = max(hx, x); hy = max(hy, y); hz = max(hz, z);
        }
    }
    const Box all = block_box(lx, ly, lz, hx, hy, hz, D, H, W, red);
    if (all.ex * all.ey * all.ez * cs_pad <= STAGE_FLOATS) {  // block-uniform: everything in one [voxel][channel] image
        stage_box(vb, lds, all, c0, cs, cs_pad, H, W, vol);
        __syncthreads();
        if (active) {
            for (int d = 0; d < D; ++d) {
                const float *q = cp + (size_t)d * HW * 3;
                Coord3 cc{q[0], q[1], q[2]};
                Taps t = make_taps(cc, D, H, W);
                const TapOff lt = rebase(t, (int)floorf(cc.x), (int)floorf(cc.y), (int)floorf(cc.z), all, cs_pad);
#pragma unroll
                for (int c = 0; c < CPB; c += 4) {
                    if (c + 4 <= cs) {
                        float tmp[4];
                        gather8x4(lds + c, lt, t.w, tmp);
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[c + k] += tmp[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c + k < cs) acc[c + k] += gather8_lds(lds + c + k, lt, t.w);
                    }
                }
            }
        }
    } else if (active) {
        // a field that travels through the volume: gather from global memory; lanes run along w (coalesced row segments for
        // a smooth field, the per-CU L1 serves the overlap between taps), x-neighbour taps in pairs
        for (int d = 0; d < D; ++d) {
            const float *q = cp + (size_t)d * HW * 3;
            const Taps t = make_taps(Coord3{q[0], q[1], q[2]}, D, H, W);
#pragma unroll
            for (int c = 0; c < CPB; ++c)
                if (c < cs) acc[c] += W >= 2 ? gather8_pairs(vb + (size_t)(c0 + c) * vol, t) : gather8(vb + (size_t)(c0 + c) * vol, t);
        }
    }
    if (!active) return;
    // DTO: the output's dtype (model dtypes) — fp32 accumulation whatever it is, the projection rounded ONCE, at the store (fp32: as it is)
#pragma unroll
    for (int c = 0; c < CPB; ++c)
        if (c < cs) out[((size_t)b * C + c0 + c) * HW + p] = narrow<DTO>(acc[c]);
}

// Fallback for W % 4 != 0 (never the case on the hot path): one thread per output voxel and channel slice.
template <int DT>
__global__ void __launch_bounds__(256)
warp_gather_scalar_kernel(const dtype_t<DT> *__restrict__ v, const float *__restrict__ coords, float *__restrict__ out,
                          int B, int C, int D, int H, int W, int cpb) {
    const size_t vol = (size_t)D * H * W;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * vol) return;
    int b = (int)(t / vol);
    size_t r = t - (size_t)b * vol;
    Coord3 c{coords[t * 3], coords[t * 3 + 1], coords[t * 3 + 2]};
    Taps taps = make_taps(c, D, H, W);
    const int c_begin = blockIdx.y * cpb, c_end = min(C, c_begin + cpb);
    for (int ch = c_begin; ch < c_end; ++ch)
        out[((size_t)b * C + ch) * vol + r] = gather8(v + ((size_t)b * C + ch) * vol, taps);
}

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_warp_field_compose(const float *theta, const float *em, const float *base_tbl, float *w,
                                        float *rt_out, float *em_out, int B, int eD, int eH, int eW, int G,
                                        void *stream) {
    MPHIP_REQUIRE(theta && em && base_tbl && w, "warp_field_compose: null pointer");
    MPHIP_REQUIRE(B > 0 && eD > 0 && eH > 0 && eW > 0 && G > 0, "warp_field_compose: bad dims");
    size_t n = (size_t)B * G * G * G;
    hipLaunchKernelGGL(warp_field_compose_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, theta, em,
                       base_tbl, w, rt_out, em_out, B, eD, eH, eW, G);
    return check_launch("warp_field_compose");
}

int mphip::check_warp_args(const char *name, const void *v, const void *field, const void *ld, const void *lh,
                           const void *lw, const void *out, int B, int C, int D, int H, int W, int fD, int fH,
                           int fW) {
    MPHIP_REQUIRE(v && field && ld && lh && lw && out, "%s: null pointer", name);
    MPHIP_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0 && fD > 0 && fH > 0 && fW > 0, "%s: bad dims", name);
    MPHIP_REQUIRE((size_t)D * H * W < (1u << 30), "%s: volume too large for 32-bit tap offsets", name);
    return MPHIP_OK;
}

static size_t k2_tiles(int B, int D, int H, int W) {
    return (size_t)B * D * ((H + K2_TH - 1) / K2_TH) * ((W + K2_TW - 1) / K2_TW);
}

static size_t k2_todo_bytes(int B, int D, int H, int W) { return ((k2_tiles(B, D, H, W) * sizeof(int) + 15) / 16) * 16; }
// coordinates [B,D,H,W,3] + one int per K2 tile (which of the two gather kernels takes it)
extern "C" size_t mphip_warp_workspace_bytes(int B, int D, int H, int W) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * D * H * W * 3 * sizeof(float) + k2_todo_bytes(B, D, H, W);
}
// K2's optional corner image (warp_corner_image_kernel): a workspace that is this much larger than the entry point's minimum lets the
// gather stage low-corner boxes — every box of the reference's own fields — from one compact copy per frame
extern "C" size_t mphip_warp_corner_image_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    size_t fl = 0;   // [frame][channel group][6^3 cells][k2_pitch(cg)], for whichever grouping the launch picks
    for (int cg : {min(C, K2_CG_MAX), 32, 16})
        if (cg <= C) fl = std::max(fl, (size_t)cdiv(C, cg) * k2_block_floats(cg));
    return (size_t)B * fl * sizeof(float);
}

int mphip::launch_coords(const float *field, const float *lin_d, const float *lin_h, const float *lin_w, float *coords,
                         int32_t *idx, int B, int D, int H, int W, int fD, int fH, int fW, hipStream_t s) {
    size_t n = (size_t)B * D * H * W;
    if (fH == H && fW == W)
        hipLaunchKernelGGL(warp_coords_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, s, field, lin_d, lin_h, lin_w,
                           coords, idx, B, D, H, W, fD, fH, fW);
    else
        hipLaunchKernelGGL(warp_coords_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, s, field, lin_d, lin_h, lin_w,
                           coords, idx, B, D, H, W, fD, fH, fW);
    return check_launch("warp_coords");
}

// the gather pass(es) of K2 on given coordinates; todo: one int per tile; corner_img: optional mphip_warp_corner_image_bytes(B, C) bytes.
// DT: the source volume's dtype (model dtypes).
template <int DT>
static int warp_volume_gather_t(const void *v_, const float *coords, float *out, float *out_range, int *todo, float *corner_img, bool img_ready,
                                int B, int C, int D, int H, int W, hipStream_t s) {
    const dtype_t<DT> *v = (const dtype_t<DT> *)v_;
    int rc;
    if (DT != MPHIP_DTYPE_F32 && W % 4 == 0 && !corner_img) {
        set_error("warp_volume (typed source): the workspace must include mphip_warp_corner_image_bytes(B, C) for the corner image");
        return MPHIP_EWORKSPACE;
    }
    const size_t nblocks = k2_tiles(B, D, H, W);
    // channel groups of the corner gather (its range slots: one per workgroup)
    const int cg = k2_group_channels(nblocks, C);
    const unsigned groups = (unsigned)cdiv(C, cg);
    if (out_range && (W % 4 != 0 || nblocks * groups > RANGE_MAX_PARTS)) {
        // (scalar fallback kernel / more workgroups than partial slots) the warp is a convex combination of v's voxels:
        // max|out| <= max|v|, so v's own range serves
        rc = cast_range_launch(v, DT, (size_t)B * C * D * H * W, nullptr, out_range, s);
        if (rc) return rc;
        out_range = nullptr;
    }
    if (W % 4 == 0) {
        const unsigned ncol = (unsigned)((size_t)B * ((H + 15) / 16) * ((W + 15) / 16) * cdiv(C, K2C_CPB));
        const dim3 gdirect((unsigned)nblocks, K2_DIRECT_SPLIT * (K2_TH / (4 * (256 / K2_TW))));
        if (corner_img && !img_ready)
            hipLaunchKernelGGL(warp_corner_image_kernel<DT>, dim3(K2_CORNER_CELLS, (unsigned)B), dim3(128), 0, s, v, corner_img, C, D, H, W, cg, (int)groups);
        hipLaunchKernelGGL(warp_gather_kernel<DT>, dim3((unsigned)nblocks, groups), dim3(K2_THREADS), 0, s, v, coords, out, out_range, todo, B, C, D, H, W,
                           (const float *)corner_img, cg);
        // the tiles it marked: smooth travelling fields -> column walk, incoherent ones -> direct gather (workgroups of the other
        // kind, and all of them on the reference's own fields, exit after one load)
        hipLaunchKernelGGL(warp_gather_columns_kernel<DT>, dim3(ncol), dim3(256), 0, s, v, (const float *)coords, out, out_range,
                           (const int *)todo, B, C, D, H, W);
        hipLaunchKernelGGL(warp_gather_direct_kernel<DT>, gdirect, dim3(256), 0, s, v, (const float *)coords,
                           out, out_range, (const int *)todo, B, C, D, H, W);
    } else {
        const int cpb = C >= 48 ? 12 : C;
        const dim3 grid(cdiv((size_t)B * D * H * W, 256), cdiv(C, cpb));
        hipLaunchKernelGGL(warp_gather_scalar_kernel<DT>, grid, dim3(256), 0, s, v, coords, out, B, C, D, H, W, cpb);
    }
    return check_launch("warp_volume");
}

static int warp_volume_gather(const void *v, int dtype, const float *coords, float *out, float *out_range, int *todo, float *corner_img,
                              bool img_ready, int B, int C, int D, int H, int W, hipStream_t s) {
    return dispatch_dtype(dtype, "warp_volume: unknown source dtype", [&](auto dt) {
        return warp_volume_gather_t<dt()>(v, coords, out, out_range, todo, corner_img, img_ready, B, C, D, H, W, s);
    });
}

// K2, coordinate pass included; `name`: the entry point that was called (error texts)
static int warp_volume_impl(const char *name, const void *v, int v_dtype, const float *field, const float *lin_d, const float *lin_h,
                            const float *lin_w, float *out, float *coords_out, int32_t *idx_out, float *out_range, int B, int C, int D, int H, int W,
                            int fD, int fH, int fW, void *workspace, size_t workspace_bytes, void *stream) {
    int rc = check_warp_args(name, v, field, lin_d, lin_h, lin_w, out, B, C, D, H, W, fD, fH, fW);
    if (rc) return rc;
    MPHIP_REQUIRE(!idx_out || coords_out, "%s: idx_out requires coords_out", name);
    const size_t need = mphip_warp_workspace_bytes(B, D, H, W), coord_bytes = (size_t)B * D * H * W * 3 * sizeof(float);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu bytes < required %zu", name, workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    float *coords = coords_out ? coords_out : (float *)workspace;
    int *todo = (int *)((char *)workspace + coord_bytes);
    float *corner_img = workspace_bytes >= need + mphip_warp_corner_image_bytes(B, C) ? (float *)((char *)workspace + need) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    rc = launch_coords(field, lin_d, lin_h, lin_w, coords, idx_out, B, D, H, W, fD, fH, fW, s);
    if (rc) return rc;
    return warp_volume_gather(v, v_dtype, coords, out, out_range, todo, corner_img, false, B, C, D, H, W, s);
}

extern "C" int mphip_warp_volume(const float *v, const float *field, const float *lin_d, const float *lin_h,
                                 const float *lin_w, float *out, float *coords_out, int32_t *idx_out, float *out_range, int B,
                                 int C, int D, int H, int W, int fD, int fH, int fW, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    return warp_volume_impl("warp_volume", v, MPHIP_DTYPE_F32, field, lin_d, lin_h, lin_w, out, coords_out, idx_out, out_range, B, C, D, H, W, fD, fH,
                            fW, workspace, workspace_bytes, stream);
}

extern "C" int mphip_warp_volume_typed(const void *v, int v_dtype, const float *field, const float *lin_d, const float *lin_h, const float *lin_w,
                                       float *out, float *coords_out, int32_t *idx_out, float *out_range, int B, int C, int D, int H, int W,
                                       int fD, int fH, int fW, void *workspace, size_t workspace_bytes, void *stream) {
    return warp_volume_impl("warp_volume_typed", v, v_dtype, field, lin_d, lin_h, lin_w, out, coords_out, idx_out, out_range, B, C, D, H, W, fD, fH,
                            fW, workspace, workspace_bytes, stream);
}

// K3's gather pass on given coordinates, the projection stored in out_dtype
static int launch_dsum(const float *v, const float *coords, void *out, int out_dtype, int B, int C, int D, int H, int W, size_t v_frame_stride,
                       hipStream_t s) {
    constexpr int CPB = 16;
    const int tiles = ((H + K3_TH - 1) / K3_TH) * ((W + K3_TW - 1) / K3_TW);
    const dim3 grid((unsigned)((size_t)B * tiles * cdiv(C, CPB)));
    return dispatch_dtype(out_dtype, "warp_volume_dsum: unknown output dtype", [&](auto dto) {
        hipLaunchKernelGGL((warp_gather_dsum_kernel<CPB, dto()>), grid, dim3(256), 0, s, v, coords, (dtype_t<dto()> *)out, B, C, D, H, W, v_frame_stride);
        return MPHIP_OK;
    });
}

static int warp_volume_dsum_impl(const char *name, const float *v, size_t v_frame_stride, const float *field,
                                 const float *lin_d, const float *lin_h, const float *lin_w, void *out, int out_dtype, int B, int C, int D,
                                 int H, int W, int fD, int fH, int fW, void *workspace, size_t workspace_bytes, void *stream) {
    int rc = check_warp_args(name, v, field, lin_d, lin_h, lin_w, out, B, C, D, H, W, fD, fH, fW);
    if (rc) return rc;
    size_t need = mphip_warp_workspace_bytes(B, D, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu bytes < required %zu", name, workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    float *coords = (float *)workspace;
    rc = launch_coords(field, lin_d, lin_h, lin_w, coords, nullptr, B, D, H, W, fD, fH, fW, s);
    if (rc) return rc;
    rc = launch_dsum(v, coords, out, out_dtype, B, C, D, H, W, v_frame_stride, s);
    if (rc) return rc;
    return check_launch(name);
}

// K1 + the coordinate pass fused (warp_field_coords_kernel): theta [B,3,4], em [B,3,eD,eH,eW] -> coords [B,D,G,G,3] of the warp of a
// (D,G,G) volume by the composed field — bit-identical to mphip_warp_field_compose + mphip_warp_coords, the field never exists.
extern "C" int mphip_warp_field_coords(const float *theta, const float *em, const float *base_tbl, const float *lin_d, const float *lin_h,
                                       const float *lin_w, float *coords, int B, int eD, int eH, int eW, int G, int D, void *stream) {
    MPHIP_REQUIRE(theta && em && base_tbl && lin_d && lin_h && lin_w && coords, "warp_field_coords: null pointer");
    MPHIP_REQUIRE(B > 0 && eD > 0 && eH > 0 && eW > 0 && G > 0 && D > 0, "warp_field_coords: bad dims");
    const size_t n = (size_t)B * D * G * G;
    hipLaunchKernelGGL(warp_field_coords_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, theta, em, base_tbl, lin_d, lin_h, lin_w,
                       coords, B, eD, eH, eW, G, D);
    return check_launch("warp_field_coords");
}

// K2 on given coordinates (mphip_warp_coords / mphip_warp_field_coords); workspace: one int per 32x32 tile
// (mphip_warp_workspace_bytes covers it).
extern "C" int mphip_warp_volume_coords(const float *v, const float *coords, float *out, float *out_range, int B, int C, int D, int H, int W,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(v && coords && out, "warp_volume_coords: null pointer");
    MPHIP_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, "warp_volume_coords: bad dims");
    MPHIP_REQUIRE((size_t)D * H * W < (1u << 30), "warp_volume_coords: volume too large for 32-bit tap offsets");
    const size_t need = k2_todo_bytes(B, D, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("warp_volume_coords: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    float *corner_img = workspace_bytes >= need + mphip_warp_corner_image_bytes(B, C) ? (float *)((char *)workspace + need) : nullptr;
    return warp_volume_gather(v, MPHIP_DTYPE_F32, coords, out, out_range, (int *)workspace, corner_img, false, B, C, D, H, W, (hipStream_t)stream);
}

// The corner image on its own: a caller that has `v` long before the coordinates (the hot slice: vs is an INPUT, the coordinates come out
// of an 18-launch generator chain) builds it early, off the critical path, and hands it to mphip_warp_volume_coords_img.
static int warp_corner_image_impl(const char *name, const void *v, int v_dtype, void *img, size_t img_bytes, int B, int C, int D, int H, int W,
                                  void *stream) {
    MPHIP_REQUIRE(v && img, "%s: null pointer", name);
    MPHIP_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", name);
    MPHIP_REQUIRE(((uintptr_t)img & 15) == 0, "%s: img must be 16-byte aligned", name);
    return dispatch_dtype(v_dtype, "warp_corner_image_typed: unknown dtype", [&](auto dt) {
        if (img_bytes < mphip_warp_corner_image_bytes(B, C)) {
            set_error("%s: buffer %zu bytes < required %zu", name, img_bytes, mphip_warp_corner_image_bytes(B, C));
            return (int)MPHIP_EWORKSPACE;
        }
        const int cg = k2_group_channels(k2_tiles(B, D, H, W), C);
        hipLaunchKernelGGL(warp_corner_image_kernel<dt()>, dim3(K2_CORNER_CELLS, (unsigned)B), dim3(128), 0, (hipStream_t)stream,
                           (const dtype_t<dt()> *)v, (float *)img, C, D, H, W, cg, cdiv(C, cg));
        return check_launch(name);
    });
}
extern "C" int mphip_warp_corner_image(const float *v, void *img, size_t img_bytes, int B, int C, int D, int H, int W, void *stream) {
    return warp_corner_image_impl("warp_corner_image", v, MPHIP_DTYPE_F32, img, img_bytes, B, C, D, H, W, stream);
}
extern "C" int mphip_warp_corner_image_typed(const void *v, int v_dtype, void *img, size_t img_bytes, int B, int C, int D, int H, int W, void *stream) {
    // (an fp32 volume reports as the untyped entry point)
    return warp_corner_image_impl(v_dtype == MPHIP_DTYPE_F32 ? "warp_corner_image" : "warp_corner_image_typed", v, v_dtype, img, img_bytes, B, C, D, H,
                                  W, stream);
}
static int warp_volume_coords_img_impl(const char *name, const void *v, int v_dtype, const float *coords, float *out, float *out_range, int B, int C,
                                       int D, int H, int W, void *workspace, size_t workspace_bytes, const void *img, void *stream) {
    MPHIP_REQUIRE(v && coords && out && img, "%s: null pointer", name);
    MPHIP_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", name);
    MPHIP_REQUIRE((size_t)D * H * W < (1u << 30), "%s: volume too large for 32-bit tap offsets", name);
    MPHIP_REQUIRE(((uintptr_t)img & 15) == 0, "%s: img must be 16-byte aligned", name);
    const size_t need = k2_todo_bytes(B, D, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu bytes < required %zu", name, workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    return warp_volume_gather(v, v_dtype, coords, out, out_range, (int *)workspace, (float *)img, true, B, C, D, H, W, (hipStream_t)stream);
}
extern "C" int mphip_warp_volume_coords_img(const float *v, const float *coords, float *out, float *out_range, int B, int C, int D, int H, int W,
                                            void *workspace, size_t workspace_bytes, const void *img, void *stream) {
    return warp_volume_coords_img_impl("warp_volume_coords_img", v, MPHIP_DTYPE_F32, coords, out, out_range, B, C, D, H, W, workspace, workspace_bytes,
                                       img, stream);
}
extern "C" int mphip_warp_volume_coords_img_typed(const void *v, int v_dtype, const float *coords, float *out, float *out_range, int B, int C, int D,
                                                  int H, int W, void *workspace, size_t workspace_bytes, const void *img, void *stream) {
    return warp_volume_coords_img_impl("warp_volume_coords_img_typed", v, v_dtype, coords, out, out_range, B, C, D, H, W, workspace, workspace_bytes,
                                       img, stream);
}

// K3 with the coordinate pass already done (mphip_warp_coords): lets a caller look at the sample positions BEFORE the volume is
// produced (mphip_warp_sample_box -> mphip_conv3d_fwd_roi).  shared != 0: v is ONE volume [1,C,D,H,W] for all B coordinate sets.
static int warp_volume_dsum_coords_impl(const char *name, const float *v, const float *coords, void *out, int out_dtype, int B, int C, int D, int H,
                                        int W, int shared, void *stream) {
    MPHIP_REQUIRE(v && coords && out, "%s: null pointer", name);
    MPHIP_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", name);
    const int rc = launch_dsum(v, coords, out, out_dtype, B, C, D, H, W, shared ? (size_t)0 : (size_t)C * D * H * W, (hipStream_t)stream);
    if (rc) return rc;
    return check_launch(name);
}
extern "C" int mphip_warp_volume_dsum_coords(const float *v, const float *coords, float *out, int B, int C, int D, int H, int W, int shared,
                                             void *stream) {
    return warp_volume_dsum_coords_impl("warp_volume_dsum_coords", v, coords, out, MPHIP_DTYPE_F32, B, C, D, H, W, shared, stream);
}
extern "C" int mphip_warp_volume_dsum_coords_typed(const float *v, const float *coords, void *out, int out_dtype, int B, int C, int D, int H, int W,
                                                   int shared, void *stream) {
    return warp_volume_dsum_coords_impl("warp_volume_dsum_coords_typed", v, coords, out, out_dtype, B, C, D, H, W, shared, stream);
}

extern "C" int mphip_warp_volume_dsum(const float *v, const float *field, const float *lin_d, const float *lin_h,
                                      const float *lin_w, float *out, int B, int C, int D, int H, int W, int fD,
                                      int fH, int fW, void *workspace, size_t workspace_bytes, void *stream) {
    return warp_volume_dsum_impl("warp_volume_dsum", v, (size_t)C * D * H * W, field, lin_d, lin_h, lin_w, out, MPHIP_DTYPE_F32, B, C, D, H, W,
                                 fD, fH, fW, workspace, workspace_bytes, stream);
}

extern "C" int mphip_warp_volume_dsum_shared(const float *v, const float *field, const float *lin_d, const float *lin_h,
                                             const float *lin_w, float *out, int B, int C, int D, int H, int W, int fD,
                                             int fH, int fW, void *workspace, size_t workspace_bytes, void *stream) {
    return warp_volume_dsum_impl("warp_volume_dsum_shared", v, 0, field, lin_d, lin_h, lin_w, out, MPHIP_DTYPE_F32, B, C, D, H, W, fD, fH, fW,
                                 workspace, workspace_bytes, stream);
}

extern "C" int mphip_warp_volume_dsum_typed(const float *v, int shared, const float *field, const float *lin_d, const float *lin_h,
                                            const float *lin_w, void *out, int out_dtype, int B, int C, int D, int H, int W, int fD, int fH, int fW,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    return warp_volume_dsum_impl("warp_volume_dsum_typed", v, shared ? (size_t)0 : (size_t)C * D * H * W, field, lin_d, lin_h, lin_w, out, out_dtype,
                                 B, C, D, H, W, fD, fH, fW, workspace, workspace_bytes, stream);
}

// ---- gn_apply_pool_warp_kernel: the pooled GroupNorm apply whose residual is K2's output (the hot-slice plan's first block) ----
// grid of the launch for a K2 of these dims: workgroups along x, K2's channels per image block, parts per block
static void gpw_grid(int N, int C, int D, int H, int W, unsigned &gx, int &cg, int &csub) {
    gx = (unsigned)((size_t)N * (D / 2) * ((H + K2_TH - 1) / K2_TH) * ((W + K2_TW - 1) / K2_TW));
    cg = k2_group_channels(k2_tiles(N, D, H, W), C);
    csub = 1;
    while ((size_t)gx * cdiv(C, cg) * csub < 256 && cg / (2 * csub) >= GPW_TRIP) csub *= 2;   // (a part: at least one trip of the walk)
}
bool mphip::gn_apply_pool_warp_ok(int N, int C, int D, int H, int W, int G) {
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || G <= 0 || C % G != 0) return false;
    if (C % GPW_TRIP != 0 || D % 2 != 0 || H % 2 != 0 || W % 4 != 0 || (size_t)D * H * W >= (1u << 30)) return false;
    unsigned gx; int cg, csub;
    gpw_grid(N, C, D, H, W, gx, cg, csub);
    return cg % GPW_TRIP == 0 && (size_t)gx * cdiv(C, cg) * csub <= RANGE_MAX_PARTS;
}
int mphip::gn_apply_pool_warp_launch(const float *x, const float *stats, const float *gamma, const float *beta, const float *residual, float *y, float *out_range, const float *coords, const int *todo, const float *img,
                                     int N, int C, int D, int H, int W, int G, hipStream_t s) {
    MPHIP_REQUIRE(x && stats && gamma && beta && residual && y && coords && todo && img, "groupnorm_apply(warp residual): null pointer");
    MPHIP_REQUIRE(gn_apply_pool_warp_ok(N, C, D, H, W, G), "groupnorm_apply(warp residual): unsupported dims");
    MPHIP_REQUIRE((((uintptr_t)x | (uintptr_t)residual | (uintptr_t)coords) & 7) == 0 && ((uintptr_t)img & 15) == 0,
                  "groupnorm_apply(warp residual): misaligned pointer");
    unsigned gx; int cg, csub;
    gpw_grid(N, C, D, H, W, gx, cg, csub);
    GnParams p{x, stats, gamma, beta, nullptr, nullptr, residual, y, C, C / G, 1, 0, out_range};
    hipLaunchKernelGGL(gn_apply_pool_warp_kernel, dim3(gx, (unsigned)(cdiv(C, cg) * csub)), dim3(GPW_THREADS), 0, s, p, coords, todo, img, D, H, W, cg,
                       csub);
    return check_launch("groupnorm_apply(warp residual)");
}

extern "C" int mphip_warp_coords(const float *field, const float *lin_d, const float *lin_h, const float *lin_w, float *coords,
                                 int B, int D, int H, int W, int fD, int fH, int fW, void *stream) {
    MPHIP_REQUIRE(field && lin_d && lin_h && lin_w && coords, "warp_coords: null pointer");
    MPHIP_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && fD > 0 && fH > 0 && fW > 0, "warp_coords: bad dims");
    return launch_coords(field, lin_d, lin_h, lin_w, coords, nullptr, B, D, H, W, fD, fH, fW, (hipStream_t)stream);
}

#ifdef MPHIP_K2_TRACE
extern "C" int mphip_debug_k2_trace(unsigned long long *host_out /* 4096 * 4 */) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mphip::g_k2_trace), sizeof(unsigned long long) * 4096 * 4) == hipSuccess ? 0 : -1;
}
#endif
