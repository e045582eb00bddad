// Tap and box helpers shared by the forward warps (warp.hip: K2/K3) and their backward (warp_bwd.hip: K10).
#pragma once
#include "mphip_common.h"
#include "mphip_resample.h"

namespace mphip {

// clipped un-normalised sample coordinate of an output voxel, per axis (warp.hip: coord_axis)
struct Coord3 {
    float x, y, z;
};

// 8-tap trilinear gather set-up for one voxel: base offset of the (z0,y0,x0) corner, the deltas
// to the +1 corners (0 when that corner is outside: ATen skips it, its weight is 0 there), and
// the 8 corner weights in ATen's accumulation order tnw,tne,tsw,tse,bnw,bne,bsw,bse.
struct Taps {
    int base, dx, dy, dz;
    float w[8];
};

__device__ __forceinline__ Taps make_taps(const Coord3 &c, int D, int H, int W) {
    Taps t;
    int x0 = (int)floorf(c.x), y0 = (int)floorf(c.y), z0 = (int)floorf(c.z);
    float wx1 = c.x - (float)x0, wx0 = (float)(x0 + 1) - c.x;
    float wy1 = c.y - (float)y0, wy0 = (float)(y0 + 1) - c.y;
    float wz1 = c.z - (float)z0, wz0 = (float)(z0 + 1) - c.z;
    bool vx = x0 + 1 < W, vy = y0 + 1 < H, vz = z0 + 1 < D;
    t.base = (z0 * H + y0) * W + x0;
    t.dx = vx ? 1 : 0;
    t.dy = vy ? W : 0;
    t.dz = vz ? H * W : 0;
    if (!vx) wx1 = 0.0f;
    if (!vy) wy1 = 0.0f;
    if (!vz) wz1 = 0.0f;
    t.w[0] = wx0 * wy0 * wz0;
    t.w[1] = wx1 * wy0 * wz0;
    t.w[2] = wx0 * wy1 * wz0;
    t.w[3] = wx1 * wy1 * wz0;
    t.w[4] = wx0 * wy0 * wz1;
    t.w[5] = wx1 * wy0 * wz1;
    t.w[6] = wx0 * wy1 * wz1;
    t.w[7] = wx1 * wy1 * wz1;
    return t;
}

__device__ __forceinline__ float gather8(const float *__restrict__ vol, const Taps &t) {
    const float *p = vol + t.base;
    float acc = 0.0f;
    acc += p[0] * t.w[0];
    acc += p[t.dx] * t.w[1];
    acc += p[t.dy] * t.w[2];
    acc += p[t.dy + t.dx] * t.w[3];
    acc += p[t.dz] * t.w[4];
    acc += p[t.dz + t.dx] * t.w[5];
    acc += p[t.dz + t.dy] * t.w[6];
    acc += p[t.dz + t.dy + t.dx] * t.w[7];
    return acc;
}

// The same 8 taps with the two x-neighbours of every (y,z) corner fetched by ONE 8-byte load (4 loads instead of 8; only
// dword alignment is needed).  Same values, same accumulation order -> bit-identical to gather8.  At the right border
// (dx == 0: the +x corner is outside, ATen skips it, its weight is 0) the pair is read one voxel to the left and both taps
// take its second element, i.e. p[0] — exactly what gather8 reads there.  Needs W >= 2.
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ float gather8_pairs(const float *__restrict__ vol, const Taps &t) {
    const float *p = vol + t.base - (t.dx ? 0 : 1);
    const f32x2u q0 = *reinterpret_cast<const f32x2u *>(p);
    const f32x2u q1 = *reinterpret_cast<const f32x2u *>(p + t.dy);
    const f32x2u q2 = *reinterpret_cast<const f32x2u *>(p + t.dz);
    const f32x2u q3 = *reinterpret_cast<const f32x2u *>(p + t.dz + t.dy);
    const bool in = t.dx != 0;
    float acc = 0.0f;
    acc += (in ? q0.x : q0.y) * t.w[0];
    acc += q0.y * t.w[1];
    acc += (in ? q1.x : q1.y) * t.w[2];
    acc += q1.y * t.w[3];
    acc += (in ? q2.x : q2.y) * t.w[4];
    acc += q2.y * t.w[5];
    acc += (in ? q3.x : q3.y) * t.w[6];
    acc += q3.y * t.w[7];
    return acc;
}

// Typed source volumes (model dtypes, include/mphip.h): the same 8 taps and accumulation order on values widened to fp32 on load —
// bitwise gather8 on the fp32 volume.  The pair form's 8-byte load has no 2-byte counterpart worth having: both read the taps one by one.
template <typename T>
__device__ __forceinline__ float gather8(const T *__restrict__ vol, const Taps &t) {
    const T *p = vol + t.base;
    float acc = 0.0f;
    acc += widen(p[0]) * t.w[0];
    acc += widen(p[t.dx]) * t.w[1];
    acc += widen(p[t.dy]) * t.w[2];
    acc += widen(p[t.dy + t.dx]) * t.w[3];
    acc += widen(p[t.dz]) * t.w[4];
    acc += widen(p[t.dz + t.dx]) * t.w[5];
    acc += widen(p[t.dz + t.dy]) * t.w[6];
    acc += widen(p[t.dz + t.dy + t.dx]) * t.w[7];
    return acc;
}
template <typename T>
__device__ __forceinline__ float gather8_pairs(const T *__restrict__ vol, const Taps &t) { return gather8(vol, t); }

struct Box {
    int ox, oy, oz, ex, ey, ez;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}

// Block-wide bounding box of the (x0,y0,z0) corners, extended by the +1 corner and clamped (NW waves; red: NW * 6 ints of LDS).
template <int NW>
__device__ __forceinline__ Box block_box_n(int lx, int ly, int lz, int hx, int hy, int hz, int D, int H, int W, int *red) {
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave * 6 + 0] = lx; red[wave * 6 + 1] = ly; red[wave * 6 + 2] = lz;
        red[wave * 6 + 3] = hx; red[wave * 6 + 4] = hy; red[wave * 6 + 5] = hz;
    }
    __syncthreads();
    int m[6] = {red[0], red[1], red[2], red[3], red[4], red[5]};
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        m[0] = min(m[0], red[w * 6]); m[1] = min(m[1], red[w * 6 + 1]); m[2] = min(m[2], red[w * 6 + 2]);
        m[3] = max(m[3], red[w * 6 + 3]); m[4] = max(m[4], red[w * 6 + 4]); m[5] = max(m[5], red[w * 6 + 5]);
    }
    Box bx;
    bx.ox = m[0]; bx.oy = m[1]; bx.oz = m[2];
    bx.ex = min(m[3] + 1, W - 1) - bx.ox + 1;
    bx.ey = min(m[4] + 1, H - 1) - bx.oy + 1;
    bx.ez = min(m[5] + 1, D - 1) - bx.oz + 1;
    return bx;
}
__device__ __forceinline__ Box block_box(int lx, int ly, int lz, int hx, int hy, int hz, int D, int H, int W,
                                         int *red /* >= 24 ints of LDS */) {
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave * 6 + 0] = lx; red[wave * 6 + 1] = ly; red[wave * 6 + 2] = lz;
        red[wave * 6 + 3] = hx; red[wave * 6 + 4] = hy; red[wave * 6 + 5] = hz;
    }
    __syncthreads();
    Box bx;
    bx.ox = min(min(red[0], red[6]), min(red[12], red[18]));
    bx.oy = min(min(red[1], red[7]), min(red[13], red[19]));
    bx.oz = min(min(red[2], red[8]), min(red[14], red[20]));
    int mx = max(max(red[3], red[9]), max(red[15], red[21]));
    int my = max(max(red[4], red[10]), max(red[16], red[22]));
    int mz = max(max(red[5], red[11]), max(red[17], red[23]));
    bx.ex = min(mx + 1, W - 1) - bx.ox + 1;
    bx.ey = min(my + 1, H - 1) - bx.oy + 1;
    bx.ez = min(mz + 1, D - 1) - bx.oz + 1;
    return bx;
}

// Stage channels [c0, c0+cs) of the box into lds[z][y][x][c] with an odd channel pitch cs_pad: a tap's LDS
// address is then the same for every channel up to an immediate offset (no per-channel address arithmetic in
// the gather loop) and lanes that read different voxels hit different banks.  Lane -> box element (decoded
// once per 64-element chunk), waves stride over channels.
__device__ __forceinline__ void stage_box(const float *__restrict__ vb /* v + b*C*vol */, float *lds, const Box &bx,
                                          int c0, int cs, int cs_pad, int H, int W, size_t vol) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int exy = bx.ex * bx.ey, bvol = exy * bx.ez;
    for (int r = lane; r < bvol; r += 64) {
        int z = r / exy, r2 = r - z * exy;
        int y = r2 / bx.ex, x = r2 - y * bx.ex;
        const float *src = vb + (size_t)c0 * vol + ((size_t)(bx.oz + z) * H + bx.oy + y) * W + bx.ox + x;
        float *dst = lds + r * cs_pad;
        // eight channel planes per trip, loads first: a load -> LDS-store trip at a time costs one L2 round trip per trip (24 of them
        // for 96 channels; r03: that was half of K2's 57 us on the reference's fields)
        for (int c = wave; c < cs; c += 32) {
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = c + 4 * k < cs ? src[(size_t)(c + 4 * k) * vol] : 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (c + 4 * k < cs) dst[c + 4 * k] = t[k];
        }
    }
}

// tap offsets of a voxel re-expressed in the staged LDS image (the 8 weights stay in the Taps)
struct TapOff {
    int base, dx, dy, dz;
};

__device__ __forceinline__ TapOff rebase(const Taps &t, int x0, int y0, int z0, const Box &bx, int cs_pad) {
    TapOff r;
    r.base = (((z0 - bx.oz) * bx.ey + (y0 - bx.oy)) * bx.ex + (x0 - bx.ox)) * cs_pad;
    r.dx = t.dx ? cs_pad : 0;
    r.dy = t.dy ? bx.ex * cs_pad : 0;
    r.dz = t.dz ? bx.ex * bx.ey * cs_pad : 0;
    return r;
}

// The tap arithmetic on the PACKED fp32 pipe, two channels per instruction: the (c, c+1) pair of a tap is exactly what one ds_read2_b32
// returns, and the tap's weight is broadcast to both halves by op_sel — weights stay single registers (pairs {w_2j, w_2j+1}, even / odd
// picked by the instruction's op_sel bits).  Written as inline assembly because hipcc's own packing of this loop duplicates every weight
// into a register pair (+180 registers, 700 B of scratch at 128).  With the staging gone the loop is VALU-bound (95 -> 52 instructions per
// channel pair).  Per channel and position still acc = 0; acc = acc + p_k * w_k in tap order, one rounding per op.
typedef float k2_f2 __attribute__((ext_vector_type(2)));
template <int ODD>
__device__ __forceinline__ k2_f2 k2_pk_mul(k2_f2 p, k2_f2 wpair) {
    k2_f2 m;
    if (ODD) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(m) : "v"(p), "v"(wpair));
    else     asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(m) : "v"(p), "v"(wpair));
    return m;
}
__device__ __forceinline__ k2_f2 k2_pk_add(k2_f2 a, k2_f2 b) {
    k2_f2 m;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(m) : "v"(a), "v"(b));
    return m;
}
// The channel pair (c, c+1) of N samples from the staged [cell][channel] image (src = image + c): tb = the eight tap addresses of a sample
// (floats, premultiplied by the even channel pitch: every read is one 8-byte-aligned ds_read_b64), wp = its weights in pairs.  All reads
// first (k2_tap_reads), then per sample the chain above (k2_tap_chain).  K2 (warp_gather_kernel) and the pooled apply that rebuilds K2's
// output (gn_apply_pool_warp_kernel, which issues the reads of the next pair ahead of the chain of this one) both get a value from these
// two and nothing else: one definition, the same bits.
template <int N>
__device__ __forceinline__ void k2_tap_reads(const float *src, const int (&tb)[N][8], k2_f2 (&pv)[N][8]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) pv[i][k] = *reinterpret_cast<const k2_f2 *>(src + tb[i][k]);   // (even pitch, even channel: 8-byte aligned)
}
template <int N>
__device__ __forceinline__ void k2_tap_chain(const k2_f2 (&pv)[N][8], const k2_f2 (&wp)[N][4], k2_f2 (&acc)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        acc[i] = k2_f2{0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[i] = k2_pk_add(acc[i], k2_pk_mul<0>(pv[i][2 * j], wp[i][j]));
            acc[i] = k2_pk_add(acc[i], k2_pk_mul<1>(pv[i][2 * j + 1], wp[i][j]));
        }
    }
}
template <int N>
__device__ __forceinline__ void k2_tap_pairs(const float *src, const int (&tb)[N][8], const k2_f2 (&wp)[N][4], k2_f2 (&acc)[N]) {
    k2_f2 pv[N][8];
    k2_tap_reads<N>(src, tb, pv);
    k2_tap_chain<N>(pv, wp, acc);
}
// a sample's tap addresses and weight pairs in that form, from its taps rebased into the image
__device__ __forceinline__ void k2_tap_setup(const TapOff &o, const Taps &t, int (&tb)[8], k2_f2 (&wp)[4]) {
    tb[0] = o.base; tb[1] = o.base + o.dx; tb[2] = o.base + o.dy; tb[3] = o.base + o.dy + o.dx;
    tb[4] = o.base + o.dz; tb[5] = o.base + o.dz + o.dx; tb[6] = o.base + o.dz + o.dy;
    tb[7] = o.base + o.dz + o.dy + o.dx;
#pragma unroll
    for (int j = 0; j < 4; ++j) wp[j] = k2_f2{t.w[2 * j], t.w[2 * j + 1]};
}

// host side, defined in warp.hip: argument checks of the warp entry points and the coordinate pass (warp_coords_kernel)
int check_warp_args(const char *name, const void *v, const void *field, const void *ld, const void *lh, const void *lw, const void *out, int B, int C,
                    int D, int H, int W, int fD, int fH, int fW);
int launch_coords(const float *field, const float *lin_d, const float *lin_h, const float *lin_w, float *coords, int32_t *idx, int B, int D, int H,
                  int W, int fD, int fH, int fW, hipStream_t s);

}  // namespace mphip
