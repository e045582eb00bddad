// K10 — backward of the warp kernels of warp.hip (K1/K2/K3).  Built with -ffp-contract=off like the forward.
#include "mphip_common.h"
#include "mphip_resample.h"
#include "mphip_warp.h"

// =====================================================================================================
// K10 — backward of K1/K2/K3 (scope row f2).  Gradients as torch.autograd gives them for the reference's ops:
// F.grid_sample(bilinear, border, align_corners=True) wrt input and grid (ATen GridSampler backward: clipped
// coordinates pass no gradient), the align_corners=True resize of the field, torch.sum(dim=2), F.affine_grid and
// the align_corners=False resize of the flow field.
namespace mphip {

// Scatter pass (dv via hardware fp32 atomics — the reference's own CUDA backward is an atomicAdd scatter too — and the
// coordinate gradient of each channel slice): a workgroup owns a 4x16x16 tile of output voxels (4 per thread) and WB_CH
// channels.  With a smooth field the source voxels of the tile form a small box (as in K2): dv contributions are
// accumulated in an LDS image of that box (ds_add_f32) and flushed with ONE global atomic per box element, in
// coalesced rows — ~1.7 global atomics per output value instead of 8 scattered ones.  (Tried on top, both without gain:
// explicit ds_add_f32 instead of flat atomics, +-0 %; handing x1 contributions to the x-neighbour lane by DPP to halve the
// LDS atomics, -20 %; storing the box image to a per-tile scratch slot and summing covering boxes per dv element in a second
// pass instead of the atomic flush, -60 %, and still not bitwise reproducible because the ds_add_f32 order varies.)  A box that does not fit
// (wild field) falls back to direct global atomics for that tile.
constexpr int WB_CH = 8;
constexpr int WB_LDS = 16384;  // floats: 64 KB of accumulation image
constexpr int FBOX_INTS = 8;   // per-frame sample box (warp_frame_box_kernel): ox, oy, oz, ex, ey, ez, dense, -
template <bool DSUM>
__global__ void __launch_bounds__(256)
warp_bwd_tiled_kernel(const float *__restrict__ v, const float *__restrict__ coords, const float *__restrict__ dout,
                      float *__restrict__ dv_all, float *__restrict__ dcoords, const int *__restrict__ fbox, int B, int C, int D,
                      int H, int W) {
    __shared__ float img[WB_LDS];
    __shared__ int red[24];
    const int HW = H * W;
    const size_t vol = (size_t)D * HW;
    const int tiles_w = (W + 15) / 16, tiles_h = (H + 15) / 16, tiles_d = (D + 3) / 4;
    int bid = blockIdx.x;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h; bid /= tiles_h;
    const int td = bid % tiles_d;
    const int b = bid / tiles_d;
    const int ox = tw * 16 + (threadIdx.x & 15), oy = th * 16 + (threadIdx.x >> 4);
    const int c0 = blockIdx.y * WB_CH, cs = min(WB_CH, C - c0);
    // a frame whose samples all fall into one small box belongs to the warp_bwd_dense_* kernels (block-uniform)
    if (fbox && fbox[b * FBOX_INTS + 6]) return;
    float *const dv = dv_all;

    bool ok[4];
    int base[4], dxyz[4];
    float wx1[4], wy1[4], wz1[4], cxs[4], cys[4], czs[4];
    int x0s[4], y0s[4], z0s[4];
    int lx = INT_MAX, ly = INT_MAX, lz = INT_MAX, hx = 0, hy = 0, hz = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int oz = td * 4 + k;
        ok[k] = ox < W && oy < H && oz < D;
        const size_t t = (size_t)b * vol + (size_t)(ok[k] ? oz : 0) * HW + (ok[k] ? oy * W + ox : 0);
        const float cx = coords[t * 3], cy = coords[t * 3 + 1], cz = coords[t * 3 + 2];
        const int x0 = (int)floorf(cx), y0 = (int)floorf(cy), z0 = (int)floorf(cz);
        cxs[k] = cx; cys[k] = cy; czs[k] = cz;
        x0s[k] = x0; y0s[k] = y0; z0s[k] = z0;
        const bool vx = x0 + 1 < W, vy = y0 + 1 < H, vz = z0 + 1 < D;
        wx1[k] = vx ? cx - (float)x0 : 0.0f;  // the +1 corner outside: ATen skips it
        wy1[k] = vy ? cy - (float)y0 : 0.0f;
        wz1[k] = vz ? cz - (float)z0 : 0.0f;
        dxyz[k] = (vx ? 1 : 0) | (vy ? 2 : 0) | (vz ? 4 : 0);
        base[k] = (z0 * H + y0) * W + x0;
        if (ok[k]) {
            lx = min(lx, x0); ly = min(ly, y0); lz = min(lz, z0);
            hx = max(hx, x0); hy = max(hy, y0); hz = max(hz, z0);
        }
    }
    const Box bx = block_box(lx, ly, lz, hx, hy, hz, D, H, W, red);
    const int bvol = bx.ex * bx.ey * bx.ez;
    const bool staged = dv != nullptr && bvol * WB_CH <= WB_LDS && bvol > 0;  // block-uniform
    if (staged) {
        for (int i = threadIdx.x; i < bvol * cs; i += 256) img[i] = 0.0f;
        __syncthreads();
    }
    float gx[4] = {0.f, 0.f, 0.f, 0.f}, gy[4] = {0.f, 0.f, 0.f, 0.f}, gz[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < cs; ++c) {
        const size_t plane = (size_t)b * C + c0 + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            const int oz = td * 4 + k;
            const float g = DSUM ? dout[plane * HW + oy * W + ox] : dout[plane * vol + (size_t)oz * HW + oy * W + ox];
            const bool vx = dxyz[k] & 1, vy = dxyz[k] & 2, vz = dxyz[k] & 4;
            const int dx = vx ? 1 : 0, dy = vy ? W : 0, dz = vz ? HW : 0;
            const float ax = (float)(x0s[k] + 1) - cxs[k], ay = (float)(y0s[k] + 1) - cys[k], az = (float)(z0s[k] + 1) - czs[k];
            const float bx1 = wx1[k], by1 = wy1[k], bz1 = wz1[k];
            if (dcoords) {
                const float *p = v + plane * vol + base[k];
                const float v000 = p[0], v100 = vx ? p[dx] : 0.0f, v010 = vy ? p[dy] : 0.0f, v110 = (vx && vy) ? p[dy + dx] : 0.0f;
                const float v001 = vz ? p[dz] : 0.0f, v101 = (vz && vx) ? p[dz + dx] : 0.0f;
                const float v011 = (vz && vy) ? p[dz + dy] : 0.0f, v111 = (vz && vy && vx) ? p[dz + dy + dx] : 0.0f;
                gx[k] += g * (((v100 - v000) * ay + (v110 - v010) * by1) * az + ((v101 - v001) * ay + (v111 - v011) * by1) * bz1);
                gy[k] += g * (((v010 - v000) * ax + (v110 - v100) * bx1) * az + ((v011 - v001) * ax + (v111 - v101) * bx1) * bz1);
                gz[k] += g * (((v001 - v000) * ax + (v101 - v100) * bx1) * ay + ((v011 - v010) * ax + (v111 - v110) * bx1) * by1);
            }
            if (dv) {
                float *q;
                int sx, sy, sz;
                if (staged) {
                    q = img + c * bvol + ((z0s[k] - bx.oz) * bx.ey + (y0s[k] - bx.oy)) * bx.ex + (x0s[k] - bx.ox);
                    sx = dx; sy = vy ? bx.ex : 0; sz = vz ? bx.ex * bx.ey : 0;
                } else {
                    q = dv + plane * vol + base[k];
                    sx = dx; sy = dy; sz = dz;
                }
                const float w00 = ay * az * g, w10 = by1 * az * g, w01 = ay * bz1 * g, w11 = by1 * bz1 * g;
                unsafeAtomicAdd(q, ax * w00);
                if (bx1 != 0.0f) unsafeAtomicAdd(q + sx, bx1 * w00);
                if (by1 != 0.0f) {
                    unsafeAtomicAdd(q + sy, ax * w10);
                    if (bx1 != 0.0f) unsafeAtomicAdd(q + sy + sx, bx1 * w10);
                }
                if (bz1 != 0.0f) {
                    unsafeAtomicAdd(q + sz, ax * w01);
                    if (bx1 != 0.0f) unsafeAtomicAdd(q + sz + sx, bx1 * w01);
                    if (by1 != 0.0f) {
                        unsafeAtomicAdd(q + sz + sy, ax * w11);
                        if (bx1 != 0.0f) unsafeAtomicAdd(q + sz + sy + sx, bx1 * w11);
                    }
                }
            }
        }
    }
    if (staged) {
        __syncthreads();
        const int exy = bx.ex * bx.ey;
        for (int i = threadIdx.x; i < bvol * cs; i += 256) {
            const float a = img[i];
            if (a == 0.0f) continue;
            const int c = i / bvol, e = i - c * bvol;
            const int z = e / exy, r2 = e - z * exy, y = r2 / bx.ex, x = r2 - y * bx.ex;
            unsafeAtomicAdd(dv + ((size_t)b * C + c0 + c) * vol + (size_t)(bx.oz + z) * HW + (bx.oy + y) * W + bx.ox + x, a);
        }
    }
    if (dcoords) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            const size_t t = (size_t)b * vol + (size_t)(td * 4 + k) * HW + oy * W + ox;
            float *o = dcoords + ((size_t)blockIdx.y * B * vol + t) * 3;
            o[0] = (cxs[k] > 0.0f && cxs[k] < (float)(W - 1)) ? gx[k] : 0.0f;
            o[1] = (cys[k] > 0.0f && cys[k] < (float)(H - 1)) ? gy[k] : 0.0f;
            o[2] = (czs[k] > 0.0f && czs[k] < (float)(D - 1)) ? gz[k] : 0.0f;
        }
    }
}

// ---- the reference's own fields: every sample of a frame inside one small box ------------------------------------------
// apply_warping_field hands grid_sample coordinates of size ~[-2, 3] as if they were voxel indices, so
// after the border clip EVERY output voxel of a frame samples the low corner of the volume: floor indices in {0, 1(, 2, 3)}.
// dv is then non-zero in E^3 voxels per channel (E = 3..5) and each of them receives a contribution from all D*H*W outputs: in the
// tiled scatter above that is ~1000 same-address LDS atomics per box element and tile, fully serialised (1.18 ms per warp at
// B=4, 15 % of a training step).  For such frames dv is a plain reduction over the outputs,
//     dv[c][cell] = sum_o dout[c][o] * Wt[o][cell],      Wt[o][cell] = fz(cell.z - z0(o)) * fy(..) * fx(..)
// i.e. a [C x outputs] x [outputs x E^3] GEMM with exact fp32 products: it runs on v_mfma_f32_32x32x2_f32 (M = 32 channels,
// N = 32 box cells, K = 2 outputs).  A lane supplies dout of its channel (one 16-byte load per four k-steps) and computes the
// trilinear weight of ITS cell for the k-step's output (zero unless the cell is one of the output's 8 corners) — no atomics, no
// LDS traffic in the loop.  Every wave reduces its own range of outputs; a workgroup folds its 4 waves in LDS and writes one
// partial [C][cells]; warp_bwd_dense_fold_kernel sums the partials of a frame in a fixed order (deterministic, unlike the scatter)
// and stores the box into the zero-filled dv.  The per-frame box comes from a one-workgroup-per-frame pass over the coordinates
// (fbox[6] = the smallest E in 3..5 that holds the frame, 0 = none): frames that do not qualify keep the tiled scatter.
constexpr int DENSE_E_MIN = 3, DENSE_E_MAX = 5;
constexpr int DENSE_SEGS = 64;       // workgroups (partials) per frame and 96-channel block
constexpr int DENSE_MT = 3;          // 32-channel MFMA row tiles per workgroup
constexpr int DENSE_COLS = 128;      // column stride of a partial (>= 5^3)
__host__ __device__ constexpr int dense_ntiles(int E) { return E == 3 ? 1 : E == 4 ? 2 : 4; }  // 32-cell MFMA column tiles

__global__ void __launch_bounds__(1024)
warp_frame_box_kernel(const float *__restrict__ coords, int *__restrict__ fbox, int D, int H, int W, int allow_dense) {
    __shared__ int red[16 * 6];
    const int b = blockIdx.x;
    const size_t vol = (size_t)D * H * W;
    const float *cb = coords + (size_t)b * vol * 3;
    int lx = INT_MAX, ly = INT_MAX, lz = INT_MAX, hx = 0, hy = 0, hz = 0;
    auto take = [&](float x, float y, float z) {
        const int x0 = (int)floorf(x), y0 = (int)floorf(y), z0 = (int)floorf(z);
        lx = min(lx, x0); ly = min(ly, y0); lz = min(lz, z0);
        hx = max(hx, x0); hy = max(hy, y0); hz = max(hz, z0);
    };
    if (vol % 4 == 0 && ((uintptr_t)cb & 15) == 0) {
        // four voxels = three 16-byte loads of contiguous memory per thread and step, four steps in flight: the frame's 786 KB stream through
        // ONE workgroup at the CU's load rate (r04's strided dword loads, 24 per step: 55 us per call, the longest single item in front of
        // the demand-driven final_conv on a one-stream step)
        const float4 *c4 = reinterpret_cast<const float4 *>(cb);
        const size_t groups = vol / 4;
        for (size_t g0 = threadIdx.x; g0 < groups; g0 += 4 * 1024) {
            float4 q[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t g = min(g0 + (size_t)u * 1024, groups - 1);  // (a clamped duplicate changes no minimum / maximum)
#pragma unroll
                for (int k = 0; k < 3; ++k) q[u][k] = c4[g * 3 + k];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                take(q[u][0].x, q[u][0].y, q[u][0].z);
                take(q[u][0].w, q[u][1].x, q[u][1].y);
                take(q[u][1].z, q[u][1].w, q[u][2].x);
                take(q[u][2].y, q[u][2].z, q[u][2].w);
            }
        }
    } else {
        for (size_t t0 = threadIdx.x; t0 < vol; t0 += 8 * 1024) {
            float c[8][3];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t t = min(t0 + (size_t)u * 1024, vol - 1);  // (a clamped duplicate changes no minimum / maximum)
                c[u][0] = cb[t * 3]; c[u][1] = cb[t * 3 + 1]; c[u][2] = cb[t * 3 + 2];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) take(c[u][0], c[u][1], c[u][2]);
        }
    }
    lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
    hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave * 6 + 0] = lx; red[wave * 6 + 1] = ly; red[wave * 6 + 2] = lz;
        red[wave * 6 + 3] = hx; red[wave * 6 + 4] = hy; red[wave * 6 + 5] = hz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            lx = min(lx, red[w * 6 + 0]); ly = min(ly, red[w * 6 + 1]); lz = min(lz, red[w * 6 + 2]);
            hx = max(hx, red[w * 6 + 3]); hy = max(hy, red[w * 6 + 4]); hz = max(hz, red[w * 6 + 5]);
        }
        const int ex = min(hx + 1, W - 1) - lx + 1, ey = min(hy + 1, H - 1) - ly + 1, ez = min(hz + 1, D - 1) - lz + 1;
        const int e = max(max(ex, ey), max(ez, DENSE_E_MIN));
        // (the GEMM walks the outputs in aligned groups of 4: 16-byte loads of dout; and in whole iterations of 32: its split over the
        // waves and the clamped prefetch of warp_bwd_dense_dv_kernel have no partial last iteration to get wrong)
        const bool shape_ok = (H * W) % 4 == 0 && vol >= 32 && vol % 32 == 0;
        int *o = fbox + b * FBOX_INTS;
        o[0] = lx; o[1] = ly; o[2] = lz; o[3] = ex; o[4] = ey; o[5] = ez;
        o[6] = (e <= DENSE_E_MAX && shape_ok && allow_dense) ? e : 0;
        o[7] = 0;
    }
}

template <bool DSUM, int E>
__global__ void __launch_bounds__(256)
warp_bwd_dense_dv_kernel(const float *__restrict__ coords, const float *__restrict__ dout, float *__restrict__ partial,
                         const int *__restrict__ fbox, int C, int D, int H, int W) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    constexpr int NT = dense_ntiles(E), MT = DENSE_MT;
    const int b = blockIdx.z;
    const int *fb = fbox + b * FBOX_INTS;
    if (fb[6] != E) return;  // block-uniform: another instantiation (or the tiled scatter) owns this frame
    const int ox = fb[0], oy = fb[1], oz = fb[2];
    const int HW = H * W;
    const size_t vol = (size_t)D * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int cblk = blockIdx.y * (MT * 32);
    // this wave's outputs: [t0, t1), walked 32 at a time: lane half h takes outputs +16h .. +16h+15, one per k-step (the order of
    // the k index is free).  One iteration = 16 k-steps x MT x NT MFMAs (1.5-6 us of matrix time), with the next iteration's
    // loads (4 x 16 B of dout per lane and row tile, one coordinate triple per lane) in flight underneath.  vol % 32 == 0 (shape_ok of
    // warp_frame_box_kernel): the 256 ranges cover the frame and every iteration is a whole one — neither holds for a ragged volume.
    const size_t per_wave = (vol / 32 + DENSE_SEGS * 4 - 1) / (DENSE_SEGS * 4) * 32;
    const size_t t0 = min(vol, ((size_t)blockIdx.x * 4 + wave) * per_wave), t1 = min(vol, t0 + per_wave);
    // LDS table of the current 32 outputs: per output the dense per-axis weight vectors fx[0..E), fy[0..E), fz[0..E) (a slot of
    // zeros at [15]); the weight of (output, cell) is one product of three table reads, no select chains in the k loop
    __shared__ __attribute__((aligned(16))) float tab_all[4][32][16];
    float (*tab)[16] = tab_all[wave];
    int offx[NT], offy[NT], offz[NT];  // table slots of this lane's column (box cell x, y, z) in every column tile
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int cell = n * 32 + col;
        offx[n] = cell % E; offy[n] = 5 + (cell / E) % E;
        offz[n] = cell < E * E * E ? 10 + cell / (E * E) : 15;  // padding columns read the zero slot
    }
    const float *gp[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) gp[m] = dout + ((size_t)b * C + min(cblk + m * 32 + col, C - 1)) * (DSUM ? (size_t)HW : vol);
    const float *cb = coords + (size_t)b * vol * 3;
    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    float4 gv[MT][4], gv_n[MT][4];
    float cx_l, cy_l, cz_l, cx_n, cy_n, cz_n;  // the coordinates of output t + lane % 32 (lanes 32..63 mirror 0..31)
    // branch-free and without selects on the loaded values (a conditional load is waited for at the end of its block, a select
    // right after the load — in both cases before the MFMAs the load should hide under): addresses are clamped into the frame;
    // outputs past the end of the range get an all-zero table row below, i.e. weight 0 (rows of channels >= C are never read back)
    auto load = [&](size_t t, float4 (*g)[4], float &lx_, float &ly_, float &lz_) {
        const size_t o = t + 16 * half;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t oq = min(o + 4 * q, vol - 4);
            const size_t gi = DSUM ? oq % (size_t)HW : oq;  // (H*W % 4 == 0: a group of 4 never leaves its plane)
#pragma unroll
            for (int m = 0; m < MT; ++m) g[m][q] = *reinterpret_cast<const float4 *>(gp[m] + gi);
        }
        const size_t oc = min(t + (size_t)col, vol - 1);
        lx_ = cb[oc * 3]; ly_ = cb[oc * 3 + 1]; lz_ = cb[oc * 3 + 2];
    };
    if (t0 < t1) load(t0, gv, cx_l, cy_l, cz_l);
    for (size_t t = t0; t < t1; t += 32) {
        load(min(t + 32, vol - 32), gv_n, cx_n, cy_n, cz_n);  // (the last iteration's prefetch is a discarded re-read)
        {   // this lane's output (t + col): the same weights as the tiled kernel — (x0+1) - cx on the floor corner, cx - x0 on
            // the +1 corner unless it is outside the volume
            const int x0 = (int)floorf(cx_l), y0 = (int)floorf(cy_l), z0 = (int)floorf(cz_l);
            const float ax = (float)(x0 + 1) - cx_l, ay = (float)(y0 + 1) - cy_l, az = (float)(z0 + 1) - cz_l;
            const float bx1 = x0 + 1 < W ? cx_l - (float)x0 : 0.0f, by1 = y0 + 1 < H ? cy_l - (float)y0 : 0.0f,
                        bz1 = z0 + 1 < D ? cz_l - (float)z0 : 0.0f;
            const int ix = x0 - ox, iy = y0 - oy;
            const int iz = t + col < t1 ? z0 - oz : -2;  // past the end of this wave's range: no z slot matches, weight 0
            float f[16];
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                f[e] = e == ix ? ax : e == ix + 1 ? bx1 : 0.0f;
                f[5 + e] = e == iy ? ay : e == iy + 1 ? by1 : 0.0f;
                f[10 + e] = e == iz ? az : e == iz + 1 ? bz1 : 0.0f;
            }
            f[15] = 0.0f;
            __builtin_amdgcn_wave_barrier();  // (every lane is past its reads of the previous table: one wave, program order)
            if (half == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(&tab[col][4 * q]) = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float *row = tab[16 * half + i];
            float w[NT];
#pragma unroll
#ifndef MPHIP_DENSE_ABL_NOTAB
            for (int n = 0; n < NT; ++n) w[n] = row[offz[n]] * row[offy[n]] * row[offx[n]];
#else
            for (int n = 0; n < NT; ++n) w[n] = cx_l + (float)(n + i);
#endif
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float4 q4 = gv[m][i >> 2];
                const float gmi = (i & 3) == 0 ? q4.x : (i & 3) == 1 ? q4.y : (i & 3) == 2 ? q4.z : q4.w;
#pragma unroll
#ifndef MPHIP_DENSE_ABL_NOMFMA
                for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(gmi, w[n], acc[m][n], 0, 0, 0);
#else
                for (int n = 0; n < NT; ++n) acc[m][n][(i + n) & 15] += gmi * w[n];
#endif
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < 4; ++q) gv[m][q] = gv_n[m][q];
        cx_l = cx_n; cy_l = cy_n; cz_l = cz_n;
    }
    // fold the 4 waves pairwise through LDS with plain stores / loads, [value][lane] (conflict-free) — ds_add_f32 costs ~4 cycles
    // per LANE: 192 of them per lane were 75 % of this kernel's time — then wave 0 writes the workgroup's partial [MT*32][DENSE_COLS]
    __shared__ float xch[2][MT * NT * 16][64];
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const int senders_from = step == 0 ? 2 : 1, nsend = step == 0 ? 2 : 1;  // waves 2,3 -> 0,1 ; then wave 1 -> 0
        if (wave >= senders_from && wave < senders_from + nsend) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) xch[wave - senders_from][(m * NT + n) * 16 + r][lane] = acc[m][n][r];
        }
        __syncthreads();
        if (wave < nsend) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][n][r] += xch[wave][(m * NT + n) * 16 + r][lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        float *pw = partial + (((size_t)b * gridDim.y + blockIdx.y) * DENSE_SEGS + blockIdx.x) * (MT * 32 * DENSE_COLS);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;  // D layout: row (channel), column = lane & 31 (cell)
                    pw[row * DENSE_COLS + n * 32 + col] = acc[m][n][r];
                }
    }
}

// dv[b][c][box cell] = sum over the frame's DENSE_SEGS partials, in index order (dv is zero-filled: only the box is written)
__global__ void __launch_bounds__(256)
warp_bwd_dense_fold_kernel(const float *__restrict__ partial, float *__restrict__ dv, const int *__restrict__ fbox, int C, int D,
                           int H, int W, int cblocks) {
    const int b = blockIdx.y;
    const int *fb = fbox + b * FBOX_INTS;
    const int E = fb[6];
    if (!E) return;
    const int cells = E * E * E;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= C * cells) return;
    const int c = t / cells, cell = t % cells;
    const int x = cell % E, y = (cell / E) % E, z = cell / (E * E);
    if (x >= fb[3] || y >= fb[4] || z >= fb[5]) return;  // outside the (border-clamped) box: its weights are all zero
    const float *p = partial + ((size_t)b * cblocks + c / (DENSE_MT * 32)) * DENSE_SEGS * (DENSE_MT * 32 * DENSE_COLS) +
                     (size_t)(c % (DENSE_MT * 32)) * DENSE_COLS + cell;
    float a = 0.0f;
    for (int sgm = 0; sgm < DENSE_SEGS; ++sgm) a += p[(size_t)sgm * (DENSE_MT * 32 * DENSE_COLS)];
    const int HW = H * W;
    dv[((size_t)b * C + c) * D * HW + (size_t)(fb[2] + z) * HW + (fb[1] + y) * W + fb[0] + x] = a;
}

// Coordinate gradient of the same frames.  d out / d coord is linear in the 8 corner values, so per output voxel
//     S_k = sum_c dout[c][o] * v[c][corner_k(o)]       (8 FMAs per channel, the corners read from an LDS copy of the box)
// and the trilinear derivative formulas are applied ONCE to the eight S_k instead of once per channel.  One slab of gradients
// (the tiled kernel writes one per 8-channel slice for the resize adjoint to sum), no re-read of v from HBM.
constexpr int DENSE_DC_CH = 96;   // channels per LDS box image (48 KB at E = 5)
template <bool DSUM>
__global__ void __launch_bounds__(256)
warp_bwd_dense_dcoords_kernel(const float *__restrict__ v, const float *__restrict__ coords, const float *__restrict__ dout,
                              float *__restrict__ dcoords, const int *__restrict__ fbox, int C, int D, int H, int W) {
    __shared__ float vbox[DENSE_DC_CH * DENSE_E_MAX * DENSE_E_MAX * DENSE_E_MAX];
    const int b = blockIdx.y;
    const int *fb = fbox + b * FBOX_INTS;
    const int E = fb[6];
    if (!E) return;  // block-uniform: the tiled kernel owns this frame
    const int ox = fb[0], oy = fb[1], oz = fb[2], ex = fb[3], ey = fb[4], ez = fb[5];
    const int cells = E * E * E;
    const int HW = H * W;
    const size_t vol = (size_t)D * HW;
    const size_t seg_len = ((vol + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
    const size_t t_begin = blockIdx.x * seg_len;
    constexpr int OPT = 4;  // outputs per thread
    float S[OPT][8];
#pragma unroll
    for (int i = 0; i < OPT; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) S[i][k] = 0.0f;
    int cbase[OPT], dx[OPT], dy[OPT], dz[OPT];
    size_t gi[OPT];
    bool ok[OPT];
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
        const size_t t = t_begin + (size_t)i * 256 + threadIdx.x;
        ok[i] = t < min(vol, t_begin + seg_len);
        const size_t tc = ok[i] ? t : 0;
        const float *cp = coords + ((size_t)b * vol + tc) * 3;
        const int x0 = (int)floorf(cp[0]), y0 = (int)floorf(cp[1]), z0 = (int)floorf(cp[2]);
        dx[i] = x0 + 1 < W ? 1 : 0;
        dy[i] = y0 + 1 < H ? E : 0;
        dz[i] = z0 + 1 < D ? E * E : 0;
        cbase[i] = ((z0 - oz) * E + (y0 - oy)) * E + (x0 - ox);
        gi[i] = DSUM ? tc % (size_t)HW : tc;
    }
    for (int c0 = 0; c0 < C; c0 += DENSE_DC_CH) {
        const int cs = min(DENSE_DC_CH, C - c0);
        __syncthreads();
        for (int i0 = threadIdx.x; i0 < cs * cells; i0 += 8 * 256) {  // eight loads in flight per thread (47 dependent ones otherwise)
            float val[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 256, cs * cells - 1);
                const int c = i / cells, cell = i - c * cells;
                const int x = cell % E, y = (cell / E) % E, z = cell / (E * E);
                const bool in = x < ex && y < ey && z < ez;
                const float got = v[((size_t)b * C + c0 + c) * vol + (size_t)(oz + min(z, ez - 1)) * HW + (oy + min(y, ey - 1)) * W + ox + min(x, ex - 1)];
                val[u] = in ? got : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u * 256 < cs * cells) vbox[i0 + u * 256] = val[u];
        }
        __syncthreads();
        const float *gp = dout + ((size_t)b * C + c0) * (DSUM ? (size_t)HW : vol);
#pragma unroll 4
        for (int c = 0; c < cs; ++c) {
            const float *vb = vbox + c * cells;
#pragma unroll
            for (int i = 0; i < OPT; ++i) {
                const float g = ok[i] ? gp[(size_t)c * (DSUM ? (size_t)HW : vol) + gi[i]] : 0.0f;
                const float *q = vb + cbase[i];
                S[i][0] = fmaf(g, q[0], S[i][0]);
                S[i][1] = fmaf(g, q[dx[i]], S[i][1]);
                S[i][2] = fmaf(g, q[dy[i]], S[i][2]);
                S[i][3] = fmaf(g, q[dy[i] + dx[i]], S[i][3]);
                S[i][4] = fmaf(g, q[dz[i]], S[i][4]);
                S[i][5] = fmaf(g, q[dz[i] + dx[i]], S[i][5]);
                S[i][6] = fmaf(g, q[dz[i] + dy[i]], S[i][6]);
                S[i][7] = fmaf(g, q[dz[i] + dy[i] + dx[i]], S[i][7]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
        if (!ok[i]) continue;
        const size_t t = t_begin + (size_t)i * 256 + threadIdx.x;
        const float *cp = coords + ((size_t)b * vol + t) * 3;
        const float cx = cp[0], cy = cp[1], cz = cp[2];
        const int x0 = (int)floorf(cx), y0 = (int)floorf(cy), z0 = (int)floorf(cz);
        const bool vx = dx[i] != 0, vy = dy[i] != 0, vz = dz[i] != 0;
        // corners outside the volume: ATen skips them (value 0, weight 0) — the same rule as the tiled kernel
        const float ax = (float)(x0 + 1) - cx, ay = (float)(y0 + 1) - cy, az = (float)(z0 + 1) - cz;
        const float bx1 = vx ? cx - (float)x0 : 0.0f, by1 = vy ? cy - (float)y0 : 0.0f, bz1 = vz ? cz - (float)z0 : 0.0f;
        const float v000 = S[i][0], v100 = vx ? S[i][1] : 0.0f, v010 = vy ? S[i][2] : 0.0f, v110 = (vx && vy) ? S[i][3] : 0.0f;
        const float v001 = vz ? S[i][4] : 0.0f, v101 = (vz && vx) ? S[i][5] : 0.0f, v011 = (vz && vy) ? S[i][6] : 0.0f,
                    v111 = (vz && vy && vx) ? S[i][7] : 0.0f;
        const float gx = ((v100 - v000) * ay + (v110 - v010) * by1) * az + ((v101 - v001) * ay + (v111 - v011) * by1) * bz1;
        const float gy = ((v010 - v000) * ax + (v110 - v100) * bx1) * az + ((v011 - v001) * ax + (v111 - v101) * bx1) * bz1;
        const float gz = ((v001 - v000) * ax + (v101 - v100) * bx1) * ay + ((v011 - v010) * ax + (v111 - v110) * bx1) * by1;
        float *o = dcoords + ((size_t)b * vol + t) * 3;  // slab 0
        o[0] = (cx > 0.0f && cx < (float)(W - 1)) ? gx : 0.0f;
        o[1] = (cy > 0.0f && cy < (float)(H - 1)) ? gy : 0.0f;
        o[2] = (cz > 0.0f && cz < (float)(D - 1)) ? gz : 0.0f;
    }
}

template <bool DSUM, int E>
static void launch_dense_dv(const float *coords, const float *dout, float *partial, const int *fbox, int B, int C, int D, int H,
                            int W, hipStream_t s) {
    hipLaunchKernelGGL((warp_bwd_dense_dv_kernel<DSUM, E>), dim3(DENSE_SEGS, cdiv(C, DENSE_MT * 32), B), dim3(256), 0, s, coords,
                       dout, partial, fbox, C, D, H, W);
}

template <bool ALIGN>
__device__ __forceinline__ void adj_bounds(int i, int in, int out, int &lo, int &hi) {
    // outputs whose source interval [i0, i1] can contain input index i (padded by one for rounding; weights decide)
    float a, b2;
    if (ALIGN) {
        const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
        if (!(scale > 0.0f)) { lo = 0; hi = out - 1; return; }
        a = ((float)i - 1.0f) / scale;
        b2 = ((float)i + 1.0f) / scale;
    } else {
        const float scale = (float)in / (float)out;
        a = ((float)i - 0.5f) / scale - 0.5f;
        b2 = ((float)i + 1.5f) / scale - 0.5f;
    }
    lo = max(0, (int)floorf(a) - 1);
    hi = min(out - 1, (int)ceilf(b2) + 1);
    if (!ALIGN && i == 0) lo = 0;  // src is clamped at 0: every o below the first source lands on i0 = 0
}
template <bool ALIGN>
__device__ __forceinline__ float adj_w(int o, int i, int in, int out) {
    const SrcIdx s = src_index<ALIGN>(o, in, out);
    float w = 0.0f;
    if (s.i0 == i) w += s.l0;
    if (s.i1 == i) w += s.l1;
    return w;
}

// adjoint of a trilinear resize [B,C,iD,iH,iW] -> [B,C,oD,oH,oW]: gin[i] = sum_o w(o -> i) * sum_slabs gout[o]
// (gather form, deterministic).  interleaved: gout is [slab][B][oVol][C] (the coordinate-gradient layout of
// warp_bwd_kernel) instead of [slab][B][C][oVol].
template <bool ALIGN>
__global__ void __launch_bounds__(256)
resize_trilinear_adjoint_kernel(const float *__restrict__ gout, float *__restrict__ gin, int B, int C, int iD, int iH, int iW,
                                int oD, int oH, int oW, int slabs_all, int interleaved, const int *__restrict__ fbox) {
    const size_t ivol = (size_t)iD * iH * iW, ovol = (size_t)oD * oH * oW;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * C * ivol) return;
    const int iw = (int)(t % iW);
    size_t r = t / iW;
    const int ih = (int)(r % iH);
    r /= iH;
    const int id = (int)(r % iD);
    r /= iD;
    const int ch = (int)(r % C), b = (int)(r / C);
    const int slabs = (fbox && fbox[b * FBOX_INTS + 6]) ? 1 : slabs_all;  // a dense frame's coordinate gradient is one slab
    int dlo, dhi, hlo, hhi, wlo, whi;
    adj_bounds<ALIGN>(id, iD, oD, dlo, dhi);
    adj_bounds<ALIGN>(ih, iH, oH, hlo, hhi);
    adj_bounds<ALIGN>(iw, iW, oW, wlo, whi);
    const size_t slab_stride = (size_t)B * C * ovol;
    float acc = 0.0f;
    for (int od = dlo; od <= dhi; ++od) {
        const float wd = adj_w<ALIGN>(od, id, iD, oD);
        if (wd == 0.0f) continue;
        float pl = 0.0f;
        for (int oh = hlo; oh <= hhi; ++oh) {
            const float wh = adj_w<ALIGN>(oh, ih, iH, oH);
            if (wh == 0.0f) continue;
            float rs = 0.0f;
            for (int ow = wlo; ow <= whi; ++ow) {
                const float ww = adj_w<ALIGN>(ow, iw, iW, oW);
                if (ww == 0.0f) continue;
                const size_t o = ((size_t)od * oH + oh) * oW + ow;
                const size_t idx = interleaved ? ((size_t)b * ovol + o) * C + ch : ((size_t)b * C + ch) * ovol + o;
                float g = gout[idx];
                for (int s = 1; s < slabs; ++s) g += gout[(size_t)s * slab_stride + idx];
                rs += ww * g;
            }
            pl += wh * rs;
        }
        acc += wd * pl;
    }
    gin[t] = acc;
}

// one axis of the same adjoint (the trilinear resize is separable): gin[outer][i][inner] = sum_o w(o -> i) * gout[outer][o][inner].
// Three of these replace the 3-D gather when the candidate box is large (16 -> 64 upsampling: ~8^3 outputs per input).
template <bool ALIGN>
__global__ void __launch_bounds__(256)
resize_adjoint_axis_kernel(const float *__restrict__ gout, float *__restrict__ gin, size_t outer, int in_len, int out_len,
                           size_t inner) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= outer * in_len * inner) return;
    const size_t q = t % inner;
    const int i = (int)((t / inner) % in_len);
    const size_t o_ = t / (inner * in_len);
    int lo, hi;
    adj_bounds<ALIGN>(i, in_len, out_len, lo, hi);
    const float *p = gout + (o_ * out_len) * inner + q;
    float acc = 0.0f;
    for (int o = lo; o <= hi; ++o) {
        const float w = adj_w<ALIGN>(o, i, in_len, out_len);
        if (w != 0.0f) acc += w * p[(size_t)o * inner];
    }
    gin[t] = acc;
}

// dtheta[b][j][k] = sum_p dw[b][j][p] * (x_p, y_p, z_p, 1)[k]   (F.affine_grid backward); partial sums per chunk
constexpr int TG_CHUNK = 8192;
__global__ void __launch_bounds__(256)
theta_grad_partial_kernel(const float *__restrict__ dw, const float *__restrict__ base, double *__restrict__ partial, int G,
                          int chunks) {
    const int bj = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const size_t vol = (size_t)G * G * G;
    const float *p = dw + (size_t)bj * vol;
    const size_t begin = (size_t)chunk * TG_CHUNK, end = min(vol, begin + TG_CHUNK);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = begin + threadIdx.x; i < end; i += 256) {
        const float g = p[i];
        const int w = (int)(i % G), h = (int)((i / G) % G), d = (int)(i / ((size_t)G * G));
        s[0] += (double)(g * base[w]);
        s[1] += (double)(g * base[h]);
        s[2] += (double)(g * base[d]);
        s[3] += (double)g;
    }
    __shared__ double red[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) s[k] += __shfl_xor(s[k], sft, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) partial[(size_t)blockIdx.x * 4 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ void theta_grad_finalize_kernel(const double *__restrict__ partial, float *__restrict__ dtheta, int n, int chunks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over B*3*4
    if (i >= n) return;
    const int bj = i / 4, k = i % 4;
    double a = 0.0;
    for (int c = 0; c < chunks; ++c) a += partial[((size_t)bj * chunks + c) * 4 + k];
    dtheta[i] = (float)a;
}

// backward of rt_theta_kernel: theta = rows 0..2 of A (or of inv(A)), A = [Rx*Ry*Rz | t; 0 0 0 1], angles in degrees.
// d(inv A) -> dA = -M^T dM M^T with M = inv(A); then the product rule through the three axis rotations.
__global__ void rt_theta_bwd_kernel(const float *__restrict__ rot, const float *__restrict__ tr, const float *__restrict__ dtheta,
                                    float *__restrict__ drot, float *__restrict__ dtr, int B, int invert) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double k = 0.017453292519943295;
    const double ra = (double)(rot[b * 3] * 0.017453292519943295f), rb = (double)(rot[b * 3 + 1] * 0.017453292519943295f),
                 rg = (double)(rot[b * 3 + 2] * 0.017453292519943295f);
    const double ca = cos(ra), sa = sin(ra), cb = cos(rb), sb = sin(rb), cg = cos(rg), sg = sin(rg);
    const double Rx[3][3] = {{1, 0, 0}, {0, ca, -sa}, {0, sa, ca}};
    const double Ry[3][3] = {{cb, 0, sb}, {0, 1, 0}, {-sb, 0, cb}};
    const double Rz[3][3] = {{cg, -sg, 0}, {sg, cg, 0}, {0, 0, 1}};
    double YZ[3][3], XY[3][3], R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0, u = 0.0;
            for (int q = 0; q < 3; ++q) { s += Ry[i][q] * Rz[q][j]; u += Rx[i][q] * Ry[q][j]; }
            YZ[i][j] = s;
            XY[i][j] = u;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int q = 0; q < 3; ++q) s += Rx[i][q] * YZ[q][j];
            R[i][j] = s;
        }
    double dA[3][4];  // gradient wrt the top three rows of A
    if (invert) {
        // A rigid: inv(A) = [R^T | -R^T t]; written through the general identity dA = -M^T dM M^T (dM's last row is 0)
        double M[4][4];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) M[i][j] = R[j][i];
            double s = 0.0;
            for (int q = 0; q < 3; ++q) s += R[q][i] * (double)tr[b * 3 + q];
            M[i][3] = -s;
        }
        M[3][0] = M[3][1] = M[3][2] = 0.0;
        M[3][3] = 1.0;
        double T[4][4];  // T = M^T dM  (dM rows 0..2 = dtheta, row 3 = 0)
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
                for (int q = 0; q < 3; ++q) s += M[q][i] * (double)dtheta[(b * 3 + q) * 4 + j];
                T[i][j] = s;
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
                for (int q = 0; q < 4; ++q) s += T[i][q] * M[j][q];
                dA[i][j] = -s;
            }
    } else {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) dA[i][j] = (double)dtheta[(b * 3 + i) * 4 + j];
    }
    for (int i = 0; i < 3; ++i) dtr[b * 3 + i] = (float)dA[i][3];
    // R = Rx * (Ry * Rz):  dRx = dR (YZ)^T,  dRy = Rx^T dR Rz^T,  dRz = (XY)^T dR
    double dRx[3][3], dRy[3][3], dRz[3][3], tmp[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0, u = 0.0, w = 0.0;
            for (int q = 0; q < 3; ++q) {
                s += dA[i][q] * YZ[j][q];
                u += Rx[q][i] * dA[q][j];
                w += XY[q][i] * dA[q][j];
            }
            dRx[i][j] = s;
            tmp[i][j] = u;
            dRz[i][j] = w;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int q = 0; q < 3; ++q) s += tmp[i][q] * Rz[j][q];
            dRy[i][j] = s;
        }
    const double da = dRx[1][1] * -sa + dRx[1][2] * -ca + dRx[2][1] * ca + dRx[2][2] * -sa;
    const double db = dRy[0][0] * -sb + dRy[0][2] * cb + dRy[2][0] * -cb + dRy[2][2] * -sb;
    const double dg = dRz[0][0] * -sg + dRz[0][1] * -cg + dRz[1][0] * cg + dRz[1][1] * -sg;
    drot[b * 3] = (float)(da * k);
    drot[b * 3 + 1] = (float)(db * k);
    drot[b * 3 + 2] = (float)(dg * k);
}

constexpr int WARP_BWD_CPB = WB_CH;  // channels per slice of the scatter pass

}  // namespace mphip

using namespace mphip;

// Per frame, the box of source voxels the samples of `coords` [B,D,H,W,3] touch (all 8 trilinear corners, zero-weight ones
// included): box[b*8 ..] = {lx, ly, lz, ex, ey, ez, -, -} — origin and extent in voxels.  One workgroup per frame.
extern "C" int mphip_warp_sample_box(const float *coords, int *box, int B, int D, int H, int W, void *stream) {
    MPHIP_REQUIRE(coords && box, "warp_sample_box: null pointer");
    MPHIP_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "warp_sample_box: bad dims");
    hipLaunchKernelGGL(warp_frame_box_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, coords, box, D, H, W, 0);
    return check_launch("warp_sample_box");
}

extern "C" size_t mphip_warp_volume_bwd_workspace_bytes(int B, int C, int D, int H, int W) {
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    const size_t groups = (size_t)cdiv(C, WARP_BWD_CPB);
    const size_t dense = (size_t)B * cdiv(C, DENSE_MT * 32) * DENSE_SEGS * (DENSE_MT * 32 * DENSE_COLS) * sizeof(float) +
                         (size_t)B * FBOX_INTS * sizeof(int);  // partials of the dense dv path + per-frame sample boxes
    return (size_t)B * D * H * W * 3 * sizeof(float) * (1 + groups) + dense;
}

extern "C" int mphip_warp_volume_bwd(const float *v, const float *field, const float *lin_d, const float *lin_h,
                                     const float *lin_w, const float *dout, float *dv, float *dfield, int B, int C, int D,
                                     int H, int W, int fD, int fH, int fW, int dsum, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    int rc = check_warp_args("warp_volume_bwd", v, field, lin_d, lin_h, lin_w, dout, B, C, D, H, W, fD, fH, fW);
    if (rc) return rc;
    MPHIP_REQUIRE(dv || dfield, "warp_volume_bwd: nothing to compute (dv and dfield are both NULL)");
    const size_t need = mphip_warp_volume_bwd_workspace_bytes(B, C, D, H, W);
    if (!workspace || workspace_bytes < need) {
        set_error("warp_volume_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
        return MPHIP_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t nvox = (size_t)B * D * H * W;
    float *coords = (float *)workspace, *dcoords = coords + nvox * 3;
    rc = launch_coords(field, lin_d, lin_h, lin_w, coords, nullptr, B, D, H, W, fD, fH, fW, s);
    if (rc) return rc;
    if (dv) {
        const size_t bytes = (size_t)B * C * D * H * W * sizeof(float);
        MPHIP_REQUIRE(bytes % 16 == 0 && ((uintptr_t)dv & 15) == 0, "warp_volume_bwd: dv must be 16-byte aligned / sized");
        zero_fill(dv, bytes, s);  // the scatter pass accumulates with atomics
    }
    const int groups = cdiv(C, WARP_BWD_CPB);
    // frames whose samples all sit in one small box (the reference's own fields) take the dense kernels: dv as a GEMM over the
    // outputs, the coordinate gradient from an LDS image of the box; every other frame the tiled scatter below
    float *partial = dcoords + nvox * 3 * groups;
    const int cblocks = cdiv(C, DENSE_MT * 32);
    int *fbox = (int *)(partial + (size_t)B * cblocks * DENSE_SEGS * (DENSE_MT * 32 * DENSE_COLS));
    const char *no_dense = getenv("MPHIP_WARP_BWD_DENSE");  // "0": every frame through the tiled scatter (tests: dense == tiled)
    hipLaunchKernelGGL(warp_frame_box_kernel, dim3(B), dim3(1024), 0, s, (const float *)coords, fbox, D, H, W,
                       (no_dense && no_dense[0] == '0') ? 0 : 1);
    if (dv) {
        if (dsum) {
            launch_dense_dv<true, 3>(coords, dout, partial, fbox, B, C, D, H, W, s);
            launch_dense_dv<true, 4>(coords, dout, partial, fbox, B, C, D, H, W, s);
            launch_dense_dv<true, 5>(coords, dout, partial, fbox, B, C, D, H, W, s);
        } else {
            launch_dense_dv<false, 3>(coords, dout, partial, fbox, B, C, D, H, W, s);
            launch_dense_dv<false, 4>(coords, dout, partial, fbox, B, C, D, H, W, s);
            launch_dense_dv<false, 5>(coords, dout, partial, fbox, B, C, D, H, W, s);
        }
        hipLaunchKernelGGL(warp_bwd_dense_fold_kernel, dim3(cdiv(C * 125, 256), B), dim3(256), 0, s, (const float *)partial, dv,
                           (const int *)fbox, C, D, H, W, cblocks);
    }
    if (dfield) {
        const dim3 dgrid((unsigned)cdiv((size_t)D * H * W, 1024), B);  // 4 outputs per thread
        if (dsum)
            hipLaunchKernelGGL(warp_bwd_dense_dcoords_kernel<true>, dgrid, dim3(256), 0, s, v, (const float *)coords, dout, dcoords,
                               (const int *)fbox, C, D, H, W);
        else
            hipLaunchKernelGGL(warp_bwd_dense_dcoords_kernel<false>, dgrid, dim3(256), 0, s, v, (const float *)coords, dout, dcoords,
                               (const int *)fbox, C, D, H, W);
    }
    dim3 grid((unsigned)((size_t)B * cdiv(D, 4) * cdiv(H, 16) * cdiv(W, 16)), groups);
    if (dsum)
        hipLaunchKernelGGL(warp_bwd_tiled_kernel<true>, grid, dim3(256), 0, s, v, (const float *)coords, dout, dv,
                           dfield ? dcoords : nullptr, (const int *)fbox, B, C, D, H, W);
    else
        hipLaunchKernelGGL(warp_bwd_tiled_kernel<false>, grid, dim3(256), 0, s, v, (const float *)coords, dout, dv,
                           dfield ? dcoords : nullptr, (const int *)fbox, B, C, D, H, W);
    if (dfield) {
        const size_t nf = (size_t)B * 3 * fD * fH * fW;
        hipLaunchKernelGGL(resize_trilinear_adjoint_kernel<true>, dim3(cdiv(nf, 256)), dim3(256), 0, s, (const float *)dcoords,
                           dfield, B, 3, fD, fH, fW, D, H, W, groups, 1, (const int *)fbox);
    }
    return check_launch("warp_volume_bwd");
}

extern "C" size_t mphip_warp_field_compose_bwd_workspace_bytes(int B, int G) {
    if (B <= 0 || G <= 0) return 0;
    const size_t theta = (size_t)B * 3 * cdiv((size_t)G * G * G, TG_CHUNK) * 4 * sizeof(double);
    const size_t axis = (size_t)B * 3 * G * G * G * sizeof(float) * 2;  // two intermediates of the separable adjoint (upper bound)
    return theta + axis;
}

extern "C" int mphip_warp_field_compose_bwd(const float *dw, const float *base_tbl, float *dtheta, float *dem, int B, int eD,
                                            int eH, int eW, int G, void *workspace, size_t workspace_bytes, void *stream) {
    MPHIP_REQUIRE(dw && base_tbl && (dtheta || dem), "warp_field_compose_bwd: null pointer");
    MPHIP_REQUIRE(B > 0 && eD > 0 && eH > 0 && eW > 0 && G > 0, "warp_field_compose_bwd: bad dims");
    hipStream_t s = (hipStream_t)stream;
    if (dtheta) {
        const size_t need = mphip_warp_field_compose_bwd_workspace_bytes(B, G);
        if (!workspace || workspace_bytes < need) {
            set_error("warp_field_compose_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        const int chunks = cdiv((size_t)G * G * G, TG_CHUNK);
        hipLaunchKernelGGL(theta_grad_partial_kernel, dim3(B * 3 * chunks), dim3(256), 0, s, dw, base_tbl, (double *)workspace, G,
                           chunks);
        hipLaunchKernelGGL(theta_grad_finalize_kernel, dim3(cdiv(B * 12, 64)), dim3(64), 0, s, (const double *)workspace, dtheta,
                           B * 12, chunks);
    }
    if (dem) {
        const size_t need = mphip_warp_field_compose_bwd_workspace_bytes(B, G);
        if (!workspace || workspace_bytes < need) {
            set_error("warp_field_compose_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
            return MPHIP_EWORKSPACE;
        }
        // separable: W, then H, then D (each pass gathers <= ~10 outputs per input along one axis)
        const size_t theta_bytes = (size_t)B * 3 * cdiv((size_t)G * G * G, TG_CHUNK) * 4 * sizeof(double);
        float *t1 = (float *)((char *)workspace + theta_bytes);          // [B*3][G][G][eW]
        float *t2 = t1 + (size_t)B * 3 * G * G * eW;                     // [B*3][G][eH][eW]
        const size_t n1 = (size_t)B * 3 * G * G * eW, n2 = (size_t)B * 3 * G * eH * eW, n3 = (size_t)B * 3 * eD * eH * eW;
        hipLaunchKernelGGL(resize_adjoint_axis_kernel<false>, dim3(cdiv(n1, 256)), dim3(256), 0, s, dw, t1, (size_t)B * 3 * G * G, eW, G,
                           (size_t)1);
        hipLaunchKernelGGL(resize_adjoint_axis_kernel<false>, dim3(cdiv(n2, 256)), dim3(256), 0, s, (const float *)t1, t2,
                           (size_t)B * 3 * G, eH, G, (size_t)eW);
        hipLaunchKernelGGL(resize_adjoint_axis_kernel<false>, dim3(cdiv(n3, 256)), dim3(256), 0, s, (const float *)t2, dem,
                           (size_t)B * 3, eD, G, (size_t)eH * eW);
    }
    return check_launch("warp_field_compose_bwd");
}

extern "C" int mphip_rt_theta_bwd(const float *rot, const float *tr, const float *dtheta, float *drot, float *dtr, int B,
                                  int invert, void *stream) {
    MPHIP_REQUIRE(rot && tr && dtheta && drot && dtr, "rt_theta_bwd: null pointer");
    MPHIP_REQUIRE(B > 0, "rt_theta_bwd: bad batch");
    hipLaunchKernelGGL(rt_theta_bwd_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, rot, tr, dtheta, drot, dtr, B,
                       invert);
    return check_launch("rt_theta_bwd");
}
