// What the F(2,3) conv kernels do OUTSIDE their schedules, once for conv3d_f16x3_wino.hip (lockstep) and _bt.hip (big tile); the role-split
// kernel keeps its own text of the same code (see its header): the output transform of a column tile through the exchange region, the GroupNorm partials, the 16-byte store pattern and the
// saturation count.  The kernels keep their own loops, barriers and store addresses (the counted vmcnt waits depend on where every store
// sits); the arithmetic and the layouts below are what has to stay bit-equal across them (tests hold the three torch.equal).
#pragma once
#include "mphip_f16x3.h"

namespace mphip {

// Exchange region: [pair0 + position][slot 0..5][lane][4] floats (pair0 = 4 * plane pair where two pairs share one region, else 0).  The four Winograd positions of an output pair live in four
// waves; per 32-channel row tile a wave (position P) parks the three quarters ("units": accumulator registers 4u..4u+3 of both column
// tiles a[0], a[1]) that the other waves finish and keeps unit P.  (P: a constant in the kernels instantiated per position, the wave's
// run-time position in the lockstep kernel — there every unit goes through a select.)
__device__ __forceinline__ void wino_park_units(const int P, const f32x16 *a, float *Ex, int pair0, int lane) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u != P) {
                const int slot = t * 3 + (u - (u > P ? 1 : 0));
                const f32x4 v = {a[t][4 * u], a[t][4 * u + 1], a[t][4 * u + 2], a[t][4 * u + 3]};
                *reinterpret_cast<f32x4 *>(Ex + (((pair0 + P) * 6 + slot) * 64 + lane) * 4) = v;
            }
}
// ... and, a barrier later, collects M[0..3] of ITS unit of column tile t: three from the other positions' slots, one from its own registers
__device__ __forceinline__ void wino_gather_M(const int P, const f32x16 &a, const float *Ex, int pair0, int lane, int t, f32x4 (&M)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q != P) {
            const int slot = t * 3 + (P - (P > q ? 1 : 0));
            M[q] = *reinterpret_cast<const f32x4 *>(Ex + (((pair0 + q) * 6 + slot) * 64 + lane) * 4);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) M[q][i] = a[4 * q + i];
        }
    }
}

// F(2,3) output transform of one output pair x 4 channels: y[2q] = (M0 + M1) + M2, y[2q+1] = (M1 - M2) - M3 (this association, in fp32),
// the GroupNorm partial sums of the RAW transformed values (gn: uniform), `* unscale + bias`, and the half swap for the stores:
// a lane holds one output pair (2 voxels) of 4 channels; lanes 2k / 2k+1 hold neighbouring pairs of a row and trade halves (quad_perm
// [1,0,3,2]): the even lane ends up with 4 consecutive voxels of channels 0-1 (va: channel 0 / 2, vb: channel 1 / 3), the odd lane with
// those of channels 2-3 — two dwordx4 stores per lane instead of four dwordx2 (the epilogue is store-ISSUE bound: 8-byte stores of
// 32-byte row pieces ran at ~7 B/clk/CU, MI355X_MICROARCH.md "epilogue store tail").
template <class B>
__device__ __forceinline__ void wino_out_pair(const f32x4 (&M)[4], const B &bv, Unscale us, bool odd, bool gn, float (&ssum)[4],
                                              float (&qsum)[4], f32x4 &va, f32x4 &vb) {
    float y0[4], y1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float r0 = (M[0][i] + M[1][i]) + M[2][i];
        const float r1 = (M[1][i] - M[2][i]) - M[3][i];
        if (gn) {
            ssum[i] += r0 + r1;
            qsum[i] = __builtin_fmaf(r0, r0, qsum[i]);
            qsum[i] = __builtin_fmaf(r1, r1, qsum[i]);
        }
        y0[i] = unscaled(r0, us, bv[i]);
        y1[i] = unscaled(r1, us, bv[i]);
    }
    auto swap = [](float v) { return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0xB1, 0xf, 0xf, false)); };
    const float g0 = swap(odd ? y0[0] : y0[2]), g1 = swap(odd ? y1[0] : y1[2]);
    const float g2 = swap(odd ? y0[1] : y0[3]), g3 = swap(odd ? y1[1] : y1[3]);
    va = f32x4{odd ? g0 : y0[0], odd ? g1 : y1[0], odd ? y0[2] : g0, odd ? y1[2] : g1};
    vb = f32x4{odd ? g2 : y0[1], odd ? g3 : y1[1], odd ? y0[3] : g2, odd ? y1[3] : g3};
}

// GroupNorm partials of one round: per-channel (sum, sum of squares) of the RAW transformed accumulators over this wave's 2 x 64 voxels
// of the channel — the 32 lanes of a half-wave hold one channel's columns (the finalize kernel applies unscale and the bias in double).
// Layout: channel-major [Co][tile * 2 + plane pair][2] floats (the finalize kernel reads rows of it), `unscale` in the word behind them.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void wino_dpp_add(float &v) {   // v += v of the lane CTRL names
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ void wino_gn_halfwave_sum(float (&ssum)[4], float (&qsum)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // row_ror:8, :4, :2, :1 -> every lane of a 16-lane row: the row's sum
        wino_dpp_add<0x128>(ssum[i]); wino_dpp_add<0x128>(qsum[i]);
        wino_dpp_add<0x124>(ssum[i]); wino_dpp_add<0x124>(qsum[i]);
        wino_dpp_add<0x122>(ssum[i]); wino_dpp_add<0x122>(qsum[i]);
        wino_dpp_add<0x121>(ssum[i]); wino_dpp_add<0x121>(qsum[i]);
        // rows 1 and 3 add the totals of rows 0 and 2 (row_bcast:15, row mask 0b1010): lanes 16-31 / 48-63 hold a half-wave's sum
        wino_dpp_add<0x142, 0xa>(ssum[i]);
        wino_dpp_add<0x142, 0xa>(qsum[i]);
    }
}
// co: the first of this half-wave's four channels; row = tile * 2 + plane pair; j = lane & 31
__device__ __forceinline__ void wino_gn_write(float *gn_part, int gn_rows, int co, size_t row, int j, float (&ssum)[4], float (&qsum)[4]) {
    wino_gn_halfwave_sum(ssum, qsum);
    if (j == 31) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float2 *>(gn_part + ((size_t)(co + i) * gn_rows + row) * 2) = make_float2(ssum[i], qsum[i]);
    }
}
__device__ __forceinline__ void wino_gn_write_unscale(float *gn_part, int gn_rows, int Co, float unscale) {
    gn_part[(size_t)gn_rows * Co * 2] = unscale;
}

// Operands outside the f16 range (non-finite inputs, or finite ones beyond a wrong caller-supplied descriptor) are not clamped — they
// propagate as Inf / NaN — but they are counted, per thread that saw any (the direct kernel counts elements): one atomic per wave.
__device__ __forceinline__ void wino_count_saturated(bool sat, unsigned long long *counter, int lane) {
    if (__builtin_amdgcn_ballot_w64(sat) != 0) {  // never taken in normal operation
        unsigned tot = sat;
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) tot += __shfl_xor(tot, sft, 64);
        if (lane == 0) atomicAdd(counter, (unsigned long long)tot);
    }
}

}  // namespace mphip
