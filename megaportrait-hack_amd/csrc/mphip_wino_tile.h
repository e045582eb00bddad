// Shared by the two F(2,3) conv kernels that use the 4x8x8-voxel tile, the 8-channel X double buffer and the [part][position][kg][co][8]
// weight slabs: conv3d_f16x3_wino_pp.hip (role-split schedule, r05) and conv3d_f16x3_wino_bt.hip (one wave per SIMD, r06).  Tile
// geometry, the LDS map, the walk over tiles and 16-channel periods (WinoStream), the LDS-DMA source mapping, the hand-issued halo loads,
// the input transform and the hi/lo split helpers — one definition, so that the two kernels stay byte-compatible (same packs, same staged
// X image, bit-identical results).  The byte-unit PP_* values are derived from the pack / tile constants of mphip_conv.h (WN_*), which the
// packer, the planner and the lockstep kernel use.  What a kernel does after its K loop is in mphip_wino_epilogue.h.
#pragma once
#include "mphip_conv.h"
#include "mphip_f16x3.h"
#include "mphip_wino_epilogue.h"

namespace mphip {

constexpr int PP_COT = WN_COT;
constexpr int PP_R = 3;                                   // slabs in the ring
constexpr int PP_SLAB_B = WN_SLAB_HALFS * 2;              // [part][position][kg][co][8] f16 = 24576 B
constexpr int PP_WPART_B = PP_SLAB_B / 2;
constexpr int PP_KGBLK_B = PP_COT * 16;                   // one (part, position, kg) block: 1536 B
constexpr int PP_TD = WN_TD, PP_TH = WN_TH, PP_TW = WN_TW;
constexpr int PP_HH = PP_TH + 2;
constexpr int PP_ROWS = (PP_TD + 2) * PP_HH;              // 60 halo rows
constexpr int PP_XPOS_B = PP_ROWS * 4 * 16;               // (part, position) block: 240 (pair, row) slots x 8 channels = 3840 B
// Inside a (part, position) block the slots are PAIR-major: [output pair 0..3][halo row 0..59][8 channels] (r06).  A staging thread owns
// (channel pair, row) and writes 4 bytes per (position, pair): with rows 16 bytes apart the 64 lanes of a wave (4 channel pairs x 16 rows)
// cover 64 consecutive banks.  r05's row-major form ([row][pair]: rows 64 bytes apart) made every one of those stores a 4-way bank
// conflict — ALL of the kernel's 17.3 M conflict cycles per launch, 28 % of its LDS-active cycles (profiles/NOTES_r06.md).  The
// fragment reads (16 bytes per lane, lane = (row j >> 2, pair j & 3)) stay conflict-free: the 16 lanes the LDS serves together hold 4 rows
// x 4 pairs, whose first banks (48 pair + 4 row) mod 64 are 16 different multiples of 4.
constexpr int PP_XROW_B = 16;                             // halo row to halo row
constexpr int PP_XPAIR_B = PP_ROWS * PP_XROW_B;           // output pair to output pair: 960 B
constexpr int PP_XPART_B = 4 * PP_XPOS_B;
constexpr int PP_XBUF_B = 2 * PP_XPART_B;                 // one 8-channel buffer: 30720 B
constexpr int PP_EX_B = 4 * 6 * 64 * 16;                  // one team's exchange round: 24576 B
constexpr int PP_AFF_CI = WN_AFF_CI;
constexpr int PP_LDS_X = PP_R * PP_SLAB_B;
constexpr int PP_LDS_EX = PP_LDS_X + 2 * PP_XBUF_B;
constexpr int PP_LDS_AFF = PP_LDS_EX + PP_EX_B;
constexpr int PP_LDS_BIAS = PP_LDS_AFF + PP_AFF_CI * 2 * 4;   // the workgroup's 96 bias values (read by the epilogue through LDS: a global
                                                              // load there would make hipcc wait vmcnt(0) — for the previous round's stores)
constexpr int PP_LDS_BYTES = PP_LDS_BIAS + PP_COT * 4;
static_assert(PP_XBUF_B >= PP_EX_B, "team B's exchange lives in X buffer 1");
static_assert(PP_LDS_BYTES <= 163840 - 128, "LDS");
static_assert(WN_KC == 16 && WN_NG == 9, "a period = 16 channels = 9 steps of two (8-channel chunk, tap) items");

__device__ constexpr int pp_rowoff(int tap) { return (tap / 3) * PP_HH + tap % 3; }   // halo-row offset of a (kd,kh) tap

// hi/lo split helpers as single instructions (hipcc has no builtin for either and, left alone, SLP-packs the surrounding fp32 arithmetic
// into v_pk_*_f32 — an anti-lever beside MFMAs, MI355X_MICROARCH.md — and converts hi back with two v_cvt_f32_f16):
//   pp_cvt_pk: {rne_f16(a), rne_f16(b)};  pp_sub_lo / pp_sub_hi: t - (float)h.lo / h.hi, the f16 read in place (exact: one rounding)
__device__ __forceinline__ unsigned pp_cvt_pk(float a, float b) {
    unsigned r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float pp_sub_lo(unsigned h, float t) {
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(t));
    return r;
}
__device__ __forceinline__ float pp_sub_hi(unsigned h, float t) {
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(t));
    return r;
}

// Halo loads, hidden from hipcc's waitcnt pass on purpose.  The two teams run ONE program half a period apart and share the staging
// registers: with compiler-visible loads the pass sees team A's pending loads on the path where team B transforms ITS (long landed) row and
// puts `s_waitcnt vmcnt(0)` there — team B then drains the LDS-DMA pieces it issued a moment ago, ~1 us in every write phase (and vice
// versa).  Ordering is by hand instead: the counted wait that ends each LOAD phase leaves only the newest operations in flight, so a
// unit's loads have landed two phases before its first use (cdna_hip_programming.md 5.7: no use of the destination before that wait,
// every phase ends in a sched_barrier; the kernel stays below the VGPR limit without spills, so no live range is split or copied).
typedef unsigned pp_u32x4 __attribute__((ext_vector_type(4)));
// (one statement per group of loads, opened by `s_nop 4` for the descriptor — see pp_dma3; early-clobber outputs: a destination must not
//  share a register with the address of a later load of the same statement)
__device__ __forceinline__ void pp_buf_load_2x4(pp_u32x4 rsrc, unsigned o0, unsigned o1, f32x4 &r0, f32x4 &r1) {
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %2, %4, 0 offen\n\tbuffer_load_dwordx4 %1, %3, %4, 0 offen"
                 : "=&v"(r0), "=&v"(r1) : "v"(o0), "v"(o1), "s"(rsrc) : "memory");
}
__device__ __forceinline__ void pp_buf_load_4x1(pp_u32x4 rsrc, unsigned o0, unsigned o1, unsigned o2, unsigned o3, float &r0, float &r1, float &r2, float &r3) {
    asm volatile("s_nop 4\n\tbuffer_load_dword %0, %4, %8, 0 offen\n\tbuffer_load_dword %1, %5, %8, 0 offen\n\t"
                 "buffer_load_dword %2, %6, %8, 0 offen\n\tbuffer_load_dword %3, %7, %8, 0 offen"
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(o0), "v"(o1), "v"(o2), "v"(o3), "s"(rsrc) : "memory");
}

__device__ __forceinline__ void pp_buf_load_1x4(pp_u32x4 rsrc, unsigned o0, f32x4 &r0) {
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, 0 offen" : "=&v"(r0) : "v"(o0), "s"(rsrc) : "memory");
}
__device__ __forceinline__ void pp_buf_load_2x1(pp_u32x4 rsrc, unsigned o0, unsigned o1, float &r0, float &r1) {
    asm volatile("s_nop 4\n\tbuffer_load_dword %0, %2, %4, 0 offen\n\tbuffer_load_dword %1, %3, %4, 0 offen"
                 : "=&v"(r0), "=&v"(r1) : "v"(o0), "v"(o1), "s"(rsrc) : "memory");
}

struct PpPeriod {   // what a 16-channel period of the K stream addresses (wave-uniform)
    int n, d0, h0, w0, chunk, tj;
};

// A persistent workgroup's walk: tiles j_first, j_first + stride, ... of the launch (or of the demand-driven list {count, id, id, ...}),
// per tile the 16-channel chunks [c_begin, c_end) of its split, per chunk nine weight slabs of the output-channel tile at `wbytes`.
// D2 (the big-tile kernel's two-frame mode): a tile = the frame pair (2 bid, 2 bid + 1) of a depth-2 volume.
struct WinoStream {
    const int *tile_list;
    int tiles_w, tiles_h, tiles_d, c_begin, c_end, stride;
    const unsigned char *wbytes;
    __device__ __forceinline__ int tile_at(int jj) const { return tile_list ? tile_list[1 + jj] : jj; }
    template <bool D2 = false>
    __device__ __forceinline__ PpPeriod period_at(int tj, int chunk) const {
        PpPeriod r;
        int bid = tile_at(tj);
        const int tw = bid % tiles_w; bid /= tiles_w;
        const int th = bid % tiles_h; bid /= tiles_h;
        if constexpr (D2) { r.n = 2 * bid; r.d0 = 0; }
        else { r.n = bid / tiles_d; r.d0 = (bid % tiles_d) * PP_TD; }
        r.h0 = th * PP_TH; r.w0 = tw * PP_TW;
        r.chunk = chunk; r.tj = tj;
        return r;
    }
    template <bool D2 = false>
    __device__ __forceinline__ PpPeriod period_next(const PpPeriod &a) const {   // (only called when a successor exists)
        if (a.chunk + 1 < c_end) { PpPeriod r = a; r.chunk = a.chunk + 1; return r; }
        return period_at<D2>(a.tj + stride, c_begin);
    }
    __device__ __forceinline__ const unsigned char *wchunk(int chunk) const { return wbytes + (size_t)chunk * 9 * PP_SLAB_B; }
};

// raw buffer descriptor (base, stride 0, num_records = bytes, 32-bit float data format): out-of-range offsets read 0 = the padding
__device__ __forceinline__ pp_u32x4 wino_rsrc(const void *base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)(uintptr_t)base;
    return pp_u32x4{(unsigned)a, (unsigned)(a >> 32) & 0xffffu, bytes, 0x00020000u};
}

// LDS-DMA source of the 16 bytes a lane writes at byte `o` of a slab image: they lie in k-group block (part, position, kg) = o / 1536 at
// channel (o % 1536) / 16; the source is the same (part, position, channel) of k-group block item / 9 of the pack's slab (chunk16,
// item % 9), item = 2 * step + kg.  Lanes of k-group block kg = 1 read one slab (24576 B) further than those of kg = 0 — item 2s+1 is the
// next tap of the same k-group of the pack — except at step 4, where item 8 is (tap 8, k-group 0) and item 9 (tap 0, k-group 1): two
// per-lane offset sets (dsrc, dsrc4), no per-step address arithmetic (the step's tap goes into the scalar base, wino_dma_base).
__device__ __forceinline__ void wino_dma_src(unsigned o, unsigned &dsrc, unsigned &dsrc4) {
    const unsigned blk = o / PP_KGBLK_B;
    const bool kg1 = (blk & 1u) != 0;
    const unsigned in_slab = (blk >> 1) * (2u * PP_KGBLK_B) + (o - blk * PP_KGBLK_B);
    dsrc = in_slab + (kg1 ? (unsigned)PP_SLAB_B : 0u);
    dsrc4 = in_slab + (kg1 ? (unsigned)PP_KGBLK_B : 8u * PP_SLAB_B);
}
__device__ constexpr unsigned wino_dma_base(int sq) {   // (tap, k-group) of item 2 sq, as a byte offset into the period's slabs
    return sq == 4 ? 0u : ((2 * sq) % 9) * PP_SLAB_B + ((2 * sq) / 9) * PP_KGBLK_B;
}

// The fused input GroupNorm's table [Ci][2] (scale, shift) of frame n: by the whole workgroup (prologue) ...
__device__ __forceinline__ void wino_load_aff(float *aff, const float *in_affine, int n, int Ci, int first, int stride) {
    for (int i = first; i < Ci * 2; i += stride) aff[i] = in_affine[(size_t)n * Ci * 2 + i];
}
// ... and for another frame as LDS-DMA (ONE wave, up to three pieces of 1 KiB; lanes beyond the table are masked off): nothing in the main
// loops is a compiler-visible load, so hipcc never waits vmcnt(0) in them
__device__ __forceinline__ void wino_dma_aff(const float *in_affine, int n, int Ci, int lane, unsigned aff_lds) {
    const unsigned char *const src = reinterpret_cast<const unsigned char *>(in_affine + (size_t)n * Ci * 2);
    const int bytes = Ci * 8;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (i * 1024 < bytes && lane * 16 + i * 1024 < bytes)
            asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"((unsigned)(lane * 16 + i * 1024)), "s"(src), "s"(aff_lds + i * 1024) : "memory");
}

// range diagnostic of two staged values: one v_max3 (|a|, |b|, m) and one unordered compare (v_max drops NaNs)
__device__ __forceinline__ void wino_note(float a, float b, float &xmaxf, bool &xnan) {
    xmaxf = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a), __builtin_fabsf(b)), xmaxf);
    xnan |= __builtin_isunordered(a, b);
}

// voxel i (0..9 = w0-1 .. w0+8) of a staged halo row (i folds: the callers' output pair is a constant) and the F(2,3) input transform of
// output pair q at Winograd position pp (fp32, after the operand scale)
__device__ __forceinline__ float wino_row_at(int i, float xl, const f32x4 &xa, const f32x4 &xb, float xr) {
    return i == 0 ? xl : i <= 4 ? xa[i - 1] : i <= 8 ? xb[i - 5] : xr;
}
__device__ __forceinline__ float wino_in_transform(int pp, int q, float xl, const f32x4 &xa, const f32x4 &xb, float xr) {
    auto v = [&](int i) { return wino_row_at(i, xl, xa, xb, xr); };
    return pp == 0 ? v(2 * q) - v(2 * q + 2) : pp == 1 ? v(2 * q + 1) + v(2 * q + 2) : pp == 2 ? v(2 * q + 2) - v(2 * q + 1) : v(2 * q + 1) - v(2 * q + 3);
}

// X fragment bases (LDS bytes) of a lane.  The two k-groups of step sp read items 2sp and 2sp+1 — one halo row apart (+16 B), eight rows
// apart (tap (kd,2) -> (kd+1,0): +128 B), or (step 4) the last tap of buffer 0 and the first of buffer 1: three per-lane bases, the step's
// own offset (off0) is an immediate.
struct WinoXBases {
    unsigned b_row, b_plane, b_buf;
    __device__ __forceinline__ WinoXBases(unsigned b_lane, int kgl)
        : b_row(b_lane + (unsigned)kgl * PP_XROW_B), b_plane(b_lane + (unsigned)kgl * (8u * PP_XROW_B)),
          b_buf(b_lane + (unsigned)kgl * (unsigned)(PP_XBUF_B - pp_rowoff(8) * PP_XROW_B)) {}
    static constexpr unsigned off(int item) { return (item / 9) * PP_XBUF_B + pp_rowoff(item % 9) * PP_XROW_B; }
    template <int SP>
    __device__ __forceinline__ unsigned base() const {   // (without off(2 SP))
        constexpr unsigned dist = off(2 * SP + 1) - off(2 * SP);
        static_assert(dist == PP_XROW_B || dist == 8 * PP_XROW_B || dist == PP_XBUF_B - pp_rowoff(8) * PP_XROW_B, "k-group distance");
        return dist == PP_XROW_B ? b_row : dist == 8 * PP_XROW_B ? b_plane : b_buf;
    }
};

// A tile's preamble: the accumulators, and an opaque 0 that is new per tile — added to the epilogue's channel index it keeps the per-channel
// address math / bias loads from being hoisted out of the tile loop into registers (where they were spilled to scratch)
template <int T>
__device__ __forceinline__ int wino_tile_begin(f32x16 (&acc)[3][T]) {
    int tz = 0;
    asm volatile("" : "+v"(tz));
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;
    return tz;
}

}  // namespace mphip
