// Host only: which kernel a precision-1 ("f16x3") conv launch takes, and the sizes of the packs those kernels read.  The dev switches of
// that choice are read here (f16x3_switches) and nowhere else; the launchers dispatch on F16x3Plan.kernel and decide nothing.
#include <stdlib.h>

#include "mphip_conv.h"

namespace mphip {

F16x3Switches f16x3_switches() {
    const auto zero = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
    const auto num = [](const char *name, long unset) { const char *e = getenv(name); return e ? atol(e) : unset; };
    static const F16x3Switches fixed = [&] {   // the "fixed" fields (mphip_conv.h)
        F16x3Switches f{};
        f.old_splits = getenv("MPHIP_F16X3_OLD_SPLITS") != nullptr;
        f.xcd_on = !zero("MPHIP_F16X3_XCD");
        f.wino_nopack = zero("MPHIP_WINOGRAD_PACK");
        f.thirds_off = zero("MPHIP_ROI_THIRDS");
        f.conv_cus = num("MPHIP_CONV_CUS", 256);
        f.gn_epilogue_off = zero("MPHIP_GN_EPILOGUE");
        f.k1_nt = (int)num("MPHIP_F16X3_K1_NT", -1);
        return f;
    }();
    F16x3Switches sw = fixed;
    sw.direct_only = getenv("MPHIP_F16X3_TILE") != nullptr;
    sw.force_splits = (int)num("MPHIP_F16X3_SPLITS", 0);
    sw.no_persist = getenv("MPHIP_F16X3_NO_PERSIST") != nullptr;
    sw.wino_off = zero("MPHIP_WINOGRAD");
    sw.d2_off = zero("MPHIP_WINOGRAD_D2");
    sw.min_tiles_set = getenv("MPHIP_WINOGRAD_MIN_TILES") != nullptr;
    sw.min_tiles = num("MPHIP_WINOGRAD_MIN_TILES", 192);
    const char *pp = getenv("MPHIP_WINO_PP");
    sw.wino_pp = !pp ? 1 : pp[0] == '0' ? 0 : pp[0] == '2' ? 2 : 1;
    sw.k1_ks = (int)num("MPHIP_F16X3_K1_KS", 0);
    sw.k1_min_voxels = num("MPHIP_F16X3_K1_MIN", 1024);
    sw.finish_off = zero("MPHIP_SHORTCUT_FINISH");
    return sw;
}

bool f16x3_supported(const F16x3Switches &sw, int N, int Ci, int Co, int D, int H, int W, int k) {
    if (k == 1)   // the k=1 GEMM kernel: whole 64-voxel wave tiles inside one sample, and enough of them to beat the split-K
                  // fp32 gather kernel (measured: 1024 voxels 29 vs 32 us at B=8, but slower below — B=1 went 1.93 -> 2.11 ms)
        return Ci % F16X3_KC == 0 && Co % F16X3_COT == 0 && ((long)D * H * W) % 64 == 0 && (long)N * D * H * W >= sw.k1_min_voxels &&
               (size_t)N * Ci * D * H * W * 4 < 0x80000000ull;
    return k == 3 && Ci % F16X3_KC == 0 && Co % F16X3_COT == 0 && H % 8 == 0 && W % 8 == 0 && D % 2 == 0 &&
           (size_t)N * Ci * D * H * W * 4 < 0x80000000ull;
}

// ---- pack sizes ----------------------------------------------------------------------------------------------------------------
size_t f16x3_packed_bytes_k1(int Co, int Ci) {
    return 16 + (size_t)(Co / F16X3_COT) * (Ci / F16X3_KC) * K1_SLAB_HALFS * sizeof(_Float16);
}

size_t f16x3_direct_bytes(int Co, int Ci) {   // header + the direct kernel's slabs
    return 16 + (size_t)(Co / F16X3_COT) * (Ci / F16X3_KC) * F16X3_NG * SLAB_HALFS * sizeof(_Float16);
}

// layers that can ever take a transformed-domain kernel get its slabs behind the direct pack (a weight tensor does not know the
// volume it will meet): Ci <= 384 covers G3d's levels 0-2 and Eapp's 3-D tail, +133 % pack bytes on <= 16 MB tensors
static size_t wino_packed_bytes(const F16x3Switches &sw, int Co, int Ci) {
    // (Ci <= 768: G3d's 2x8x8 level — 384 / 768 channels — takes the two-frame mode of the big-tile kernel, r06; the LDS table of the fused
    //  input GroupNorm limits the 4-plane kernels to Ci <= 384 only when the norm is fused, checked at launch)
    if (sw.wino_nopack || Ci % WN_KC || Co % WN_COT || Ci > 2 * WN_AFF_CI) return 0;
    return (size_t)(Co / WN_COT) * (Ci / WN_KC) * WN_NG * WN_SLAB_HALFS * sizeof(_Float16);
}
size_t f16x3_wino_packed_bytes(int Co, int Ci) { return wino_packed_bytes(f16x3_switches(), Co, Ci); }

size_t f16x3_packed_bytes(int Co, int Ci) {   // ... + the transformed-domain slabs of the layers that can take those kernels
    return f16x3_direct_bytes(Co, Ci) + f16x3_wino_packed_bytes(Co, Ci);
}

// ---- the planner ---------------------------------------------------------------------------------------------------------------
// split-K only when the launch cannot give every resident workgroup slot a workgroup (each split adds a slab write + a reduce pass): the
// largest whole-chunk split that still fits the chip in ONE round of `slots` resident workgroups.
// r03 sweep (tools/sweep_conv_plans.py): a second round costs more than it hides (B=8, 384->192 @4x16x16: 256 workgroups 98 us,
// 512 106 us), and below that one chunk per workgroup beats three (B=1, 768->384 @2x8x8: 16 splits 41 us, 48 splits 24 us — the
// launch is one workgroup's serial chain of chunks).
static int split_k(long base, int nchunks, long slots) {
    int sp = 1;
    if (base < slots)
        for (int dv = 2; dv <= nchunks; ++dv)
            if (nchunks % dv == 0 && base * dv <= slots) sp = dv;
    return sp;
}

// tiles of an F(2,3) launch: 4 x 8 x 8 voxels of one frame, or — depth-2 volumes, the two-frame mode — 2 x 8 x 8 voxels of TWO frames
static long wino_tiles(int N, int D, int H, int W) {
    return D == 2 ? (long)((N + 1) / 2) * (H / WN_TH) * (W / WN_TW) : (long)N * (D / WN_TD) * (H / WN_TH) * (W / WN_TW);
}

// split-K factor with which an F(2,3) kernel takes the launch, 0 = the direct kernels take it
static int wino_splits(const F16x3Switches &sw, int N, int Ci, int Co, int D, int H, int W, bool roi) {
    if (sw.direct_only || sw.wino_off || wino_packed_bytes(sw, Co, Ci) == 0 || H % WN_TH || W % WN_TW) return 0;
    if (D == 2) {
        // the two-frame mode takes whole launches only (demand-driven launches of a depth-2 volume stay on the direct kernel).
        // two frames per tile: a single frame leaves half of every tile empty — B = 1, 768 -> 768: 31.6 us against the direct kernel's
        // 28.8; from B = 4, the training shard, the mode wins: tools/d2_check.py.  (MPHIP_WINOGRAD_MIN_TILES, whatever its value, lifts
        // that batch rule: the tests reach the mode at small batches with it.)
        if (roi || sw.d2_off || (N < 4 && !sw.min_tiles_set)) return 0;
    } else if (D % WN_TD || Ci > WN_AFF_CI) {   // (the 4-plane kernels keep r05's range: their launches may fuse the input GroupNorm through the LDS table)
        return 0;
    }
    // one workgroup per CU, ~1 us per (kd,kh) slab: worth it when the launch (with its split-K factor) fills the chip and the direct
    // kernel's advantage — a 512-voxel tile's weight economy, thirds of a tile per CU — does not apply (measured: tools/wino_check.py).
    // Demand-driven launches of depth % 4 == 0 volumes follow the full launch's choice, so that the tiles they compute carry the same bits.
    const long base = wino_tiles(N, D, H, W) * (Co / WN_COT);
    const int sp = split_k(base, Ci / WN_KC, 256);
    return base * sp >= sw.min_tiles ? sp : 0;
}

F16x3Plan f16x3_plan(const F16x3Switches &sw, int N, int Ci, int Co, int D, int H, int W, bool roi, bool half_products) {
    F16x3Plan p{};
    const int cot = Co / F16X3_COT, nchunks = Ci / F16X3_KC;
    long tiles;
    p.tile[1] = p.tile[2] = 8;
    p.tile_list = true;
    p.max_gn_ci = F16X3_AFF_CI;
    p.wgs_per_cu = 1;
    if (const int wsp = wino_splits(sw, N, Ci, Co, D, H, W, roi)) {
        // MPHIP_WINO_PP: 0 the lockstep kernel (r04), 1 the role-split kernel (r05), 2 the big-tile kernel (r06: one wave per SIMD;
        // bit-identical to 1).  The one-product (autocast) arithmetic exists on the role-split schedule only; the two-frame mode exists in
        // the big-tile kernel only (three-product arithmetic under the autocast policy as well: this level is 4 % of the slice's multiplies)
        p.kernel = D == 2 ? F16X3_WINO_TWO_FRAME : (sw.wino_pp == 2 && !half_products) ? F16X3_WINO_BIG_TILE
                 : sw.wino_pp != 0 ? F16X3_WINO_ROLE_SPLIT : F16X3_WINO_LOCKSTEP;
        p.one_product = half_products && p.kernel == F16X3_WINO_ROLE_SPLIT;
        p.tile[0] = WN_TD;
        if (p.kernel == F16X3_WINO_TWO_FRAME) {
            p.gn_rows = 0;
            p.tile_list = false;
        } else {
            p.gn_rows = 2;   // one row per plane pair
            p.max_gn_ci = WN_AFF_CI;
        }
        tiles = wino_tiles(N, D, H, W);
        p.splits = wsp;
    } else {
        // the direct kernels: (td,8,8) tile, 256 / 128 voxels per workgroup.  (Until r05 a (4,8,16) tile, 512 voxels per workgroup, the
        // r02-r03 kernel of the chip-filling launches, was kept as the fallback of MPHIP_WINOGRAD=0; it was the one hot instantiation with
        // scratch (248-256 B) and every launch it could take is an F(2,3) kernel's: removed.)
        const int td = D % 4 == 0 ? 4 : 2;
        p.kernel = td == 4 ? F16X3_DIRECT_4 : F16X3_DIRECT_2;
        p.tile[0] = td;
        p.gn_rows = td == 4 ? 8 : 4;   // = the kernel's waves
        p.wgs_per_cu = td == 4 ? 1 : 2;   // (LDS: two workgroups of the 4-wave (2,8,8) kernel fit a CU)
        tiles = (long)N * (D / td) * (H / 8) * (W / 8);
        const long base = tiles * cot;
        int sp = 1;
        if (sw.old_splits) {
            if (base < 256)
                while (base * sp < 512 && nchunks / (sp * 2) >= 3) sp *= 2;
        } else {
            sp = split_k(base, nchunks, 256 * p.wgs_per_cu);
        }
        if (sw.force_splits > 0 && nchunks % sw.force_splits == 0) sp = sw.force_splits;   // (whole chunks per split only)
        p.splits = sp;
    }
    p.chunks_per_split = (nchunks + p.splits - 1) / p.splits;
    p.grid = dim3((unsigned)tiles, (unsigned)cot, (unsigned)p.splits);
    return p;
}

}  // namespace mphip
