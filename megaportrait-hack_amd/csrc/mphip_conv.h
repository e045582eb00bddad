// Shared by every conv translation unit (conv3d.hip: exact fp32 kernels + C ABI; conv3d_f16x3*.hip and their planner; the backward
// conv), api.hip / plan.hip and the GroupNorm code (norm.hip): buffer-load helpers, the pack / tile layout constants, the plan, the launch
// contracts.
#pragma once
#include <hip/hip_ext.h>

#include "mphip_common.h"

namespace mphip {

constexpr unsigned OOB = 0x80000000u;  // >= num_records -> buffer load returns 0 (zero padding)

__device__ __forceinline__ float buf_load_f(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 0));
}

typedef float mphip_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mphip_f32x4 buf_load_f4(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
    return __builtin_bit_cast(mphip_f32x4, (u32x4_)__builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0));
}

// Pack layout of the precision-1 weights: what the size helpers and the planner (conv3d_f16x3_plan.hip) share with the kernels.
constexpr int F16X3_KC = 16;              // input channels per chunk = K of one MFMA
constexpr int F16X3_TG = 3;               // taps per packed weight slab
constexpr int F16X3_NG = 27 / F16X3_TG;   // slabs per 16-channel chunk
constexpr int F16X3_COT = 96;             // output channels per workgroup (3 MFMA row tiles)
constexpr int SLAB_HALFS = 2 * F16X3_TG * 2 * F16X3_COT * 8;  // [part][tap][kg][co][8] = 9216 halfs = 18432 B
constexpr int K1_SLAB_HALFS = 2 * 2 * F16X3_COT * 8;   // [part][kg][co][8] = 3072 halfs = 6 KB per (co tile, chunk)
constexpr int F16X3_AFF_CI = 768;         // fused input GroupNorm table of the direct and two-frame kernels (their AFF_MAX_CI)
// F(2,3) kernels (conv3d_f16x3_wino*.hip): THE definition of their pack and tile; mphip_wino_tile.h derives its byte-unit PP_* values from these
constexpr int WN_KC = 16;                                  // input channels per chunk = K of one MFMA
constexpr int WN_COT = 96;                                 // output channels per workgroup (3 MFMA row tiles)
constexpr int WN_NG = 9;                                   // (kd,kh) slabs per chunk
constexpr int WN_SLAB_HALFS = 2 * 4 * 2 * WN_COT * 8;      // [part][position][kg][co][8] = 12288 halfs = 24576 B
constexpr int WN_TD = 4, WN_TH = 8, WN_TW = 8;             // output tile
constexpr int WN_AFF_CI = 384;                             // fused input GroupNorm table: Ci <= 384 (LDS: 98304 + 61952 + 3072 B + the range fold's 68)

// ---- conv3d_f16x3_plan.hip: the one place that decides which kernel a precision-1 launch takes ------------------------------------
// Dev switches of the choice and of the launch geometry, read by f16x3_switches() and nowhere else.  "per call": read from the
// environment by every f16x3_switches() (tests and tools flip these in-process).  "fixed": read by the first f16x3_switches() of the
// process and kept (set them before the first conv query or launch).
struct F16x3Switches {
    bool direct_only;      // per call  MPHIP_F16X3_TILE (set to anything): the direct kernels only
    int force_splits;      // per call  MPHIP_F16X3_SPLITS=n: split-K factor of a DIRECT launch when n divides the chunk count (F(2,3) launches ignore it)
    bool no_persist;       // per call  MPHIP_F16X3_NO_PERSIST (set): one workgroup per tile — direct launches only
    bool wino_off;         // per call  MPHIP_WINOGRAD=0: no F(2,3) launches (packs keep the slabs)
    bool d2_off;           // per call  MPHIP_WINOGRAD_D2=0: no two-frame launches
    bool min_tiles_set;    // per call  MPHIP_WINOGRAD_MIN_TILES (set to anything): lifts the two-frame mode's N >= 4 rule ...
    long min_tiles;        // per call  ... and its value is the workgroup count from which an F(2,3) kernel takes a launch (default 192)
    int wino_pp;           // per call  MPHIP_WINO_PP: 0 lockstep, 2 big tile (without half products), anything else / unset 1 = role-split
    int k1_ks;             // per call  MPHIP_F16X3_K1_KS=1|4|8: waves sharing a tile of the k = 1 kernel (0 = the rule)
    long k1_min_voxels;    // per call  MPHIP_F16X3_K1_MIN: voxels from which the k = 1 kernel takes a launch (default 1024)
    bool finish_off;       // per call  MPHIP_SHORTCUT_FINISH=0: the k = 1 shortcut conv does not finish its ResBlock3D (the separate apply pass)
    bool old_splits;       // fixed     MPHIP_F16X3_OLD_SPLITS (set): r02's split-K rule on direct launches
    bool xcd_on;           // fixed     MPHIP_F16X3_XCD=0 clears it: the hardware's round-robin tile placement
    bool wino_nopack;      // fixed     MPHIP_WINOGRAD_PACK=0: packs carry no F(2,3) slabs (so no launch takes those kernels)
    bool thirds_off;       // fixed     MPHIP_ROI_THIRDS=0: demand-driven (4,8,8) launches run whole tiles
    long conv_cus;         // fixed     MPHIP_CONV_CUS=n: CUs a persistent grid fills (default 256)
    bool gn_epilogue_off;  // fixed     MPHIP_GN_EPILOGUE=0: GroupNorm statistics by a pass of their own
    int k1_nt;             // fixed     MPHIP_F16X3_K1_NT=1|2: column tiles per wave of the k = 1 kernel (-1 = the rule)
};
F16x3Switches f16x3_switches();

enum F16x3Kernel {
    F16X3_DIRECT_2,         // conv3d_f16x3.hip, (2,8,8) tile, 4 waves, two workgroups per CU
    F16X3_DIRECT_4,         // conv3d_f16x3.hip, (4,8,8) tile, 8 waves ("thirds" of it on demand-driven launches)
    F16X3_WINO_LOCKSTEP,    // conv3d_f16x3_wino.hip: F(2,3), the r04 schedule (A/B reference)
    F16X3_WINO_ROLE_SPLIT,  // conv3d_f16x3_wino_pp.hip: F(2,3), the default of depth % 4 == 0 volumes
    F16X3_WINO_BIG_TILE,    // conv3d_f16x3_wino_bt.hip: F(2,3), one wave per SIMD (A/B; three-product arithmetic only)
    F16X3_WINO_TWO_FRAME,   // conv3d_f16x3_wino_bt.hip: its mode for depth-2 volumes, a tile = 2 planes of two frames
};
inline bool f16x3_is_wino(F16x3Kernel k) { return k >= F16X3_WINO_LOCKSTEP; }

// The whole decision for one 3x3x3 launch; every consumer (workspace sizes, launch, statistics) reads these fields.
struct F16x3Plan {
    F16x3Kernel kernel;
    int tile[3];            // output tile (d,h,w) a tile index of grid.x stands for (two-frame: the granule of the 4-plane kernels)
    int gn_rows;            // GroupNorm-partial rows the kernel leaves per tile, 0 = none (separate statistics pass)
    bool tile_list;         // accepts a demand-driven tile list
    bool one_product;       // the autocast arithmetic (one f16 product per multiply): the role-split kernel under the half-products flag
    int max_gn_ci;          // largest Ci with a fused input GroupNorm
    int wgs_per_cu;         // resident workgroups per CU (the persistent grid and the split-K rule count 256 CUs of them)
    int splits, chunks_per_split;
    dim3 grid;              // logical grid: tiles, output-channel tiles, splits
};
F16x3Plan f16x3_plan(const F16x3Switches &sw, int N, int Ci, int Co, int D, int H, int W, bool roi, bool half_products);

bool f16x3_supported(const F16x3Switches &sw, int N, int Ci, int Co, int D, int H, int W, int k);
size_t f16x3_direct_bytes(int Co, int Ci);   // header + the direct kernel's slabs: where the F(2,3) slabs begin
size_t f16x3_packed_bytes(int Co, int Ci);
size_t f16x3_packed_bytes_k1(int Co, int Ci);
int f16x3_launch_k1(const F16x3Switches &sw, const float *x, const void *wpacked, const float *bias, float *dst, int N, int Ci, int Co,
                    int DHW, const float *x_range, hipStream_t s);
void f16x3_k1_plan_query(const F16x3Switches &sw, int N, int Ci, int Co, int DHW, int out[5]);   // f16x3_k1_geometry, for the debug query
// the k = 1 launch that finishes its ResBlock3D: relu(GN(y2) + conv(x)) (+ AvgPool3d(2)) and the range descriptor of the result (mphip_gn.h)
struct GnParams;
bool f16x3_k1_finish_supported(const F16x3Switches &sw, int N, int Ci, int Co, int D, int H, int W, int groups, int pool2);
int f16x3_launch_k1_finish(const F16x3Switches &sw, const float *x, const void *wpacked, const float *bias, int N, int Ci, int Co, int D, int H,
                           int W, const float *x_range, const GnParams &fin, int pool2, hipStream_t s);
int f16x3_pack(const float *w_oidhw, void *out, int Co, int Ci, int k, int transposed, const void *header_from, hipStream_t s);
// Batched re-packing (mphip_pack_table_*): one launch per kernel kind for every weight of a module.  PackJob is the device-side job
// (the public mphip_pack_job + what the host resolved); PackSel a launch's selection: indices into the job array and the first block
// of each selected job (n + 1 entries), both device arrays.
struct PackJob {
    const float *w;
    void *wp;
    const void *like;      // precision 1: a pack of the same weight whose header (max|w|) is reused, or nullptr
    size_t wino_off;       // precision 1, k = 3: byte offset of the F(2,3) slabs in wp, 0 = none
    int Co, Ci, k, precision, transposed, reserved;
};
struct PackSel {
    const int *job;
    const int *first;
    int n, blocks;
};
int f16x3_pack_blocks(const PackJob &j, int kind /* 0 absmax, 1 k = 3 pack, 2 k = 1 pack */);
size_t f16x3_pack_wino_offset(int Co, int Ci);
int f16x3_pack_many(const PackJob *jobs, PackSel absmax, PackSel k3, PackSel k1, hipStream_t s);
// roi (optional): 8 ints per box {lx,ly,lz,ex,ey,ez,-,-}: only the output tiles a box touches are computed (roi_frames == 0: one box per
// frame; > 0: the conv's frames... single frame serves that many boxes)
int f16x3_launch(const F16x3Switches &sw, const F16x3Plan &p, const float *x, const void *wpacked, const float *bias, float *dst, int N, int Ci,
                 int Co, int D, int H, int W, const float *in_affine, int in_relu, const float *x_range, hipStream_t s,
                 const int *roi = nullptr, int roi_frames = 0, int *tile_list = nullptr /* 1 + plan.grid.x ints when roi */, int roi_dilate = 0,
                 float *gn_part = nullptr /* [Co][plan.grid.x][plan.gn_rows][2]: per-wave (sum, sumsq) of the output, splits == 1 only */,
                 hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr /* stamped with the conv kernel's own begin / end */);

// A kernel launch whose begin / end are stamped on t0 / t1 when both are given (the measurement hook's events ride on the kernel command
// itself, so what another stream's kernel makes the launch WAIT for CUs is not counted as its duration).  The argument types must be the
// kernel's parameter types.
template <class K, class... A>
void launch_timed(K kern, dim3 grid, dim3 block, hipStream_t s, hipEvent_t t0, hipEvent_t t1, A... args) {
    if (t0 && t1) hipExtLaunchKernelGGL(kern, grid, block, 0, s, t0, t1, 0, args...);
    else hipLaunchKernelGGL(kern, grid, block, 0, s, args...);
}

// The parameters of the 3x3x3 f16x3 forward kernels, in kernarg order (the direct kernels take one more, roi_frames, before gn_part);
// f16x3_launch fills it once.
struct F16x3ConvArgs {
    const float *x;
    const _Float16 *slabs;
    const float *hdr, *bias;
    float *dst;
    int N, Ci, Co, D, H, W, cps;
    unsigned xb;
    const float *in_affine;
    int in_relu;
    const float *x_range;
    int tiles, xcd_on;
    const int *tile_list;   // demand-driven: {count, tile ids} or NULL
    float *gn_part;
};
template <class K>
void f16x3_wino_launch_kernel(K kern, dim3 grid, dim3 block, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const F16x3ConvArgs &a) {
    launch_timed(kern, grid, block, s, t0, t1, a.x, a.slabs, a.hdr, a.bias, a.dst, a.N, a.Ci, a.Co, a.D, a.H, a.W, a.cps, a.xb, a.in_affine,
                 a.in_relu, a.x_range, a.tiles, a.xcd_on, a.tile_list, a.gn_part);
}

// The same split-f16 arithmetic in the 1-D Winograd F(2,3) domain (2/3 of the MFMAs).  Its slabs live behind the direct slabs of a
// precision-1 k=3 pack (0 bytes when the layer can never take an F(2,3) kernel).  Three kernels, one contract; f16x3_launch picks among
// them by F16x3Plan.kernel.  Each unit keeps a saturation counter (f16x3_counter_read).
size_t f16x3_wino_packed_bytes(int Co, int Ci);
// conv3d_f16x3_wino.hip: lockstep schedule (A/B reference)
void f16x3_wino_launch(dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const F16x3ConvArgs &a);
int f16x3_wino_saturation(unsigned long long *count, int reset);
// conv3d_f16x3_wino_pp.hip: role-split ("ping-pong") schedule
void f16x3_wino_pp_launch(dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const F16x3ConvArgs &a, bool half_products);
int f16x3_wino_pp_saturation(unsigned long long *count, int reset);
// conv3d_f16x3_wino_bt.hip: one wave per SIMD and a 96 x 128 register tile (three-product arithmetic only); results bit-identical to
// the role-split kernel's
void f16x3_wino_bt_launch(dim3 grid, hipStream_t s, hipEvent_t t0, hipEvent_t t1, const F16x3ConvArgs &a, bool two_frame);
int f16x3_wino_bt_saturation(unsigned long long *count, int reset);
// conv2d_f16x3.hip: the 2-D 3x3 conv (mphip_conv2d_fwd) keeps a counter of its own as well
int conv2d_f16x3_saturation(unsigned long long *count, int reset);
// conv2d_gn_f16x3.hip: its two-source form (mphip_conv2d_cat_fwd), likewise
int conv2d_gn_f16x3_saturation(unsigned long long *count, int reset);
// conv2d_lp.hip: the typed and one-product instantiations of both (mphip_conv2d_fwd_typed, mphip_conv2d_cat_fwd_typed), likewise
int conv2d_lp_saturation(unsigned long long *count, int reset);
// conv2d_s2_f16x3.hip: the stride-2 form (mphip_conv2d_s2_fwd), likewise
int conv2d_s2_saturation(unsigned long long *count, int reset);
// conv2d_up2_f16x3.hip: the two forms with a bilinear x2 up-sample folded in (mphip_conv2d_up2_fwd, mphip_conv2d_resup2_fwd), likewise
int conv2d_up2_saturation(unsigned long long *count, int reset);
// conv2d_grp_f16x3.hip: the grouped form (mphip_conv2d_grouped_fwd), likewise
int conv2d_grp_saturation(unsigned long long *count, int reset);
// conv2d_splitk_f16x3.hip: the split-K form (mphip_conv2d_split_fwd, splits > 1), likewise
int conv2d_split_saturation(unsigned long long *count, int reset);
// conv2d_pw_f16x3.hip: the pointwise (1x1) form (mphip_conv2d_pw_fwd), likewise
int conv2d_pw_saturation(unsigned long long *count, int reset);
// conv2d_stem7_f16x3.hip: the 7x7 stem (mphip_conv2d_stem7_fwd), likewise
int conv2d_stem7_saturation(unsigned long long *count, int reset);

// The forms of the 2-D conv (3x3 but for the last): what conv2d_run's table (conv2d_run.hip) is indexed by.  One C entry each, the first
// two a typed one too.
enum C2Form {
    C2_PLAIN,    // one source; x1, residual and y in their dtypes, one product or three
    C2_CAT,      // the two-source kernels (also with C2 == 0: they are kernels of their own); fp32 sources, typed residual and y
    C2_S2,       // conv2d_s2_f16x3.hip: stride 2; y and residual are [N,Co,(H+1)/2,(W+1)/2]
    C2_UP2,      // conv2d_up2_f16x3.hip: the source is up2(x1), x1 and H, W the LOW-resolution map, y and residual [N,Co,2H,2W]
    C2_RESUP2,   // conv2d_up2_f16x3.hip: the residual is up2(r), r [N,Co,H/2,W/2], H and W even
    C2_GROUPED,  // conv2d_grp_f16x3.hip: x1 [N,C1,H,W] in `groups` groups, the pack that of a [Co,C1/groups,3,3] weight; 1: the plain kernel
    C2_SPLIT,    // conv2d_splitk_f16x3.hip: the grouped form with the reduction in `splits` K ranges that leave partial maps in the
                 // workspace, behind the descriptor slot, and a finish launch; 1: the grouped form's launch
    C2_PW,       // conv2d_pw_f16x3.hip: a 1x1 conv at `stride` 1 or 2 with a pack of its own; y and residual are
                 // [N,Co,(H+stride-1)/stride,(W+stride-1)/stride]
    C2_FORMS
};
// One call of the 2-D conv, as its ten C entries describe it to conv2d_run.  Zero-initialised it is the plain fp32 three-product
// call: one source (C2 = 0, no tables), fp32 dtypes (MPHIP_DTYPE_F32 == 0); only `products` = 0 asks for the thread's policy.  Every
// form but the first two is one source, fp32 maps and three products (c2_call_f32).
struct C2Call {
    const char *who;        // the entry's name, for messages
    C2Form form;
    int groups, splits;     // the caller's counts (C2_GROUPED, C2_SPLIT), as they came: the form's shape rule refuses what is below 1
    int stride;             // the caller's stride (C2_PW), as it came: the form's shape rule refuses what is neither 1 nor 2
    const void *x1, *x2;    // sources [N,C1,H,W] and [N,C2,H,W] or NULL; x1 in x_dtype (fp32 when C2_CAT), x2 fp32
    const float *aff1, *aff2, *x1_range, *x2_range;
    int relu1, relu2, C1, C2;
    int x_dtype, residual_dtype, y_dtype;
    int products;           // 3, 1, or 0 = the calling thread's policy flag; conv2d_run resolves it to 3 or 1 for the launchers
    const void *w_packed;
    const float *bias;
    const void *residual;
    void *y;
    float *out_range;
    int N, Co, H, W, relu;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t stream;
};
// the call of an fp32, one-source, three-product entry; a typed or two-source entry sets its dtypes, product count and second source on top
inline C2Call c2_call_f32(const char *who, C2Form form, const void *x, const float *x_range, const void *w_packed, const float *bias,
                          const void *residual, void *y, float *out_range, int N, int Ci, int Co, int H, int W, int relu, void *workspace,
                          size_t workspace_bytes, void *stream) {
    C2Call c{};
    c.who = who, c.form = form;
    c.x1 = x, c.x1_range = x_range, c.C1 = Ci;
    c.x_dtype = c.residual_dtype = c.y_dtype = MPHIP_DTYPE_F32, c.products = 3;
    c.w_packed = w_packed, c.bias = bias, c.residual = residual, c.y = y, c.out_range = out_range;
    c.N = N, c.Co = Co, c.H = H, c.W = W, c.relu = relu;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = (hipStream_t)stream;
    return c;
}
struct C2Grid {
    dim3 grid;
    int tiles_w, tiles_h;   // (C2_PW: tiles_w tiles of the flat pixel index per image, tiles_h = 1)
    unsigned nslots;        // partial maxima of out_range
    float *part;            // C2_SPLIT with c.splits > 1: c.splits maps of y's size in the workspace; else NULL
};
// the workspace: one library-computed range descriptor per source that comes without one (C2_SPLIT: its partial maps behind them)
inline size_t c2_workspace_bytes(int descriptors) { return (size_t)descriptors * MPHIP_RANGE_FLOATS * sizeof(float); }
// conv2d_run.hip: validate, carve the workspace, scan the ranges, size the grid, initialise out_range, launch: in this order, for every entry
int conv2d_run(C2Call c);
// each unit's launcher of its instantiations (c.products resolved, every range in place)
void conv2d_plain_launch(const C2Call &c, const C2Grid &g);   // conv2d_f16x3.hip: conv2d_k3_f16x3_kernel
void conv2d_cat_launch(const C2Call &c, const C2Grid &g);     // conv2d_gn_f16x3.hip: conv2d_k3_cat_f16x3_kernel
void conv2d_lp_launch(const C2Call &c, const C2Grid &g);      // conv2d_lp.hip: the one-product kernels of C2_PLAIN and C2_CAT
void conv2d_s2_launch(const C2Call &c, const C2Grid &g);      // conv2d_s2_f16x3.hip: conv2d_k3s2_f16x3_kernel
void conv2d_up2_launch(const C2Call &c, const C2Grid &g);     // conv2d_up2_f16x3.hip: conv2d_k3_up2_f16x3_kernel / conv2d_k3_resup2_f16x3_kernel
void conv2d_grouped_launch(const C2Call &c, const C2Grid &g); // conv2d_grp_f16x3.hip: conv2d_k3_grp_f16x3_kernel; c.groups == 1: the plain launch
void conv2d_split_launch(const C2Call &c, const C2Grid &g);   // conv2d_splitk_f16x3.hip: its two launches; g.part == NULL: the grouped launch
void conv2d_pw_launch(const C2Call &c, const C2Grid &g);      // conv2d_pw_f16x3.hip: conv2d_pw_f16x3_kernel; one grid dimension, channel tile fastest
// conv2d_s2_f16x3.hip: its output tile (64 channels x 8 rows x 16 columns per workgroup) and its shape rule (H, W: the input map)
constexpr int C2S2_TH = 8, C2S2_TW = 16;
bool c2_s2_supported(int N, int Ci, int Co, int H, int W);
// conv2d_pw_f16x3.hip: its tile (64 channels x 256 consecutive output pixels of an image per workgroup) and its shape rule (H, W: the
// input map; stride 1 or 2)
constexpr int C2PW_PIX = 256;
bool c2_pw_supported(int N, int Ci, int Co, int H, int W, int stride);
// conv2d_up2_f16x3.hip: the shape rule of its up-sampled-source form (h, w: the LOW-resolution input map): c2_supported on [2h, 2w]
bool c2_up2_supported(int N, int Ci, int Co, int h, int w);
// conv2d_grp_f16x3.hip: its shape rule: groups >= 1 and c2_supported; groups > 1: Ci and Co multiples of groups, (Ci / groups) % 16 == 0,
// (Co / groups) % 64 == 0
bool c2_grouped_supported(int N, int Ci, int Co, int H, int W, int groups);
// conv2d_splitk_f16x3.hip: its shape rule: c2_grouped_supported, 1 <= splits <= C2_MAX_SPLITS, ((Ci / groups) / 16) % splits == 0; the
// constants of mphip_conv2d_splits; the workgroups of its finish launch over ny = N * Co * H * W elements (one
// out_range slot each, up to RANGE_MAX_PARTS)
constexpr int C2_MAX_SPLITS = 16;
constexpr int C2_SPLIT_MAX_S = 8, C2_SPLIT_MIN_CHUNKS = 2, C2_SPLIT_MAX_WG = 512, C2_SPLIT_MIN_K = 8, C2_SPLIT_MAX_UNSPLIT_WG = 128;
bool c2_split_supported(int N, int Ci, int Co, int H, int W, int groups, int splits);
unsigned c2_split_finish_blocks(size_t ny);

// api.hip: the calling thread's conv arithmetic policy (mphip_conv3d_set_half_products): true inside torch.autocast(float16) regions
bool conv_half_products();

// conv3d_bwd_f16x3.hip: 3x3x3 backward-weight on the f16 matrix cores (split precision)
bool bwd_weight_f16x3_supported(int N, int Ci, int Co, int D, int H, int W, int k);
// the one decision of a launch: the launcher, the workspace size and mphip_debug_conv3d_bwd_weight_f16x3_plan all read it
struct BwdWeightF16x3Plan {
    int kernel;   // 0 = the shape is not supported, 1 = the 3x3x3 kernel, 2 = the 1x1x1 kernel
    int splits;   // slabs = grid z; the slab reduce folds them in order
    int tps;      // voxel tiles per split (the last split may hold fewer)
    int ntiles;   // voxel tiles of the launch: N x (2,8,8) tiles (k = 3), N x 128-voxel tiles (k = 1)
    int bxy;      // (ci, co) blocks = grid x
};
BwdWeightF16x3Plan bwd_weight_f16x3_plan(int N, int Ci, int Co, int D, int H, int W, int k);
size_t bwd_weight_f16x3_ws_bytes(int N, int Ci, int Co, int D, int H, int W, int k);
int bwd_weight_f16x3_launch(const float *x, const float *x_range, const float *dy, const float *dy_scale, float *dw, int N, int Ci,
                            int Co, int D, int H, int W, int k, void *workspace, hipStream_t s, const int *dy_boxes = nullptr);

// norm.hip: GroupNorm statistics of x [N,C,S] -> stats [N*G][2] (workspace sized by groupnorm_ws_bytes)
// GnTable (optional): the statistics kernels also write what mphip_groupnorm_affine_table would — table[n][c] = (scale, shift) of the
// norm folded into the NEXT conv's staging and the data-independent range descriptor of the normalised tensor — with the same
// arithmetic, saving that launch on the dependent chain (one per residual block).
struct GnTable {
    const float *gamma = nullptr, *beta = nullptr, *w2 = nullptr, *b2 = nullptr;
    float *table = nullptr, *range = nullptr;
    int C = 0, cpg = 0;
    float sqrt_ng = 0.0f;
};
size_t groupnorm_ws_bytes(int N, int C, int S, int G);
int groupnorm_stats_launch(const float *x, float *stats, int N, int C, int S, int G, float eps, void *workspace,
                           hipStream_t s, const GnTable *tbl = nullptr);
// ... from the per-(tile, wave, channel) partial sums (of value - bias) an f16x3 conv launch left in part [C][N*tiles_per_frame][waves][2]
// y: the conv's stored output, re-read for a group whose epilogue moments are ill-conditioned (|mean| >> sigma)
int groupnorm_stats_from_tiles(const float *part, const float *bias, const float *y, float *stats, int N, int C, int S, int G, float eps,
                               int tiles_per_frame, int waves, hipStream_t s, const GnTable *tbl = nullptr);

}  // namespace mphip
