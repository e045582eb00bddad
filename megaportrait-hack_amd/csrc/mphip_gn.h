// The per-element arithmetic of a GroupNorm apply pass, shared by norm.hip's apply kernels and by the conv epilogues that finish a block with
// the same expression (conv3d_f16x3.hip: the 1x1x1 shortcut conv).  One definition, so the fused and the separate form give the same bits.
#pragma once
#include "mphip_common.h"

namespace mphip {

struct GnParams {
    const float *x, *stats, *gamma, *beta, *w2, *b2, *residual;
    float *y;
    int C, cpg;
    int relu, tanh_;
    float *range;  // optional: range descriptor of y (zeroed by the launcher; max|y| is folded in — the next conv's f16x3 scale)
};

__device__ __forceinline__ float gn_value(const GnParams &p, float xv, float mean, float rstd, float g, float b,
                                          float w2, float b2, bool has2, float res, bool has_res) {
    float v = (xv - mean) * rstd * g + b;
    if (has2) v = v * w2 + b2;
    if (has_res) v += res;
    if (p.relu) v = fmaxf(v, 0.0f);
    if (p.tanh_) v = tanhf(v);
    return v;
}


// host side, defined in warp.hip: mphip_groupnorm_apply(no second affine, relu = 1, tanh = 0, pool2 = 1) whose residual is the output of the
// K2 that ran on `coords` with the corner image `img` and left its per-tile marks in `todo`.  The residual is rebuilt from the image
// wherever K2 took it from there (gn_apply_pool_warp_kernel) and loaded elsewhere: bitwise the plain launch.  _ok: whether the kernel
// covers the shape.
bool gn_apply_pool_warp_ok(int N, int C, int D, int H, int W, int G);
int gn_apply_pool_warp_launch(const float *x, const float *stats, const float *gamma, const float *beta, const float *residual, float *y,
                              float *out_range, const float *coords, const int *todo, const float *img, int N, int C, int D, int H, int W, int G,
                              hipStream_t s);

}  // namespace mphip
