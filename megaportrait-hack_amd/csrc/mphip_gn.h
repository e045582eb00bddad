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

}  // namespace mphip
