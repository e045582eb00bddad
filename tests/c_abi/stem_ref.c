/* Plain-C statement of mphip_conv2d_stem_fwd's contract (include/mphip.h), for tests/test_gpu_conv2d_stem.py:
 * acc = +0; fmaf(w, x, acc) over ci, dy, dx in that order (padded taps skipped: the same bits as a multiply by 0 for finite weights);
 * one rounded + bias; ReLU: negative values and zeros -> +0, NaN kept; the 3x3 stride-2 max over the positions inside the map, NaN wins.
 * Build: gcc -O1 -ffp-contract=off -shared -fPIC stem_ref.c -lm */
#include <math.h>

static float conv_at(const float *x, const float *w, float bias, int H, int W, int r, int s, int relu) {
    float acc = 0.0f;
    for (int ci = 0; ci < 3; ++ci)
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) {
                const int yy = r + dy - 1, xx = s + dx - 1;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc = fmaf(w[(ci * 3 + dy) * 3 + dx], x[((long)ci * H + yy) * W + xx], acc);
            }
    float v = acc + bias;
    if (relu && v <= 0.0f) v = 0.0f;
    return v;
}

void stem_ref(const float *x, const float *w, const float *bias, float *y, int N, int Co, int H, int W, int relu, int pool) {
    const int Ho = pool ? (H + 1) / 2 : H, Wo = pool ? (W + 1) / 2 : W;
    for (int n = 0; n < N; ++n)
        for (int co = 0; co < Co; ++co)
            for (int i = 0; i < Ho; ++i)
                for (int j = 0; j < Wo; ++j) {
                    const float *xn = x + (long)n * 3 * H * W, *wc = w + (long)co * 27;
                    float m = 0.0f;
                    if (!pool) {
                        m = conv_at(xn, wc, bias[co], H, W, i, j, relu);
                    } else {
                        int first = 1;
                        for (int a = 0; a < 3; ++a)
                            for (int b = 0; b < 3; ++b) {
                                const int r = 2 * i + a - 1, s = 2 * j + b - 1;
                                if (r < 0 || r >= H || s < 0 || s >= W) continue;
                                const float v = conv_at(xn, wc, bias[co], H, W, r, s, relu);
                                if (first || (m == m && (v > m || v != v))) m = v;
                                first = 0;
                            }
                    }
                    y[(((long)n * Co + co) * Ho + i) * Wo + j] = m;
                }
}
