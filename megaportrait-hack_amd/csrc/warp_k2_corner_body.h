// Body of K2's corner gather (warp.hip: warp_gather_kernel and warp_gather_typed_kernel<DT>), included inside both kernels so that
// the fp32 kernel's code is exactly what it was before the typed one existed.  No include guard: it is included twice on purpose.
// The including kernel defines K2_MAYBE(cond): whether the tile may lie in the corner the image holds (fp32: `cond`, the test of the
// tile's first sample; typed: always — the typed kernel has no fp32 volume to stage from, it brings the image in for every tile).
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
    const float *c0p = coords + (((size_t)b * D + d) * HW + (size_t)(tile / tiles_w) * K2_TH * W + (tile % tiles_w) * K2_TW) * 3;
    const float fx = c0p[0], fy = c0p[1], fz = c0p[2];
    const bool maybe = K2_MAYBE(fx >= 0.0f && fx < (float)(K2_CORNER_E - 1) && fy >= 0.0f && fy < (float)(K2_CORNER_E - 1) && fz >= 0.0f && fz < (float)(K2_CORNER_E - 1));
    const bool dma = maybe && img != nullptr;
#ifndef MPHIP_K2_ABL_NOSTAGE   /* dev ablations (timing only, wrong results): tools/k2_ablate.sh */
    if (dma) k2_dma_image(img + ((size_t)b * gridDim.y + blockIdx.y) * k2_block_floats(cg), lds, (int)k2_block_floats(cg));
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
    // 0: done here; 1: a box of moderate size = a smooth field that travels -> warp_gather_columns_body (plane reuse down the
    // slices); 2: no locality to exploit (a box like the whole volume) -> warp_gather_direct_body (most loads in flight)
    if (threadIdx.x == 0 && blockIdx.y == 0) todo[bid] = in_corner ? 0 : (bx.ex * bx.ey * bx.ez <= K2_COLUMNS_MAX_BOX ? 1 : 2);
    unsigned mbits = 0;
    if (dma) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the image have landed
    if (in_corner) {
        float *ob = out + (size_t)b * C * vol + (size_t)d * HW + p0;
#ifndef MPHIP_K2_ABL_NOSTAGE
        if (!dma) k2_stage_corner(v + (size_t)b * C * vol, lds, cg0, Cg, cgp, D, H, W);
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
                k2_f2 pv[2][8];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int k = 0; k < 8; ++k) pv[i][k] = *reinterpret_cast<const k2_f2 *>(src + tb[i][k]);   // (even pitch, even channel: 8-byte aligned)
                k2_f2 acc[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    acc[i] = k2_f2{0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[i] = k2_pk_add(acc[i], k2_pk_mul<0>(pv[i][2 * j], wp[i][j]));
                        acc[i] = k2_pk_add(acc[i], k2_pk_mul<1>(pv[i][2 * j + 1], wp[i][j]));
                    }
                }
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
