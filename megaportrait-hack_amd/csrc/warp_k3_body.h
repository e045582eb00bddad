// Body of K3 (warp.hip: warp_gather_dsum_kernel<CPB> and warp_gather_dsum_typed_kernel<CPB, DTO>), included inside both kernels so that
// the fp32 kernel's code is exactly what it was before the typed one existed.  No include guard: it is included twice on purpose.
// The including kernel defines K3_STORE(x): the value stored for the fp32 sum x (fp32: x; typed: narrow<DTO>(x), rounded once).
    __shared__ __attribute__((aligned(16))) float lds[STAGE_FLOATS];
    __shared__ int red[24];
    const int HW = H * W;
    const int tiles_w = (W + K3_TW - 1) / K3_TW, tiles_h = (H + K3_TH - 1) / K3_TH, ntile = tiles_w * tiles_h;
    // XCD-aware order: the tiles of one (frame, channel slice) are consecutive logical ids, i.e. they run on ONE XCD at about the
    // same time — w-neighbours share every 128-byte line of a source row, h-neighbours the halo rows, and with the hardware's
    // round-robin (tile t -> XCD t % 8) each of those lines was fetched into up to four different L2s (travelling fields: 5x the
    // algorithmic bytes crossed the fabric, at 6.9 TB/s — the kernel's limit)
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = (int)(bid % ntile); bid /= ntile;
    const int slices = (C + CPB - 1) / CPB;
    const int slice = (int)(bid % slices), b = (int)(bid / slices);
    static_assert(K3_TH * K3_TW == 256, "one thread per position of the tile");
    const int h = (tile / tiles_w) * K3_TH + (int)(threadIdx.x / K3_TW);
    const int w = (tile % tiles_w) * K3_TW + (int)(threadIdx.x % K3_TW);
    const bool active = h < H && w < W;
    const int p = h * W + w;
    const size_t vol = (size_t)D * HW;
    const int c0 = slice * CPB;
    const int cs = min(CPB, C - c0);
    const int cs_pad = lds_pitch_for(cs);
    const float *cp = coords + ((size_t)b * D * HW + (active ? p : 0)) * 3;
    const float *vb = v + (size_t)b * v_frame_stride;

    float acc[CPB];
#pragma unroll
    for (int c = 0; c < CPB; ++c) acc[c] = 0.0f;

    int lx = INT_MAX, ly = INT_MAX, lz = INT_MAX, hx = 0, hy = 0, hz = 0;
    if (active) {
        for (int d = 0; d < D; ++d) {
            const float *q = cp + (size_t)d * HW * 3;
            int x = (int)floorf(q[0]), y = (int)floorf(q[1]), z = (int)floorf(q[2]);
            lx = min(lx, x); ly = min(ly, y); lz = min(lz, z);
            hx = max(hx, x); hy = max(hy, y); hz = max(hz, z);
        }
    }
    const Box all = block_box(lx, ly, lz, hx, hy, hz, D, H, W, red);
    if (all.ex * all.ey * all.ez * cs_pad <= STAGE_FLOATS) {  // block-uniform: everything in one [voxel][channel] image
        stage_box(vb, lds, all, c0, cs, cs_pad, H, W, vol);
        __syncthreads();
        if (active) {
            for (int d = 0; d < D; ++d) {
                const float *q = cp + (size_t)d * HW * 3;
                Coord3 cc{q[0], q[1], q[2]};
                Taps t = make_taps(cc, D, H, W);
                const TapOff lt = rebase(t, (int)floorf(cc.x), (int)floorf(cc.y), (int)floorf(cc.z), all, cs_pad);
#pragma unroll
                for (int c = 0; c < CPB; c += 4) {
                    if (c + 4 <= cs) {
                        float tmp[4];
                        gather8x4(lds + c, lt, t.w, tmp);
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[c + k] += tmp[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c + k < cs) acc[c + k] += gather8_lds(lds + c + k, lt, t.w);
                    }
                }
            }
        }
    } else if (active) {
        // a field that travels through the volume: gather from global memory; lanes run along w (coalesced row segments for
        // a smooth field, the per-CU L1 serves the overlap between taps), x-neighbour taps in pairs
        for (int d = 0; d < D; ++d) {
            const float *q = cp + (size_t)d * HW * 3;
            const Taps t = make_taps(Coord3{q[0], q[1], q[2]}, D, H, W);
#pragma unroll
            for (int c = 0; c < CPB; ++c)
                if (c < cs) acc[c] += W >= 2 ? gather8_pairs(vb + (size_t)(c0 + c) * vol, t) : gather8(vb + (size_t)(c0 + c) * vol, t);
        }
    }
    if (!active) return;
#pragma unroll
    for (int c = 0; c < CPB; ++c)
        if (c < cs) out[((size_t)b * C + c0 + c) * HW + p] = K3_STORE(acc[c]);
