// Conv2d 3x3 (stride 1, padding 1) on the f16 matrix cores with fp32-class accuracy: the "f16x3" split of conv3d_f16x3.hip on NCHW
// maps, with the epilogue G2d's ResBlock2D needs at inference (BatchNorm folded into weights and bias by the caller):
//     y = act( conv(x, w) + bias[co] (+ residual[n,co,h,w]) ),   act = ReLU or identity
//
// Arithmetic (the 3-D direct kernel's): each operand tensor is scaled by its own power of two and split v*S = hi + lo with split_f16;
// the product is Wlo*Xhi + Whi*Xhi + Whi*Xlo in the fp32 accumulator of v_mfma_f32_32x32x16_f16; the accumulator is unscaled (by 1/scale_w,
// then by 1/scale_x: two powers of two, each exact; their single product can underflow) and bias, residual and ReLU are applied in fp32.  Out-of-range and non-finite inputs are not clamped (split_f16), they
// are counted in this unit's saturation counter, which mphip_f16x3_saturation_count sums with the others.
//
// Tile: a workgroup of 4 waves computes 64 output channels x (16 rows x 16 columns); a wave owns all 64 channels of 4 rows = 2 x 2
// MFMA tiles (64 accumulator registers), so one tap costs 8 fragment reads for 12 MFMAs.  Per 16-channel chunk the workgroup stages
//   the 18 x 18 halo tile, split while staging:      [part][kg][pixel][8] f16 = 20736 B   (zero padding lives in the masked loads)
//   the chunk's packed 9-tap weight slab:            [part][tap][kg][co][8] f16 = 36864 B
// = 57600 B of LDS, single buffered: two workgroups share a CU (2 waves per SIMD, 256 registers each) and one computes while the
// other stages; inside a workgroup the next chunk's global loads are issued before the current chunk's MFMAs and written to LDS
// after them.  Fragment reads are 16-byte and conflict-free: weights are co-contiguous, and a 16-lane ds_read_b128 group reads one
// whole 16-pixel row (the lane -> pixel slot permutation of the 3-D kernel).
//
// MFMA operand layout (conv3d_f16x3.hip): A = weights [32 co x 16 ci], B = pixels [16 ci x 32 px]; lane l holds k = 8*(l>>5)..+7 of
// row / column l&31; C: column = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
#include "conv2d_f16x3_tile.h"   // the constants, the shape rule and the tile code (shared with conv2d_gn_f16x3.hip)

namespace mphip {

__device__ unsigned long long g_conv2d_saturated;

// ---- weight packing: header (16 B, the 3-D pack's: [0] 1/scale [1] scale [2] max|w| bits [3] unused), then the slabs ---------------
__global__ void __launch_bounds__(256) conv2d_absmax_kernel(const float *__restrict__ w, size_t n, unsigned *__restrict__ hdr) {
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(w[i]));
    unsigned b = wave_umax(__float_as_uint(m));   // (non-negative floats order like their bits)
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        b = max(max(red[0], red[1]), max(red[2], red[3]));
        if (b > __hip_atomic_load(hdr + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hdr + 2, b);
    }
}

// one thread = one 16-byte fragment (8 consecutive ci of one co and tap), hi and lo; output channels past Co are zeros.
// transposed: Co, Ci are the PACK's (the conv it serves maps Ci -> Co) and w is the OIHW weight [Ci][Co][3][3] of the conv whose
// backward-data that is: element (co, ci, tap) is w[ci][co][8 - tap], the flipped, transposed weight.
__global__ void __launch_bounds__(256)
conv2d_pack_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, const unsigned *__restrict__ hdr_in, float *__restrict__ hdr_out,
                   int Co, int Ci, int total, int transposed) {
    const float scale = weight_scale(hdr_in[2]);
    const int nchunks = Ci / C2_KC;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        const int co = i % C2_COT;
        int r = i / C2_COT;
        const int kg = r % 2; r /= 2;
        const int tap = r % 9; r /= 9;
        const int chunk = r % nchunks;
        const int cot = r / nchunks;
        const int cog = cot * C2_COT + co;
        half8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = chunk * C2_KC + kg * 8 + e;
            const float v = cog >= Co ? 0.0f : transposed ? w[((size_t)ci * Co + cog) * 9 + (8 - tap)] : w[((size_t)cog * Ci + ci) * 9 + tap];
            _Float16 h, l;
            split_f16(v * scale, h, l);
            hi[e] = h; lo[e] = l;
        }
        const size_t slab = (size_t)cot * nchunks + chunk;
        const size_t inner = ((size_t)(tap * 2 + kg) * C2_COT + co) * 8;
        *reinterpret_cast<half8 *>(out + slab * C2_SLAB_HALFS + inner) = hi;
        *reinterpret_cast<half8 *>(out + slab * C2_SLAB_HALFS + C2_SLAB_HALFS / 2 + inner) = lo;
    }
    if (i == 0) {
        hdr_out[0] = 1.0f / scale;
        hdr_out[1] = scale;
    }
}

// ---- range descriptors -----------------------------------------------------------------------------------------------------------
// max|x| of the input when the caller hands in no descriptor: one partial maximum per workgroup (any alignment of x)
__global__ void __launch_bounds__(256) conv2d_range_kernel(const float *__restrict__ x, size_t n, float *__restrict__ range) {
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, range_bits(x[i]));
    range_note_block(m, range, blockIdx.x, gridDim.x);
}
// the output's descriptor before the conv fills it: derive mode, `nslots` partial maxima at 0 (the epilogue folds its tiles into them
// with an integer atomicMax on the float's bits: order-independent, so the descriptor is reproducible)
__global__ void __launch_bounds__(256) conv2d_out_range_init_kernel(float *__restrict__ range, unsigned nslots) {
    unsigned *r = reinterpret_cast<unsigned *>(range);
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4) r[i] = i == 3 ? nslots : 0u;
    if (i < nslots) r[4 + i] = 0u;
}

// ---- the conv kernel: the plain instantiation of conv2d_f16x3_tile.h ----------------------------------------------------------------
__global__ void __launch_bounds__(C2_NTHR) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv2d_k3_f16x3_kernel(const float *__restrict__ x, const float *__restrict__ x_range, const _Float16 *__restrict__ wslabs,
                       const float *__restrict__ whdr, const float *__restrict__ bias, const float *__restrict__ residual,
                       float *__restrict__ y, float *__restrict__ out_range, int Ci, int Co, int H, int W, int relu, int tiles_w,
                       int tiles_h, unsigned nslots) {
    conv2d_k3_tile<false, &g_conv2d_saturated>(x, x_range, C2CatArgs{}, wslabs, whdr, bias, residual, y, out_range, Ci, Co, H, W, relu, tiles_w,
                                               tiles_h, nslots);
}

void conv2d_range_launch(const float *x, size_t n, float *range, hipStream_t s) {
    const unsigned blocks = (unsigned)std::min<size_t>(2048, (n + 8191) / 8192);
    hipLaunchKernelGGL(conv2d_range_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, x, n, range);
}
void conv2d_out_range_init_launch(float *range, unsigned nslots, hipStream_t s) {
    hipLaunchKernelGGL(conv2d_out_range_init_kernel, dim3(cdiv(nslots + 4, 256)), dim3(256), 0, s, range, nslots);
}

void conv2d_plain_launch(const C2Call &c, const C2Grid &g) {
    hipLaunchKernelGGL(conv2d_k3_f16x3_kernel, g.grid, dim3(C2_NTHR), 0, c.stream, (const float *)c.x1, c.x1_range,
                       (const _Float16 *)((const char *)c.w_packed + 16), (const float *)c.w_packed, c.bias, (const float *)c.residual,
                       (float *)c.y, c.out_range, c.C1, c.Co, c.H, c.W, c.relu, g.tiles_w, g.tiles_h, g.nslots);
}

int conv2d_f16x3_saturation(unsigned long long *count, int reset) { return f16x3_counter_read(&g_conv2d_saturated, count, reset); }

}  // namespace mphip

using namespace mphip;

extern "C" int mphip_conv2d_supported(int N, int Ci, int Co, int H, int W) { return c2_supported(N, Ci, Co, H, W) ? 1 : 0; }

extern "C" size_t mphip_conv2d_packed_weight_bytes(int Co, int Ci) {
    if (Ci < C2_KC || Co < 32 || Ci % C2_KC || Co % 32) return 0;
    return c2_packed_bytes(Co, Ci);
}

// the pack of w (transposed == 0) or of its flipped transpose; Co, Ci: the pack's
static int pack_conv2d_weight(const char *who, const float *w_oihw, void *w_packed, int Co, int Ci, int transposed, void *stream) {
    MPHIP_REQUIRE(w_oihw && w_packed, "%s: null pointer", who);
    MPHIP_REQUIRE(Ci >= C2_KC && Co >= 32 && Ci % C2_KC == 0 && Co % 32 == 0 && c2_cots(Co) <= 65535,
                  transposed ? "%s: Co = %d, Ci = %d: Co must be a multiple of 16 and Ci a multiple of 32 (the roles swap)"
                             : "%s: Co = %d, Ci = %d: Ci must be a multiple of 16 and Co a multiple of 32",
                  who, transposed ? Ci : Co, transposed ? Co : Ci);
    MPHIP_REQUIRE(((uintptr_t)w_packed & 15) == 0, "%s: w_packed must be 16-byte aligned", who);
    const long long total = (long long)c2_cots(Co) * (Ci / C2_KC) * 9 * 2 * C2_COT;
    MPHIP_REQUIRE(total < (1ll << 31) - 256, "%s: Co = %d, Ci = %d is too large", who, transposed ? Ci : Co, transposed ? Co : Ci);
    hipStream_t s = (hipStream_t)stream;
    zero_fill(w_packed, 16, s);   // header: the absmax kernel accumulates with atomicMax
    const size_t n = (size_t)Co * Ci * 9;
    hipLaunchKernelGGL(conv2d_absmax_kernel, dim3((unsigned)std::min<size_t>(1024, (n + 2047) / 2048)), dim3(256), 0, s, w_oihw, n,
                       (unsigned *)w_packed);
    hipLaunchKernelGGL(conv2d_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w_oihw,
                       (_Float16 *)((char *)w_packed + 16), (const unsigned *)w_packed, (float *)w_packed, Co, Ci, (int)total, transposed);
    return check_launch(who);
}

extern "C" int mphip_pack_conv2d_weight(const float *w_oihw, void *w_packed, int Co, int Ci, void *stream) {
    return pack_conv2d_weight("pack_conv2d_weight", w_oihw, w_packed, Co, Ci, 0, stream);
}

// Co, Ci: those of the conv w_oihw [Co,Ci,3,3] belongs to; the pack is the one of a Co -> Ci conv (mphip_conv2d_packed_weight_bytes(Ci, Co))
extern "C" int mphip_pack_conv2d_weight_bwd_data(const float *w_oihw, void *w_packed, int Co, int Ci, void *stream) {
    return pack_conv2d_weight("pack_conv2d_weight_bwd_data", w_oihw, w_packed, Ci, Co, 1, stream);
}

extern "C" size_t mphip_conv2d_workspace_bytes(int N, int Ci, int Co, int H, int W) {
    return c2_supported(N, Ci, Co, H, W) ? c2_workspace_bytes(1) : 0;   // the library-computed descriptor of x (x_range == NULL)
}

extern "C" int mphip_conv2d_fwd(const float *x, const float *x_range, const void *w_packed, const float *bias, const float *residual,
                                float *y, float *out_range, int N, int Ci, int Co, int H, int W, int relu, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return mphip_conv2d_fwd_typed(x, MPHIP_DTYPE_F32, x_range, w_packed, bias, residual, MPHIP_DTYPE_F32, y, MPHIP_DTYPE_F32, out_range, N, Ci,
                                  Co, H, W, relu, 3, workspace, workspace_bytes, stream);
}
