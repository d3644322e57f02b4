// Weight gradients of the dense projections on the CDNA4 matrix cores: out[n][k] = sum_m dY[m][n] * X[m][k], bf16 or fp16 in (one
// template parameter, as in linear.hip), fp32 accumulate, split over the TOKENS.  C ABI: zigma_linear_wgrad.
//
// Replaces the GEMM autograd's linear backward runs for dW at Mamba.in_proj / x_proj / dt_proj / out_proj (reference mamba_simple.py:290-294,
// selective_scan_interface.py:318-323,365) and CrossAttention.to_q / to_out (model_zigma.py:104-135).  The tokens (m = 65 536 at the headline
// shape) are the CONTRACTION index and both operands are row-major [token][feature]: every MFMA operand is a COLUMN read.
//
//   * tile: 128 features of dY x BK features of X (BK = 128, or 64 where k <= 64 — then the tile covers k whole and dY is read exactly
//     once; n <= 128 is one tile row of the 128-wide form, so X is read exactly once) over one slab of tokens, in steps of 64 tokens.
//     256 threads: 4 waves as 2 (n) x 2 (k), wave tile 64 x BK / 2, v_mfma_f32_32x32x16 with dY as the A operand (D row = n) and X as
//     the B operand (D column = k: the 32 lanes of an accumulator register are 128 contiguous bytes of an output row).
//   * both tiles are staged as they lie in memory, [token][feature] in 16-byte pieces (predicated global loads: rows past the slab and
//     columns past n / k arrive as zeros, so the LDS pad needs no separate fill), one step ahead in registers.
//   * fragments by ds_read_b64_tr_b16, two per fragment: group g = lane >> 4 of read t (0, 1) of k-step s takes the 4 token rows
//     16 s + 8 (g >> 1) + 4 t + q and the 16 features 16 (g & 1) + i — lane (r = l & 31, h = l >> 5) then holds tokens 16 s + 8 h + j of
//     feature r in element j, for A and B alike (the natural assignment).  Row pitch = 64 B (mod 128 B) — 320 B for 128 features, 192 B
//     for 64: the four rows a 32-lane half reads start 64 B apart modulo 256 B, so its 32 8-byte pieces cover the 64 banks exactly once
//     (conflict-free without an XOR).  Every lane's address is a multiple of 8 B; the reads sit in wave-uniform control flow only (EXEC all
//     ones: the loop bounds depend on blockIdx alone, and nothing returns early); the LDS arrays are static and 16-byte aligned.
//   * grid = tiles x S slabs.  S > 1: every workgroup writes its fp32 partial tile into the caller's workspace ([S][n][k], private layout)
//     and wgrad_reduce_kernel adds the S partials in ascending slab order in fp32, rounds once and writes out.  S = 1: the GEMM kernel
//     writes out itself.  No atomics: the result does not depend on timing.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; the build fails on scratch or a spill in any instantiation):
//   wgrad_kernel<bf16 | f16, 128>: 94 VGPR + 64 AGPR, 40 960 B LDS, 3 waves / SIMD (3 workgroups per CU), no scratch
//   wgrad_kernel<bf16 | f16, 64>:  84 VGPR + 32 AGPR, 32 768 B LDS, 4 waves / SIMD (4 workgroups per CU), no scratch
//   wgrad_reduce_kernel:           14 VGPR, no LDS, 8 waves / SIMD, no scratch
#include "wgrad_plan.h"
#include "zigma_common.h"

namespace zigma {

struct wgrad_args_t {
    const uint16_t *dy, *x;
    void *out;            // S == 1: the result (out_f32 ? float : T), pitch out_pitch;  S > 1: the fp32 workspace [S][n][k]
    int64_t dy_pitch, x_pitch, out_pitch;
    int64_t m, slab_rows;
    int32_t n, k, n_tiles, out_f32, direct;
};

typedef short tr_i16x4 __attribute__((ext_vector_type(4)));
typedef short tr_i16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) tr_i16x4 *lds_tr_ptr_t;

// one MFMA operand: 8 consecutive tokens (4 per read) of this lane's feature, from a [token][feature] image
template <typename T> __device__ __forceinline__ frag8_t<T> tr_frag(const unsigned char *lo, const unsigned char *hi) {
    const tr_i16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr_t)(lo));
    const tr_i16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr_t)(hi));
    const tr_i16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(frag8_t<T>, v);
}

// 16-byte pieces of a 64-token x W-feature tile, one step: piece c = tid + 256 i is row c / (W / 8), chunk c % (W / 8)
template <int W> __device__ __forceinline__ void wgrad_fetch(uint4 (&r)[W / 32], const uint16_t *base, const int64_t pitch, const int64_t row0,
                                                            const int64_t row_end, const int col0, const int cols, const int tid) {
    constexpr int CH = W / 8;
#pragma unroll
    for (int i = 0; i < W / 32; ++i) {
        const int c = tid + kWgThreads * i;
        const int64_t row = row0 + c / CH;
        const int col = col0 + (c % CH) * 8;
        uint4 v = {0u, 0u, 0u, 0u};
        if (row < row_end && col < cols) v = *reinterpret_cast<const uint4 *>(base + row * pitch + col);
        r[i] = v;
    }
}

template <int W, int PITCH> __device__ __forceinline__ void wgrad_stage(const uint4 (&r)[W / 32], unsigned char *s, const int tid) {
    constexpr int CH = W / 8;
#pragma unroll
    for (int i = 0; i < W / 32; ++i) {
        const int c = tid + kWgThreads * i;
        *reinterpret_cast<uint4 *>(s + (c / CH) * PITCH + (c % CH) * 16) = r[i];
    }
}

template <typename T, int BK>
__global__ __launch_bounds__(kWgThreads) void wgrad_kernel(const wgrad_args_t p) {
    constexpr int PA = kWgBN * 2 + 64, PB = BK * 2 + 64;          // row pitches: 64 B (mod 128 B)
    constexpr int KB = BK / 64;                                   // 32-column blocks of a wave along k
    __shared__ __attribute__((aligned(16))) unsigned char s_a[kWgKT * PA];
    __shared__ __attribute__((aligned(16))) unsigned char s_b[kWgKT * PB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x % p.n_tiles, tk = blockIdx.x / p.n_tiles, slab = blockIdx.y;
    const int n0 = tn * kWgBN, k0 = tk * BK;
    const int64_t row_begin = slab * p.slab_rows;
    const int64_t row_end = row_begin + p.slab_rows < p.m ? row_begin + p.slab_rows : p.m;

    // transposed-read addresses of this lane: token row q (+ 8 per lane half), features 4 p ... 4 p + 3 of block (g & 1)
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int wn = wave >> 1, wk = wave & 1;
    const int tr_row = 8 * (g >> 1) + q, tr_col = 16 * (g & 1) + 4 * pp;
    const unsigned char *a_rd = s_a + tr_row * PA + (wn * 64 + tr_col) * 2;
    const unsigned char *b_rd = s_b + tr_row * PB + (wk * (BK / 2) + tr_col) * 2;

    mfma_f32x16 acc[2][KB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    uint4 ra[kWgBN / 32], rb[BK / 32];
    if (row_begin < row_end) {                                    // (uniform: blockIdx only)
        wgrad_fetch<kWgBN>(ra, p.dy, p.dy_pitch, row_begin, row_end, n0, p.n, tid);
        wgrad_fetch<BK>(rb, p.x, p.x_pitch, row_begin, row_end, k0, p.k, tid);
    }
    for (int64_t row = row_begin; row < row_end; row += kWgKT) {
        __syncthreads();                                          // the previous step's fragment reads are done
        wgrad_stage<kWgBN, PA>(ra, s_a, tid);
        wgrad_stage<BK, PB>(rb, s_b, tid);
        __syncthreads();
        if (row + kWgKT < row_end) {                              // next step's pieces fly under this step's MFMAs
            wgrad_fetch<kWgBN>(ra, p.dy, p.dy_pitch, row + kWgKT, row_end, n0, p.n, tid);
            wgrad_fetch<BK>(rb, p.x, p.x_pitch, row + kWgKT, row_end, k0, p.k, tid);
        }
#pragma unroll
        for (int s = 0; s < kWgKT / 16; ++s) {
            frag8_t<T> fa[2], fb[KB];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = tr_frag<T>(a_rd + (16 * s) * PA + i * 64, a_rd + (16 * s + 4) * PA + i * 64);
#pragma unroll
            for (int j = 0; j < KB; ++j) fb[j] = tr_frag<T>(b_rd + (16 * s) * PB + j * 64, b_rd + (16 * s + 4) * PB + j * 64);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < KB; ++j) acc[i][j] = mfma_32x32x16<T>(fa[i], fb[j], acc[i][j]);
        }
    }

    // D[i][j]: j = lane & 31 (k column), i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (n row); only out[:n, :k] is written
    const int col_l = lane & 31, h = lane >> 5;
    float *const ws = p.direct ? nullptr : reinterpret_cast<float *>(p.out) + static_cast<int64_t>(slab) * p.n * p.k;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const int col = k0 + wk * (BK / 2) + j * 32 + col_l;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nrow = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (nrow < p.n && col < p.k) {
                    const float v = acc[i][j][r];
                    if (!p.direct) ws[static_cast<int64_t>(nrow) * p.k + col] = v;
                    else if (p.out_f32) reinterpret_cast<float *>(p.out)[nrow * p.out_pitch + col] = v;
                    else reinterpret_cast<uint16_t *>(p.out)[nrow * p.out_pitch + col] = from_float<T>(v);
                }
            }
        }
}

// out[i][4 c ... 4 c + 3] = round(sum over the slabs, ascending, fp32): one thread per 4 columns
template <typename T>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ ws, void *__restrict__ out, const int64_t out_pitch, const int n,
                                                           const int k, const int slabs, const int out_f32) {
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int kq = k / 4;
    if (idx >= static_cast<int64_t>(n) * kq) return;
    const int i = static_cast<int>(idx / kq), c = static_cast<int>(idx % kq) * 4;
    const int64_t plane = static_cast<int64_t>(n) * k;
    const float *src = ws + static_cast<int64_t>(i) * k + c;
    v4f sum = *reinterpret_cast<const v4f *>(src);
    for (int s = 1; s < slabs; ++s) sum += *reinterpret_cast<const v4f *>(src + s * plane);
    if (out_f32) {
        *reinterpret_cast<v4f *>(reinterpret_cast<float *>(out) + i * out_pitch + c) = sum;
    } else {
        uint2 pk;
        pk.x = pack2<T>(sum[0], sum[1]);
        pk.y = pack2<T>(sum[2], sum[3]);
        *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(out) + i * out_pitch + c) = pk;
    }
}

}  // namespace zigma

using namespace zigma;

extern "C" int64_t zigma_linear_wgrad_workspace_bytes(const zigma_linear_wgrad_params_t *pp) { return pp ? plan_wgrad(*pp).need : 0; }

extern "C" int zigma_linear_wgrad(const zigma_linear_wgrad_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    const zigma_linear_wgrad_params_t &p = *pp;
    const WgradPlan plan = plan_wgrad(p);
    if (!plan.kernel) return plan.status;

    (void)hipGetLastError();                                             // (after the refusals: a refused block never touches the device)
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int S = plan.slabs;
    wgrad_args_t a;
    a.dy = static_cast<const uint16_t *>(p.dy);
    a.x = static_cast<const uint16_t *>(p.x);
    a.direct = S == 1;
    a.out = a.direct ? p.out : p.workspace;
    a.dy_pitch = p.dy_row_stride, a.x_pitch = p.x_row_stride, a.out_pitch = p.out_row_stride;
    a.m = p.m;
    a.slab_rows = plan.slab_rows;
    a.n = p.n, a.k = p.k, a.n_tiles = plan.n_tiles;
    a.out_f32 = p.out_dtype == ZIGMA_F32;
    const dim3 grid(plan.gx, plan.gy);
    if (plan.bk == 64) {
        ZIGMA_DISPATCH_16BIT(p.dtype, T, hipLaunchKernelGGL((wgrad_kernel<T, 64>), grid, dim3(plan.block), 0, stream, a))
    } else {
        ZIGMA_DISPATCH_16BIT(p.dtype, T, hipLaunchKernelGGL((wgrad_kernel<T, 128>), grid, dim3(plan.block), 0, stream, a))
    }
    set_last_kernel(plan.kernel);
    int st = check_launch();
    if (st != ZIGMA_OK || S == 1) return st;
    const int64_t quads = static_cast<int64_t>(p.n) * (p.k / 4);
    ZIGMA_DISPATCH_16BIT(p.dtype, T, hipLaunchKernelGGL(wgrad_reduce_kernel<T>, dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0, stream,
                                                      static_cast<const float *>(p.workspace), p.out, p.out_row_stride, p.n, p.k, S, a.out_f32))
    return check_launch();
}

extern "C" int zigma_linear_wgrad_plan(const zigma_linear_wgrad_params_t *pp, const char **kernel) {
    return pp && kernel ? query_wgrad(*pp, kernel) : ZIGMA_ERR_NULL;
}
