// fp32 projections on the bf16 matrix cores by splitting ("bf16 x 3"): out = x @ W^T (+ bias) with x, bias and out in float32 and W as two
// bf16 planes.  C ABI: zigma_linear_f32_split (include/zigma_hip.h holds the definition of the arithmetic).
//
// Serves the F.linear of an fp32 model at Mamba.in_proj / out_proj (reference mamba_simple.py:290-294, selective_scan_interface.py:365) and
// CrossAttention.to_q / to_out (model_zigma.py:104-135) when zigma_amd.fp32_matmul.PRECISION is "high" (3 passes) or "medium" (1 pass).  gfx950
// has no xf32 MFMA and its fp32 MFMA runs at 1/16 of the bf16 rate: an fp32 value is hi + lo of two bf16 values to 16 significant bits, so
// x_hi w_hi + x_lo w_hi + x_hi w_lo is a GEMM with about 16 mantissa bits for 3/16 of the fp32 matrix time.
//
//   * operands lie [token][k] and [feature][k] as in linear.hip / linear_sm.hip, and the product is evaluated transposed like theirs: D[n][m],
//     W rows are the MFMA A operand, tokens the B operand, so a lane holds 4 consecutive features of ONE token per accumulator quad.
//   * workgroup = 4 waves as 2 (features) x 2 (tokens) = one tile of 128 tokens x 128 features, wave tile 64 x 64 (2 x 2 accumulators of
//     v_mfma_f32_32x32x16_bf16 for hi x hi, and with 3 passes 2 x 2 more for the two cross terms: the small terms are added among themselves
//     first and meet the large sum once, at the end).  k-steps of 64.
//   * the weight planes were split once by the host (they are static at inference); only x is split here: a lane takes 8 consecutive fp32 of a
//     token row from global memory into registers (the NEXT k-step's loads fly under this step's MFMAs), converts them with v_cvt_pk_bf16_f32,
//     subtracts, converts the remainder, and writes one 16-byte piece into each of the two LDS planes.  No split activations ever reach HBM.
//   * LDS: planes of 128 rows x 128 B (w_hi, w_lo, x_hi, x_lo) in linear_sm.hip's layout — 16-byte slot ^= swz_slot(row) (csrc/lds_pipe.h) on the writes and
//     again on the fragment reads (conflict-free ds_read_b128 for 32 consecutive rows).
//   * epilogue: hi x hi + cross (+ bias), fp32, transposed through a wave-private LDS tile (32 tokens x 64 features, 16-byte padded pitch) so
//     every global store instruction covers 4 token rows x 256 contiguous bytes.  Token rows past m are neither loaded nor stored.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; the build fails on scratch or a spill in either instantiation): DESIGN.md §3.4.
#include "lds_pipe.h"
#include "linear_plan.h"

namespace zigma {
namespace lsp {

constexpr int kBM = kSplitBM, kBN = kSplitBN, kBK = 64, kThreads = 256;      // (the tile plan_linear_split() counts the grid in)
constexpr int kPlane = 128 * 128;                       // bytes of one LDS plane: 128 rows x 64 bf16
constexpr int kEpiPitch = 64 * 4 + 16;                  // epilogue tile: bytes per token row (64 fp32 features, padded)
constexpr uint32_t kMaxBf16Bits = 0x7f7f0000u;          // the largest finite bf16 as an fp32 pattern

struct args_t {
    const float *x;
    const uint16_t *w_hi, *w_lo;
    const float *bias;
    float *out;
    int64_t x_pitch, wh_pitch, wl_pitch, o_pitch;       // elements
    int64_t m;
    int32_t n, k, tiles_n;
};

// split of one value outside the fast path's range (|a| >= the largest finite bf16, infinities, NaNs): hi in the low, lo in the high half
__device__ __forceinline__ uint32_t split_edge(const float a) {
    const uint32_t mag = __float_as_uint(a) & 0x7fffffffu;
    if (mag >= 0x7f800000u) return from_float<BF16>(a);                                      // non-finite: hi = bf16(a), lo = 0
    const float top = __uint_as_float(kMaxBf16Bits);
    const uint16_t h = from_float<BF16>(fminf(fmaxf(a, -top), top));                         // a finite a never becomes infinite
    return static_cast<uint32_t>(h) | (static_cast<uint32_t>(from_float<BF16>(a - to_float<BF16>(h))) << 16);
}

// 8 consecutive fp32 of a row -> one 16-byte piece of the hi plane and one of the lo plane
__device__ __forceinline__ void split8(const v4f a, const v4f b, u32x4 &hi, u32x4 &lo) {
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    uint32_t mx = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t mag = __float_as_uint(v[e]) & 0x7fffffffu;
        mx = mag > mx ? mag : mx;
    }
    uint32_t h[4], l[4];
    if (mx < kMaxBf16Bits) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = pack2_pk<BF16>(v[2 * e], v[2 * e + 1]);
            l[e] = pack2_pk<BF16>(v[2 * e] - lo16<BF16>(h[e]), v[2 * e + 1] - hi16<BF16>(h[e]));     // (the subtraction is exact in fp32)
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t s0 = split_edge(v[2 * e]), s1 = split_edge(v[2 * e + 1]);
            h[e] = (s0 & 0xffffu) | (s1 << 16);
            l[e] = (s0 >> 16) | (s1 & 0xffff0000u);
        }
    }
    hi = u32x4{h[0], h[1], h[2], h[3]};
    lo = u32x4{l[0], l[1], l[2], l[3]};
}

template <int PASSES>
// (two workgroups per CU: one's staging and barriers run under the other's MFMAs — 2 x 64 KB of LDS, at most 256 registers per lane)
__global__ __launch_bounds__(kThreads, 2) void linear_split_kernel(const args_t p) {
    constexpr bool LO = PASSES == 3;
    constexpr int STAGE = (LO ? 4 : 2) * kPlane, EPI = 4 * 32 * kEpiPitch;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[STAGE > EPI ? STAGE : EPI];
    unsigned char *const s_wh = smem, *const s_xh = smem + kPlane;
    unsigned char *const s_wl = smem + (LO ? 2 * kPlane : 0), *const s_xl = smem + (LO ? 3 * kPlane : 0);      // (used with 3 passes only)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wm = wave & 1;
    const int j = lane & 31, kh = lane >> 5;
    // consecutive workgroup ids go round the 8 XCDs: XCD x takes a contiguous eighth of the (m-tile, n-tile) raster, as in linear_sm.hip
    int tile = blockIdx.x;
    if ((gridDim.x & 7) == 0) tile = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int mt = tile / p.tiles_n, nt = tile - mt * p.tiles_n;
    const int64_t m0 = static_cast<int64_t>(mt) * kBM;
    const int n0 = nt * kBN;
    const int nk = p.k / kBK;

    // staging: piece c = tid + 256 i of a plane is row c >> 3, 16-byte piece c & 7 (8 bf16 = 8 consecutive k)
    const int s_row = tid >> 3, s_piece = tid & 7;            // + 32 rows per i
    const float *xg = p.x + (m0 + s_row) * p.x_pitch + s_piece * 8;
    const uint16_t *whg = p.w_hi + static_cast<int64_t>(n0 + s_row) * p.wh_pitch + s_piece * 8;
    const uint16_t *wlg = LO ? p.w_lo + static_cast<int64_t>(n0 + s_row) * p.wl_pitch + s_piece * 8 : nullptr;

    v4f xr[4][2];
    u32x4 whr[4], wlr[LO ? 4 : 1];
    auto fetch = [&](const int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v4f a = {0.f, 0.f, 0.f, 0.f}, b = a;
            if (m0 + s_row + 32 * i < p.m) {                                 // token rows past m arrive as zeros
                const float *src = xg + 32 * i * p.x_pitch + kt * kBK;
                a = *reinterpret_cast<const v4f *>(src);
                b = *reinterpret_cast<const v4f *>(src + 4);
            }
            xr[i][0] = a, xr[i][1] = b;
            whr[i] = *reinterpret_cast<const u32x4 *>(whg + 32 * i * p.wh_pitch + kt * kBK);      // (n % 128 == 0: every weight row exists)
            if constexpr (LO) wlr[i] = *reinterpret_cast<const u32x4 *>(wlg + 32 * i * p.wl_pitch + kt * kBK);
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int off = swz(s_row + 32 * i, s_piece);
            u32x4 hi, lo;
            split8(xr[i][0], xr[i][1], hi, lo);
            *reinterpret_cast<u32x4 *>(s_wh + off) = whr[i];
            *reinterpret_cast<u32x4 *>(s_xh + off) = hi;
            if constexpr (LO) {
                *reinterpret_cast<u32x4 *>(s_wl + off) = wlr[i];
                *reinterpret_cast<u32x4 *>(s_xl + off) = lo;
            }
        }
    };

    mfma_f32x16 acc[2][2], crs[LO ? 2 : 1][LO ? 2 : 1];       // [feature block][token block]: hi x hi, and the two cross terms
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[a][b][r] = 0.f;
                if constexpr (LO) crs[a][b][r] = 0.f;
            }

    // fragment reads: every row base is a multiple of 32, so swz_slot(row) = swz_slot(j)
    const int sw = swz_slot(j);
    const int a_row0 = (wn * 64 + j) * 128, b_row0 = (wm * 64 + j) * 128;

    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                                      // the previous step's fragment reads are done
        stage();
        __syncthreads();
        if (kt + 1 < nk) fetch(kt + 1);                       // the next step's rows fly under this step's MFMAs
#pragma unroll
        for (int ks = 0; ks < kBK / 16; ++ks) {
            const int off = (((ks << 1) | kh) ^ sw) << 4;
            frag8_t<BF16> ah[2], bh[2], al[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = __builtin_bit_cast(frag8_t<BF16>, *reinterpret_cast<const u32x4 *>(s_wh + a_row0 + i * 32 * 128 + off));
                bh[i] = __builtin_bit_cast(frag8_t<BF16>, *reinterpret_cast<const u32x4 *>(s_xh + b_row0 + i * 32 * 128 + off));
                if constexpr (LO) {
                    al[i] = __builtin_bit_cast(frag8_t<BF16>, *reinterpret_cast<const u32x4 *>(s_wl + a_row0 + i * 32 * 128 + off));
                    bl[i] = __builtin_bit_cast(frag8_t<BF16>, *reinterpret_cast<const u32x4 *>(s_xl + b_row0 + i * 32 * 128 + off));
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[a][b] = mfma_32x32x16<BF16>(ah[a], bh[b], acc[a][b]);
                    if constexpr (LO) {
                        crs[a][b] = mfma_32x32x16<BF16>(ah[a], bl[b], crs[a][b]);
                        crs[a][b] = mfma_32x32x16<BF16>(al[a], bh[b], crs[a][b]);
                    }
                }
        }
    }

    // ---- epilogue: D[i][jj], jj = token (lane & 31), i = feature = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  The wave transposes 32 tokens x 64
    // features at a time through its own LDS tile (the planes are free behind the barrier) and stores 16-byte pieces along the token rows
    __syncthreads();
    unsigned char *const scr = smem + wave * (32 * kEpiPitch);
    const int col0 = n0 + wn * 64;                            // first feature of this wave
    const int rd_tok = lane >> 4, rd_pc = lane & 15;          // reads: 4 token rows x 16 pieces per instruction
    v4f bias4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) bias4 = *reinterpret_cast<const v4f *>(p.bias + col0 + rd_pc * 4);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v4f v = {acc[nb][mb][q * 4], acc[nb][mb][q * 4 + 1], acc[nb][mb][q * 4 + 2], acc[nb][mb][q * 4 + 3]};
                if constexpr (LO) v += v4f{crs[nb][mb][q * 4], crs[nb][mb][q * 4 + 1], crs[nb][mb][q * 4 + 2], crs[nb][mb][q * 4 + 3]};
                *reinterpret_cast<v4f *>(scr + j * kEpiPitch + (nb * 32 + q * 8 + kh * 4) * 4) = v;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                      // wave-private tile: writes and reads of one wave
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int tok = it * 4 + rd_tok;
            const int64_t row = m0 + wm * 64 + mb * 32 + tok;
            if (row < p.m) {
                const v4f v = *reinterpret_cast<const v4f *>(scr + tok * kEpiPitch + rd_pc * 16) + bias4;
                *reinterpret_cast<v4f *>(p.out + row * p.o_pitch + col0 + rd_pc * 4) = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                      // ... before the next token block overwrites the tile
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace lsp
}  // namespace zigma

using namespace zigma;

extern "C" int zigma_linear_f32_split(const zigma_linear_split_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    const zigma_linear_split_params_t &p = *pp;
    const LinearSplitPlan plan = plan_linear_split(p);         // every refusal: csrc/linear_plan.h
    if (!plan.kernel) return plan.status;
    const bool lo = plan.lo;

    (void)hipGetLastError();                                  // (after the refusals: a refused block never touches the device)
    lsp::args_t a;
    a.x = static_cast<const float *>(p.x);
    a.w_hi = static_cast<const uint16_t *>(p.w_hi);
    a.w_lo = lo ? static_cast<const uint16_t *>(p.w_lo) : nullptr;
    a.bias = static_cast<const float *>(p.bias);
    a.out = static_cast<float *>(p.out);
    a.x_pitch = p.x_row_stride, a.wh_pitch = p.w_hi_row_stride, a.wl_pitch = lo ? p.w_lo_row_stride : 0, a.o_pitch = p.out_row_stride;
    a.m = p.m, a.n = p.n, a.k = p.k, a.tiles_n = p.n / lsp::kBN;
    const dim3 grid(static_cast<unsigned>(plan.tiles)), block(lsp::kThreads);
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (lo) hipLaunchKernelGGL(lsp::linear_split_kernel<3>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(lsp::linear_split_kernel<1>, grid, block, 0, stream, a);
    set_last_kernel(plan.kernel);
    return check_launch();
}

extern "C" int zigma_linear_f32_split_plan(const zigma_linear_split_params_t *pp, const char **kernel) {
    return pp && kernel ? query_linear_split(*pp, kernel) : ZIGMA_ERR_NULL;
}
