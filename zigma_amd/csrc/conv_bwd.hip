// Depthwise causal conv1d (+bias, +SiLU) BACKWARD, token-major operands, gfx950.  C ABI: zigma_causal_conv1d_bwd.
//
// Replaces causal_conv1d_bwd_kernel / causal_conv1d_channellast_bwd_kernel (reference
// dis_causal_conv1d/csrc/causal_conv1d_bwd.cu:46-240,301-470).  With x' the (optionally gathered) input sequence:
//     pre[k]  = bias + sum_t w[t] x'[k - (W-1-t)]                          (recomputed, not stored)
//     dpre[k] = dout[k] * sigmoid(pre) (1 + pre (1 - sigmoid(pre)))        (SiLU) | dout[k]
//     dx'[k]  = sum_t w[t] dpre[k + (W-1-t)]          dw[t] = sum_{b,k} dpre[k] x'[k - (W-1-t)]        db = sum dpre
// HBM streaming like the forward: a lane owns 4 adjacent channels; a wave walks a SEGMENT of the sequence in tiles
// of 16 positions (all 16+2(W-1) x' rows and 16+(W-1) dout rows of a tile in flight before the first FMA) and keeps
// its partial dw / db in registers; one partial per (sample, segment) goes to the workspace and a finishing kernel
// adds them in a fixed order (the reference uses float atomics: not reproducible).
// dx is scattered through the same row table the forward gathered with (a permutation): dx[row[k]] = dx'[k].
#include "buffer_io.h"
#include "bwd_plan.h"

namespace zigma {

template <typename IO, typename WT, int W, bool SILU>
__global__ __launch_bounds__(64) void conv_bwd_tok_kernel(const zigma_conv_bwd_params_t p, float *ws) {
    using P = typename Pack<IO, 4>::type;
    constexpr int ES = static_cast<int>(sizeof(typename IO::raw)), LT = kCbLT;
    constexpr int NX = LT + 2 * (W - 1), ND = LT + (W - 1);       // x' rows k0-(W-1) .. k0+LT+W-2, dout rows k0 .. k0+LT+W-2
    static_assert(NX <= 64, "row table of a tile must fit one wave");
    const int lane = threadIdx.x;
    const int c0 = (blockIdx.x * 64 + lane) * 4;
    const int seg = blockIdx.y, b = blockIdx.z, L = p.seqlen;
    const bool live = c0 < p.dim;
    const int cc = live ? c0 : 0;

    float w[4][W], bias[4], dw[4][W], db[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < W; ++j) { w[i][j] = ld<WT>(p.weight, (cc + i) * p.weight_c_stride + j * p.weight_width_stride); dw[i][j] = 0.f; }
        bias[i] = p.bias ? ld<WT>(p.bias, cc + i) : 0.f;
        db[i] = 0.f;
    }
    const int64_t span = static_cast<int64_t>(L - 1);
    const int x_ls = static_cast<int>(p.x_l_stride) * ES, g_ls = static_cast<int>(p.dout_l_stride) * ES, o_ls = static_cast<int>(p.dx_l_stride) * ES;
    auto mk = [&](const void *base, int64_t bs, int ls) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<typename IO::raw *>(reinterpret_cast<const typename IO::raw *>(base) + b * bs), 0,
                                                  static_cast<int>(span * ls + static_cast<int64_t>(p.dim) * ES), 0x00020000);
    };
    const rsrc_t x_rs = mk(p.x, p.x_batch_stride, x_ls), g_rs = mk(p.dout, p.dout_batch_stride, g_ls), o_rs = mk(p.dx, p.dx_batch_stride, o_ls);
    const unsigned lane_off = static_cast<unsigned>(cc) * ES;
    const int k_seg = seg * kCbSeg, k_end = k_seg + kCbSeg < L ? k_seg + kCbSeg : L;

#pragma unroll 1
    for (int k0 = k_seg; k0 < k_end; k0 += LT) {
        // the sequence this tile belongs to (LT divides reset_period): positions outside [k_lo, k_hi) are another sequence — their x' reads
        // as the zero padding, their dout does not reach this tile's dx
        const int k_lo = p.reset_period > 0 ? (k0 / p.reset_period) * p.reset_period : 0;
        const int k_hi = p.reset_period > 0 && k_lo + p.reset_period < L ? k_lo + p.reset_period : L;
        int rowv;      // lane i <- row of scan position k0 - (W-1) + i   (input gather AND dx scatter table)
        {
            int k = k0 - (W - 1) + lane;
            k = k < 0 ? 0 : (k < L ? k : L - 1);
            rowv = p.x_row_index ? p.x_row_index[k] : k;
        }
        P xr[NX], gr[ND];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int k = k0 - (W - 1) + i;
            const int row = __builtin_amdgcn_readlane(rowv, i);
            xr[i] = P{};
            if (k >= k_lo && k < k_hi) xr[i] = buf_ld4<IO>(x_rs, lane_off, row * x_ls);
        }
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int k = k0 + i;
            gr[i] = P{};
            if (k < k_hi) gr[i] = buf_ld4<IO>(g_rs, lane_off, k * g_ls);     // dout is in scan order
        }
        // dpre at positions k0 .. k0+LT+W-2
        float dp[ND][4];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            float go[4];
            unpack4<IO>(gr[i], go);
            if (SILU) {
                float pre[4] = {bias[0], bias[1], bias[2], bias[3]};
#pragma unroll
                for (int t = 0; t < W; ++t) {
                    float xin[4];
                    unpack4<IO>(xr[i + t], xin);       // x'[k0 + i - (W-1-t)] sits at index i + t
#pragma unroll
                    for (int q = 0; q < 4; ++q) pre[q] += w[q][t] * xin[q];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float sg = fast_rcp(1.f + fast_exp2(-pre[q] * kLog2e));
                    go[q] *= sg * (1.f + pre[q] * (1.f - sg));
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) dp[i][q] = go[q];
        }
#pragma unroll
        for (int j = 0; j < LT; ++j) {
            const int k = k0 + j;
            if (k < L) {
                float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < W; ++t) {
                    float xin[4];
                    unpack4<IO>(xr[j + t], xin);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        o[q] += w[q][t] * dp[j + (W - 1 - t)][q];
                        dw[q][t] += dp[j][q] * xin[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) db[q] += dp[j][q];
                const int row = __builtin_amdgcn_readlane(rowv, j + (W - 1));
                if (live) buf_st4<IO>(pack4<IO>(o), o_rs, lane_off, row * o_ls);
            }
        }
    }
    if (live) {
        float *out = ws + ((static_cast<int64_t>(b) * gridDim.y + seg) * p.dim + c0) * (W + 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int t = 0; t < W; ++t) out[q * (W + 1) + t] = dw[q][t];
            out[q * (W + 1) + W] = db[q];
        }
    }
}

// one block per 64 (channel, tap) entries: 4 waves each add every 4th partial, then fold
__global__ __launch_bounds__(256) void conv_bwd_finish(const zigma_conv_bwd_params_t p, const float *ws, int n_parts) {
    __shared__ float s_acc[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W1 = p.width + 1, total = p.dim * W1;
    const int i = blockIdx.x * 64 + lane;                     // (c, t')  t' in [0, W]
    float acc = 0.f;
    if (i < total)
        for (int q = wave; q < n_parts; q += 4) acc += ws[static_cast<int64_t>(q) * total + i];
    s_acc[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && i < total) {
        acc = (s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane]);
        const int c = i / W1, t = i % W1;
        if (t < p.width) p.dweight[c * p.width + t] = acc;
        else if (p.dbias) p.dbias[c] = acc;
    }
}

template <typename IO, typename WT>
static void launch_conv_bwd(const zigma_conv_bwd_params_t &p, const BwdPlan &s, hipStream_t stream) {
    const dim3 grid(s.gx, s.gy, s.gz), block(s.block);
    float *ws = reinterpret_cast<float *>(p.workspace);
#define ZIGMA_CB(W_)                                                                                                 \
    if (s.silu) hipLaunchKernelGGL((conv_bwd_tok_kernel<IO, WT, W_, true>), grid, block, 0, stream, p, ws);          \
    else hipLaunchKernelGGL((conv_bwd_tok_kernel<IO, WT, W_, false>), grid, block, 0, stream, p, ws);
    switch (s.inst) {
        case 2: ZIGMA_CB(2) break;
        case 3: ZIGMA_CB(3) break;
        default: ZIGMA_CB(4) break;
    }
#undef ZIGMA_CB
}

}  // namespace zigma

using namespace zigma;

extern "C" int64_t zigma_causal_conv1d_bwd_workspace_bytes(const zigma_conv_bwd_params_t *p) { return p ? plan_conv_bwd(*p).need : 0; }

extern "C" int zigma_causal_conv1d_bwd_plan(const zigma_conv_bwd_params_t *pp, const char **kernel) {
    return pp && kernel ? query_bwd(plan_conv_bwd(*pp), kernel) : ZIGMA_ERR_NULL;
}

extern "C" int zigma_causal_conv1d_bwd(const zigma_conv_bwd_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_conv_bwd_params_t &p = *pp;
    const BwdPlan s = plan_conv_bwd(p);
    if (!s.kernel) return s.status;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ZIGMA_DISPATCH_DTYPE(s.io, IO, {
        ZIGMA_DISPATCH_DTYPE(s.wt, WT, { launch_conv_bwd<IO, WT>(p, s, stream); })
    })
    hipLaunchKernelGGL(conv_bwd_finish, dim3(s.fin_gx), dim3(s.fin_block), 0, stream, p, reinterpret_cast<const float *>(p.workspace), s.n_parts);
    set_last_kernel(s.kernel);
    return check_launch();
}
