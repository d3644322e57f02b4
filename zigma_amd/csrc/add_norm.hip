// Fused (gated-branch add) + residual add + RMSNorm/LayerNorm (+ adaLN modulate) forward, gfx950.
// C ABI: zigma_add_norm_fwd (include/zigma_hip.h).
//
// Replaces the Triton kernel _layer_norm_fwd_1pass_kernel (reference dis_mamba/mamba_ssm/ops/triton/
// layernorm.py:65-120) and folds in the elementwise glue Block.forward wraps around it
// (model_zigma.py:53-54,441-458): the gate*branch residual of the previous sub-layer on the way in,
// the adaLN modulate on the way out.  Pure HBM streaming: one wave owns one row, the row lives in
// registers between the statistics and the normalisation, so every operand is read or written once.
#include "norm_plan.h"
#include "vec_io.h"

namespace zigma {

// VEC = 8 / 4 (vector paths) or 1 (scalar path, any alignment); a row is shared by LPR lanes (64 / LPR rows per wave) that walk it in
// ITERS chunks of LPR * VEC columns.  LPR = 16 is for rows of a few hundred 16-bit elements (E = 640: 5 x 16 bytes per lane, every
// lane busy, 4 rows per wave instruction and per reduction step); LPR = 64 is one row per wave.
template <typename XT, typename RT, typename WT, typename MT, int VEC, int ITERS, int LPR = 64>
__global__ __launch_bounds__(256) void add_norm_kernel(const zigma_norm_params_t p) {
    const int lane = (threadIdx.x & 63) % LPR;
    const int64_t r = (static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6)) * (64 / LPR) + (threadIdx.x & 63) / LPR;
    if (r >= p.rows) return;            // (rows % (64 / LPR) == 0 on the multi-row path: whole waves leave together)
    const int b = static_cast<int>(r / p.rows_per_batch);
    const int cols = p.cols;

    float v[ITERS][VEC];
    float sum = 0.f, sq = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * LPR + lane) * VEC;
        if (c < cols) {
            float x[VEC];
            loadv<XT, VEC>(p.x, r * p.x_row_stride + c, x);
            if (p.branch) {
                float br[VEC], g[VEC];
                loadv<XT, VEC>(p.branch, r * p.branch_row_stride + c, br);
                loadv<MT, VEC>(p.gate, b * p.mod_batch_stride + c, g);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    float s = x[i] + g[i] * br[i];
                    // fp16: keep the fp32 sum a value of its own.  hipcc otherwise folds product, sum and narrowing into one
                    // v_fma_mixlo_f16, which rounds the exact sum ONCE to fp16; x' is the fp32 sum rounded to x's type, which is what
                    // the unfused composition stores (they differ where the fp32 rounding lands on an fp16 tie: 12 of 1 M elements)
                    if constexpr (XT::id == ZIGMA_F16) asm("" : "+v"(s));
                    x[i] = rnd<XT>(s);
                }
                if (p.x_out) {
                    storev<XT, VEC>(p.x_out, r * p.x_out_row_stride + c, x);
                }
            }
            if (p.residual) {
                float rs[VEC];
                loadv<RT, VEC>(p.residual, r * p.res_row_stride + c, rs);
#pragma unroll
                for (int i = 0; i < VEC; ++i) x[i] += rs[i];
            }
            if (p.residual_out) {
                storev<RT, VEC>(p.residual_out, r * p.res_out_row_stride + c, x);
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) { v[it][i] = x[i]; sum += x[i]; sq += x[i] * x[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[it][i] = 0.f;
        }
    }
    float mean = 0.f, rstd;
    if (p.is_rms) {
        rstd = rsqrtf(wave_sum<LPR>(sq) / cols + p.eps);
    } else {  // two-pass variance on the register copy, like the Triton kernel (layernorm.py:102-107)
        mean = wave_sum<LPR>(sum) / cols;
        float var = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * LPR + lane) * VEC;
            if (c < cols) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) { const float dlt = v[it][i] - mean; var += dlt * dlt; }
            }
        }
        rstd = rsqrtf(wave_sum<LPR>(var) / cols + p.eps);
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * LPR + lane) * VEC;
        if (c < cols) {
            float y[VEC], w[VEC], bs[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) { w[i] = 1.f; bs[i] = 0.f; }
            if (p.weight) loadv<WT, VEC>(p.weight, c, w);
            if (p.bias) loadv<WT, VEC>(p.bias, c, bs);
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = (v[it][i] - mean) * rstd * w[i] + bs[i];
            if (p.y_out) {
                storev<XT, VEC>(p.y_out, r * p.y_row_stride + c, y);
            }
            if (p.shift) {
                float sh[VEC], sc[VEC];
                loadv<MT, VEC>(p.shift, b * p.mod_batch_stride + c, sh);
                loadv<MT, VEC>(p.scale, b * p.mod_batch_stride + c, sc);
#pragma unroll
                for (int i = 0; i < VEC; ++i) y[i] = rnd<XT>(y[i]) * (1.f + sc[i]) + sh[i];
                storev<XT, VEC>(p.y_mod, r * p.y_mod_row_stride + c, y);
            }
        }
    }
}

template <typename XT, typename RT, typename WT>
static void launch_norm(const zigma_norm_params_t &p, const NormPlan &s, hipStream_t stream) {
    const dim3 grid(s.gx), block(s.block);
#define ZIGMA_NORM(V_, I_, L_) hipLaunchKernelGGL((add_norm_kernel<XT, RT, WT, XT, V_, I_, L_>), grid, block, 0, stream, p)
    if (s.lpr == 16) {
        switch (s.iters) {
            case 1: ZIGMA_NORM(8, 1, 16); break;
            case 2: ZIGMA_NORM(8, 2, 16); break;
            case 3: ZIGMA_NORM(8, 3, 16); break;
            case 4: ZIGMA_NORM(8, 4, 16); break;
            case 5: ZIGMA_NORM(8, 5, 16); break;
            case 6: ZIGMA_NORM(8, 6, 16); break;
            case 7: ZIGMA_NORM(8, 7, 16); break;
            default: ZIGMA_NORM(8, 8, 16); break;
        }
    } else if (s.vec == 8) ZIGMA_NORM(8, 2, 64);
    else if (s.vec == 4 && s.iters == 4) ZIGMA_NORM(4, 4, 64);
    else if (s.vec == 4) ZIGMA_NORM(4, 16, 64);
    else if (s.iters == 16) ZIGMA_NORM(1, 16, 64);
    else ZIGMA_NORM(1, 64, 64);
#undef ZIGMA_NORM
}

}  // namespace zigma

using namespace zigma;

extern "C" int zigma_add_norm_fwd_plan(const zigma_norm_params_t *pp, const char **kernel) {
    return pp && kernel ? query_norm(plan_add_norm(*pp), kernel) : ZIGMA_ERR_NULL;
}

extern "C" int zigma_add_norm_fwd(const zigma_norm_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();  // a stale error of an unrelated earlier call is not ours to report
    const zigma_norm_params_t &p = *pp;
    const NormPlan s = plan_add_norm(p);
    if (!s.kernel) return s.status;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ZIGMA_DISPATCH_NORM_SLOT(p.x_dtype, s.res32, s.w32, XT, RT, WT, { launch_norm<XT, RT, WT>(p, s, stream); })
    set_last_kernel(s.kernel);
    return check_launch();
}
