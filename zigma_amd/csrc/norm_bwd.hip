// RMSNorm / LayerNorm (+ residual / prenorm) BACKWARD, gfx950.  C ABI: zigma_add_norm_bwd.
//
// Replaces the Triton kernel _layer_norm_bwd_kernel and its host _layer_norm_bwd (reference
// dis_mamba/mamba_ssm/ops/triton/layernorm.py:196-377).  With s = the tensor that was normalised (x, or x + residual =
// the forward's residual_out), xhat = (s - mean) * rstd (mean = 0 for RMSNorm), wdy = dy * weight:
//     c1 = mean(xhat * wdy),  c2 = mean(wdy)  (LayerNorm only)
//     ds = (wdy - xhat * c1 - c2) * rstd + dresidual_out          ->  dx (x dtype) and dresidual (residual dtype)
//     dweight = sum_rows dy * xhat,   dbias = sum_rows dy
// mean / rstd are recomputed from s (one extra pass over registers, no extra HBM traffic: the row is read once).
// One wave per row at a time, each wave walks rows with a fixed stride and keeps its partial dweight / dbias in
// registers; the partials go to the workspace and a finishing kernel adds them in a fixed order (the reference
// does the same with one partial per SM, layernorm.py:330-347).
#include "norm_plan.h"
#include "vec_io.h"

namespace zigma {

template <typename XT, typename RT, typename WT, int VEC, int ITERS>
__global__ __launch_bounds__(64 * kNbWaves) void add_norm_bwd_kernel(const zigma_norm_bwd_params_t p, float *ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * kNbWaves + wave, n_gw = gridDim.x * kNbWaves;
    const int cols = p.cols;
    float dw[ITERS][VEC], db[ITERS][VEC], w[ITERS][VEC];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * 64 + lane) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) { dw[it][v] = 0.f; db[it][v] = 0.f; w[it][v] = 1.f; }
        if (p.weight && c < cols) loadv<WT, VEC>(p.weight, c, w[it]);
    }
    for (int64_t r = gw; r < p.rows; r += n_gw) {
        float s[ITERS][VEC], dy[ITERS][VEC];
        float sum = 0.f, sq = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * 64 + lane) * VEC;
#pragma unroll
            for (int v = 0; v < VEC; ++v) { s[it][v] = 0.f; dy[it][v] = 0.f; }
            if (c < cols) {
                loadv<RT, VEC>(p.xsum, r * p.xsum_row_stride + c, s[it]);
                loadv<XT, VEC>(p.dy, r * p.dy_row_stride + c, dy[it]);
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) { sum += s[it][v]; sq += s[it][v] * s[it][v]; }
        }
        float mean = 0.f, rstd;
        if (p.is_rms) {
            rstd = rsqrtf(wave_sum<64>(sq) / cols + p.eps);
        } else {
            mean = wave_sum<64>(sum) / cols;
            float var = 0.f;
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int c = (it * 64 + lane) * VEC;
                if (c < cols) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) { const float d = s[it][v] - mean; var += d * d; }
                }
            }
            rstd = rsqrtf(wave_sum<64>(var) / cols + p.eps);
        }
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * 64 + lane) * VEC;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float xhat = c < cols ? (s[it][v] - mean) * rstd : 0.f;
                const float wdy = dy[it][v] * w[it][v];
                c1 += xhat * wdy; c2 += wdy;
                dw[it][v] += dy[it][v] * xhat; db[it][v] += dy[it][v];
                s[it][v] = xhat;
                dy[it][v] = wdy;
            }
        }
        c1 = wave_sum<64>(c1) / cols;
        c2 = p.is_rms ? 0.f : wave_sum<64>(c2) / cols;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int c = (it * 64 + lane) * VEC;
            if (c < cols) {
                float ds[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) ds[v] = (dy[it][v] - s[it][v] * c1 - c2) * rstd;
                if (p.dresidual_out) {
                    float dr[VEC];
                    loadv<RT, VEC>(p.dresidual_out, r * p.dres_out_row_stride + c, dr);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) ds[v] += dr[v];
                }
                if (p.dx) storev<XT, VEC>(p.dx, r * p.dx_row_stride + c, ds);
                if (p.dresidual) storev<RT, VEC>(p.dresidual, r * p.dres_row_stride + c, ds);
            }
        }
    }
    // fold the 4 waves' partials through LDS: one partial per WORKGROUP goes to the workspace
    __shared__ float s_fold[kNbWaves][2][64 * VEC];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int c = (it * 64 + lane) * VEC;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            s_fold[wave][0][lane * VEC + v] = dw[it][v];
            s_fold[wave][1][lane * VEC + v] = db[it][v];
        }
        __syncthreads();
        if (wave < 2 && c < cols) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const int q = lane * VEC + v;
                ws[(static_cast<int64_t>(blockIdx.x) * 2 + wave) * cols + c + v] =
                    (s_fold[0][wave][q] + s_fold[1][wave][q]) + (s_fold[2][wave][q] + s_fold[3][wave][q]);
            }
        }
    }
}

// one block per 64 columns of dweight or dbias: 4 waves each add every 4th partial (coalesced 256-byte reads), then fold
__global__ __launch_bounds__(256) void add_norm_bwd_finish(const zigma_norm_bwd_params_t p, const float *ws, int n_parts) {
    __shared__ float s_acc[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int blocks_per = (p.cols + 63) / 64;
    const int which = blockIdx.x / blocks_per, c = (blockIdx.x % blocks_per) * 64 + lane;
    float acc = 0.f;
    if (c < p.cols)
        for (int q = wave; q < n_parts; q += 4) acc += ws[(static_cast<int64_t>(q) * 2 + which) * p.cols + c];
    s_acc[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < p.cols) {
        acc = (s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane]);
        if (which == 0) { if (p.dweight) p.dweight[c] = acc; }
        else if (p.dbias) p.dbias[c] = acc;
    }
}

template <typename XT, typename RT, typename WT>
static void launch_norm_bwd(const zigma_norm_bwd_params_t &p, const NormPlan &s, hipStream_t stream) {
    float *ws = reinterpret_cast<float *>(p.workspace);
#define ZIGMA_NB(V_, I_) hipLaunchKernelGGL((add_norm_bwd_kernel<XT, RT, WT, V_, I_>), dim3(s.gx), dim3(s.block), 0, stream, p, ws)
    if (s.vec == 4 && s.iters == 3) ZIGMA_NB(4, 3);
    else if (s.vec == 4) ZIGMA_NB(4, 8);
    else if (s.iters == 4) ZIGMA_NB(1, 4);
    else if (s.iters == 12) ZIGMA_NB(1, 12);
    else ZIGMA_NB(1, 32);
#undef ZIGMA_NB
    hipLaunchKernelGGL(add_norm_bwd_finish, dim3(s.fin_gx), dim3(256), 0, stream, p, ws, static_cast<int>(s.gx));
}

}  // namespace zigma

using namespace zigma;

extern "C" int64_t zigma_add_norm_bwd_workspace_bytes(const zigma_norm_bwd_params_t *p) { return p ? plan_add_norm_bwd(*p).need : 0; }

extern "C" int zigma_add_norm_bwd_plan(const zigma_norm_bwd_params_t *pp, const char **kernel) {
    return pp && kernel ? query_norm(plan_add_norm_bwd(*pp), kernel) : ZIGMA_ERR_NULL;
}

extern "C" int zigma_add_norm_bwd(const zigma_norm_bwd_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_norm_bwd_params_t &p = *pp;
    const NormPlan s = plan_add_norm_bwd(p);
    if (!s.kernel) return s.status;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ZIGMA_DISPATCH_NORM_SLOT(p.x_dtype, s.res32, s.w32, XT, RT, WT, { launch_norm_bwd<XT, RT, WT>(p, s, stream); })
    set_last_kernel(s.kernel);
    return check_launch();
}
