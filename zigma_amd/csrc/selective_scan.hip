// Selective-scan forward for gfx950 (MI355X).  C ABI: zigma_selective_scan_fwd (include/zigma_hip.h).
//
// Replaces the reference's selective_scan_fwd_kernel (dis_mamba/csrc/selective_scan/
// selective_scan_fwd_kernel.cuh:67-303).  The reference gives one 64-thread block a whole (b, d)
// row, lays L across the threads and runs `dstate` CUB block scans of (a, b) pairs.  That shape is
// wrong for this machine: the recurrence is VALU / transcendental bound on CDNA4 (16 exp2 per
// element against 8 B of HBM traffic; measured v_exp_f32 ~ 1.8 v_fma_f32 issue slots), so every
// cross-lane combine of a parallel scan is pure overhead, and B/C would be re-read through L2 by every
// one of the 1280 channel rows of a sample.
//
// Three kernels; scan_plan.h chooses one of them, its form and its template switches for every call:
//
//  scan_tok2_kernel  — the hot path (scan_tok2.inc): 16-bit I/O, dstate 16, whole 16-step tiles, gated output;
//      also the training form, the sequence split and dt_proj inside the kernel.
//
//  scan_tok_kernel   — the first-generation token-major kernel (scan_tok.inc), for the rest of the token-major
//      layout: f32, dstate 8, ragged lengths, no gate, carries without a split.  Token-major operands (channel
//      contiguous), one LANE per channel, time runs sequentially inside the lane, so there is NO scan and no
//      cross-lane combine: per (element, state) exactly v_mul, v_exp, v_mul, v_fma, v_fmac.  A workgroup owns a
//      64-channel slab of one sample; its NW waves split the dstate dimension (4 states each).  The
//      B_l / C_l values of a 4-step group sit in ONE VGPR per operand (lane -> (step, state), the same
//      16 values in every row of 16 lanes) and reach the FMAs as DPP row_newbcast operands: no SGPR
//      traffic, no LDS traffic, no extra instruction.  Per-element work (softplus, D*u, SiLU gate) is
//      done once per element by a cooperative prologue / epilogue around each LT-step tile and shared
//      through LDS.  The zigzag reordering is two row-index tables applied to whole 128-byte rows
//      (z gather, out_z scatter): coalesced by construction.
//
//  scan_generic_kernel — any strides / constant or grouped B,C / any dstate <= 256: the reference's
//      full call surface (selective_scan.cpp:233-305).  One row per NS lanes (one lane per state),
//      butterfly reduction for y.  Compatibility path, not tuned.
#include "scan_plan.h"
#include "zigma_common.h"

namespace zigma {

// =================================================================================================
// generic kernel
// =================================================================================================
template <typename IO, typename BCT, int NS, int SPL>
__global__ __launch_bounds__(64) void scan_generic_kernel(const zigma_scan_params_t p) {
    constexpr int RPW = 64 / NS;  // rows per wave
    const int lane = threadIdx.x;
    const int sub = lane % NS;
    const int64_t nrows = static_cast<int64_t>(p.batch) * p.dim;
    int64_t row = static_cast<int64_t>(blockIdx.x) * RPW + lane / NS;
    const bool row_ok = row < nrows;
    if (!row_ok) row = nrows - 1;  // keep the lane in the shuffles
    const int b = static_cast<int>(row / p.dim);
    const int d = static_cast<int>(row % p.dim);
    const int g = d / (p.dim / p.n_groups);
    const int N = p.dstate;
    const int chunk_len = p.chunk_len > 0 ? p.chunk_len : 2048;
    const int n_chunks = (p.seqlen + chunk_len - 1) / chunk_len;

    float a2[SPL], h[SPL], bc_const_b[SPL], bc_const_c[SPL];
    bool n_ok[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int n = sub + j * NS;
        n_ok[j] = n < N;
        const int nn = n_ok[j] ? n : 0;
        a2[j] = reinterpret_cast<const float *>(p.A)[d * p.A_d_stride + nn * p.A_dstate_stride] * kLog2e;
        h[j] = 0.f;
        bc_const_b[j] = p.is_variable_B ? 0.f
                        : reinterpret_cast<const float *>(p.B)[d * p.B_d_stride + nn * p.B_dstate_stride];
        bc_const_c[j] = p.is_variable_C ? 0.f
                        : reinterpret_cast<const float *>(p.C)[d * p.C_d_stride + nn * p.C_dstate_stride];
    }
    const float Dv = p.D ? reinterpret_cast<const float *>(p.D)[d] : 0.f;
    const float bias = p.delta_bias ? reinterpret_cast<const float *>(p.delta_bias)[d] : 0.f;
    const int64_t u_off = b * p.u_batch_stride + d * p.u_d_stride;
    const int64_t dl_off = b * p.delta_batch_stride + d * p.delta_d_stride;
    const int64_t z_off = b * p.z_batch_stride + d * p.z_d_stride;
    const int64_t o_off = b * p.out_batch_stride + d * p.out_d_stride;
    const int64_t oz_off = b * p.out_z_batch_stride + d * p.out_z_d_stride;
    const int64_t B_off = b * p.B_batch_stride + g * p.B_group_stride;
    const int64_t C_off = b * p.C_batch_stride + g * p.C_group_stride;
    float cum = 0.f;

    for (int l = 0; l < p.seqlen; ++l) {
        const float uv = ld<IO>(p.u, u_off + l * p.u_l_stride);
        float dv = ld<IO>(p.delta, dl_off + l * p.delta_l_stride) + bias;
        if (p.delta_softplus) dv = softplus20(dv);
        const float du = dv * uv;
        cum += dv;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            const int n = sub + j * NS;
            if (n_ok[j]) {
                const float Bv = p.is_variable_B ? ld<BCT>(p.B, B_off + n * p.B_dstate_stride + l * p.B_l_stride)
                                                 : bc_const_b[j];
                const float Cv = p.is_variable_C ? ld<BCT>(p.C, C_off + n * p.C_dstate_stride + l * p.C_l_stride)
                                                 : bc_const_c[j];
                h[j] = fast_exp2(dv * a2[j]) * h[j] + du * Bv;
                acc += h[j] * Cv;
            }
        }
#pragma unroll
        for (int s = NS / 2; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (sub == 0 && row_ok) {
            const float y = acc + Dv * uv;
            const int64_t orow = p.out_row_index ? p.out_row_index[l] : l;
            if (p.out) st<IO>(p.out, o_off + orow * p.out_l_stride, y);
            if (p.z) {
                const int64_t zrow = p.z_row_index ? p.z_row_index[l] : l;
                const float zv = ld<IO>(p.z, z_off + zrow * p.z_l_stride);
                st<IO>(p.out_z, oz_off + orow * p.out_z_l_stride, y * silu(zv));
            }
        }
        if (p.x && row_ok && ((l + 1) % chunk_len == 0 || l == p.seqlen - 1)) {
            const int chunk = l / chunk_len;
            float *xr = reinterpret_cast<float *>(p.x) + (row * n_chunks + chunk) * 2 * N;
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                const int n = sub + j * NS;
                if (n_ok[j]) {
                    xr[2 * n] = fast_exp2(cum * a2[j]);
                    xr[2 * n + 1] = h[j];
                }
            }
        }
    }
}

// token-major kernels: scan_tok.inc, scan_tok2.inc, one launcher per I/O element type in scan_tok_{bf16,f16,f32}.hip
int launch_scan_tok_bf16(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream);
int launch_scan_tok_f16(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream);
int launch_scan_tok_f32(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream);

// =================================================================================================
// host dispatch
// =================================================================================================
template <typename IO, typename BCT>
static void launch_generic(const zigma_scan_params_t &p, hipStream_t stream) {
    void (*const kernels[])(zigma_scan_params_t) = {   // NS lanes per row: dstate rounded up to a power of two, at most 64; SPL states per lane
        scan_generic_kernel<IO, BCT, 1, 1>, scan_generic_kernel<IO, BCT, 2, 1>, scan_generic_kernel<IO, BCT, 4, 1>,
        scan_generic_kernel<IO, BCT, 8, 1>, scan_generic_kernel<IO, BCT, 16, 1>, scan_generic_kernel<IO, BCT, 32, 1>,
        scan_generic_kernel<IO, BCT, 64, 1>, scan_generic_kernel<IO, BCT, 64, 2>, scan_generic_kernel<IO, BCT, 64, 4>};
    int i = 0;
    while ((1 << i) < p.dstate) ++i;
    const int rpw = 64 >> (i < 6 ? i : 6);    // rows per wave
    const int64_t nrows = static_cast<int64_t>(p.batch) * p.dim;
    hipLaunchKernelGGL(kernels[i], dim3(static_cast<unsigned>((nrows + rpw - 1) / rpw)), dim3(64), 0, stream, p);
}

// one planned call: report the kernel, launch it
static int launch(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream) {
    if (!plan.family) return plan.status;
    set_last_kernel(plan.kernel);
    if (p.info) { p.info[0] = plan.family; p.info[1] = plan.info1; }
    const zigma_scan_params_t q = scan_operands(p);
    if (plan.family == ZIGMA_SCAN_KERNEL_GENERIC) {
        ZIGMA_DISPATCH_DTYPE(p.io_dtype, IO, { ZIGMA_DISPATCH_DTYPE(p.bc_dtype, BCT, { launch_generic<IO, BCT>(q, stream); }) })
        return check_launch();
    }
    return p.io_dtype == ZIGMA_BF16 ? launch_scan_tok_bf16(q, plan, stream)
           : p.io_dtype == ZIGMA_F16 ? launch_scan_tok_f16(q, plan, stream) : launch_scan_tok_f32(q, plan, stream);
}

}  // namespace zigma

using namespace zigma;

extern "C" int zigma_selective_scan_fwd(const zigma_scan_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();  // a stale error of an unrelated earlier call is not ours to report
    const zigma_scan_params_t &p = *pp;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return for_each_scan_call(p, [stream](const zigma_scan_params_t &q, const ScanPlan &plan) { return launch(q, plan, stream); });
}

extern "C" int zigma_selective_scan_fwd_plan(const zigma_scan_params_t *pp, const char **kernel) {
    return pp && kernel ? query_scan(*pp, kernel) : ZIGMA_ERR_NULL;
}
