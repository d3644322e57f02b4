/*
 * zigma_hip.h — C ABI of libzigma_hip.so, the MI355X (gfx950) native kernels behind the
 * ZigMa denoiser-forward / ODE-sampling hot path.
 *
 * Drop-in boundary.  Each entry point replaces one native entry of the
 * reference (CompVis/zigma); the parameter blocks mirror the PODs the reference already hands to
 * its CUDA kernels, widened so that token-major (channel-contiguous) layouts and the zigzag row
 * tables can be expressed without a separate index_select pass.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer on the current device;
 *   - the caller owns all memory and allocates the outputs; the library never allocates,
 *     never synchronises, keeps no state a caller depends on and is re-entrant (which kernel variant served a
 *     call is reported through the parameter block's optional `info` out-field; zigma_last_kernel() is a
 *     thread-local DIAGNOSTIC for tests and logs only);
 *   - `stream` is a hipStream_t passed as void*; one call = one or more kernel launches on it;
 *   - strides are in ELEMENTS of the tensor's own dtype;
 *   - returns ZIGMA_OK (0) or a negative zigma_status_t; zigma_strerror() names it.  The Python
 *     shim turns a non-zero status into RuntimeError, as TORCH_CHECK does in the reference.
 */
#ifndef ZIGMA_HIP_H_
#define ZIGMA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZIGMA_ABI_VERSION 11  /* 2: parameter blocks grew (row tables in the backward, checkpoints, reset_period)
                               * 3: scan block: `info` out-field, ZIGMA_SCAN_Z_PREACTIVATED flag; zigma_linear_fwd
                               * 4: zigma_linear_params_t grew (gated residual epilogue); zigma_conv_x_proj_fwd, zigma_q_attn_fwd
                               * 5: pruned — zigma_q_attn_fwd and the dt product of zigma_conv_xproj_params_t removed (measured no faster,
                               *    archived under tools/experiments/)
                               * 6: zigma_cross_attn_bwd / zigma_cross_attn_bwd_chunks added
                               * 7: reset_period in the two backward blocks (zigma_scan_bwd_params_t reuses its padding, zigma_conv_bwd_params_t grew)
                               * 8: zigma_patch_embed_fwd, zigma_timestep_embed_fwd, zigma_final_layer_fwd, zigma_skinny_linear_fwd added
                               * 9: zigma_scan_params_t grew: dt_x / dt_w (dt_proj + softplus inside the scan kernel)
                               * 10: zigma_calib_launch (bench.py's box calibration) added; new ZIGMA_LINEAR_* kernel selectors of round 6
                               * (10, no block changed): zigma_linear_wgrad / zigma_linear_wgrad_workspace_bytes added
                               * (10, no block changed): zigma_linear_f32_split added
                               * (10, no block changed): zigma_norm_linear_fwd / zigma_norm_linear_params_t added
                               * (10, no block changed): zigma_multi_cast_fwd / zigma_multi_cast_params_t added
                               * 11: the host-only plan queries zigma_*_fwd_plan of the Mamba inner's five forward entry points added
                               * (11, no block changed): zigma_optim_* added
                               * (11, no block changed): zigma_final_layer_cfg_fwd / zigma_final_layer_cfg_params_t added
                               * (11, no block changed): zigma_sde_step_fwd / zigma_sde_advance and their blocks added
                               * (11, no block changed): the plan queries zigma_linear_fwd_plan, zigma_norm_linear_fwd_plan, zigma_linear_f32_split_plan added
                               * (11, no block changed): zigma_optim16_* added
                               * (11, no block changed): the plan queries of the operators around the blocks, cross-attention, zigma_scale_reduce_bwd and
                               *    zigma_linear_wgrad added (zigma_patch_embed_fwd_plan ... zigma_linear_wgrad_plan)
                               * (11, no block changed): the plan queries zigma_add_norm_fwd_plan, zigma_add_norm_bwd_plan, zigma_selective_scan_bwd_plan,
                               *    zigma_causal_conv1d_bwd_plan added */

/* zigma_scan_params_t.flags */
#define ZIGMA_SCAN_Z_PREACTIVATED 2   /* z already holds silu(z) (the in_proj GEMM epilogue applied it): out_z = y * z */
#define ZIGMA_SCAN_ACCUMULATE 4        /* out_z += y * silu(z) instead of out_z = ...: the second sweep of the bidirectional `v2` scan type
                                       * (mamba_simple.py:335-339) adds itself to the first one's result; served with dt_x / dt_w only (ABI 10) */
#define ZIGMA_SCAN_PROBE_V1 0x100     /* A/B probe (tools/scan_ab.py): pin the first-generation token-major kernel */
#define ZIGMA_SCAN_PROBE_PRIO_SHIFT 9 /* A/B probe: bit 9 = scan_tok2_kernel WITHOUT its wave-priority rotation */
#define ZIGMA_SCAN_PROBE_R5_SHIFT 10  /* A/B probe: bit 10 = never the six-resident-workgroups form of scan_tok2_kernel */

/* zigma_scan_params_t.info[0]: which kernel family served the call */
#define ZIGMA_SCAN_KERNEL_GENERIC 1
#define ZIGMA_SCAN_KERNEL_TOK 2    /* scan_tok_kernel: token-major, all features (carries, checkpoints, reset_period) */
#define ZIGMA_SCAN_KERNEL_TOK2 3   /* scan_tok2_kernel: token-major hot kernel (16-bit I/O, dstate 16, gate only)      */

typedef enum zigma_status {
    ZIGMA_OK = 0,
    ZIGMA_ERR_NULL = -1,        /* required pointer is NULL                                  */
    ZIGMA_ERR_SHAPE = -2,       /* size out of the supported range                           */
    ZIGMA_ERR_DTYPE = -3,       /* unsupported element type                                  */
    ZIGMA_ERR_STRIDE = -4,      /* layout not supported by any kernel                        */
    ZIGMA_ERR_LAUNCH = -5,      /* hipLaunchKernel / hipGetLastError failed                  */
    ZIGMA_ERR_UNSUPPORTED = -6  /* feature of the reference that is out of scope (complex A) */
} zigma_status_t;

typedef enum zigma_dtype { ZIGMA_F32 = 0, ZIGMA_F16 = 1, ZIGMA_BF16 = 2 } zigma_dtype_t;

/* ------------------------------------------------------------------------------------------
 * Selective scan forward.
 * Replaces  selective_scan_cuda.fwd  (reference dis_mamba/csrc/selective_scan/selective_scan.cpp:226-336,
 * kernel selective_scan_fwd_kernel.cuh:67-303); parameter block mirrors SSMParamsBase
 * (selective_scan.h:26-69).  Real A only (the reference's complex variant is never reached by ZigMa,
 * mamba_simple.py:298).
 *
 *   delta' = delta + delta_bias[d];  if delta_softplus: delta' = delta' <= 20 ? log1p(exp(delta')) : delta'
 *   h_n[l] = exp(delta'[l] * A[d,n]) * h_n[l-1] + delta'[l] * B[n,l] * u[l]
 *   out[l] = sum_n C[n,l] * h_n[l] + D[d] * u[l];      out_z[l] = out[l] * z[l] / (1 + exp(-z[l]))
 *
 * u, delta, z, out, out_z are logically (batch, dim, seqlen) with arbitrary batch/d/l strides:
 *   reference layout  = l_stride 1 (the reference REQUIRES this, selective_scan.cpp:252-253);
 *   token-major layout = d_stride 1, l_stride = row pitch (what the fused ZigMa block uses).
 * Variable B/C are (batch, n_groups, dstate, seqlen); constant B/C are (dim, dstate) float32.
 * x receives the running prefix at every `chunk_len` boundary, (batch, dim, n_chunks, 2*dstate) f32,
 * contiguous: x[b,d,c,2n] = prod_{l<=end(c)} exp(delta' A), x[b,d,c,2n+1] = h_n[end(c)]
 * (selective_scan_fwd_kernel.cuh:251-254); last_state = x[:, :, -1, 1::2].  May be NULL.
 *
 * z_row_index / out_row_index (optional, int32[seqlen]) fuse the zigzag reordering of
 * mamba_simple.py:55-61,362-395 into the kernel's own loads/stores: scan position k reads its gate
 * from row z_row_index[k] of z and writes out/out_z to row out_row_index[k].
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_scan_params {
    int32_t batch, dim, seqlen, dstate, n_groups;
    int32_t is_variable_B, is_variable_C, delta_softplus;
    int32_t io_dtype;   /* zigma_dtype_t of u, delta, z, out, out_z                                */
    int32_t bc_dtype;   /* zigma_dtype_t of VARIABLE B / C (reference: == io_dtype)               */
    int32_t chunk_len;  /* carry spacing for x; 0 -> 2048 (reference: selective_scan.cpp:307)      */
    int32_t flags;      /* 0, ZIGMA_SCAN_Z_PREACTIVATED, ZIGMA_SCAN_ACCUMULATE (+ ZIGMA_SCAN_PROBE_* bits; others must be 0) */

    int64_t u_batch_stride, u_d_stride, u_l_stride;
    int64_t delta_batch_stride, delta_d_stride, delta_l_stride;
    int64_t z_batch_stride, z_d_stride, z_l_stride;
    int64_t out_batch_stride, out_d_stride, out_l_stride;
    int64_t out_z_batch_stride, out_z_d_stride, out_z_l_stride;
    int64_t A_d_stride, A_dstate_stride;
    int64_t B_batch_stride, B_group_stride, B_d_stride, B_dstate_stride, B_l_stride;
    int64_t C_batch_stride, C_group_stride, C_d_stride, C_dstate_stride, C_l_stride;

    const void *u, *delta, *A, *B, *C;
    const void *D;           /* float32 (dim) or NULL  */
    const void *delta_bias;  /* float32 (dim) or NULL  */
    const void *z;           /* or NULL: no gating      */
    void *out;               /* ungated y; may be NULL when z != NULL (only backward needs it)     */
    void *out_z;             /* required iff z != NULL  */
    void *x;                 /* float32 or NULL         */
    const int32_t *z_row_index;
    const int32_t *out_row_index;
    /* optional float32 [batch][dim/64][ceil(seqlen/16)][dstate][64]: the state h BEFORE every 16-step tile, written by the
     * token-major kernel when both out and out_z are requested (the training forward); zigma_selective_scan_bwd takes it
     * back as `checkpoints` and skips its own forward phase.  Ignored (left untouched) by every other kernel variant:
     * pass `info` and check info[1] == 1 before trusting it. */
    float *checkpoints;
    /* > 0: the sequence is a concatenation of independent sequences of this many steps (a multiple of 16): the state is
     * reset to 0 at every multiple.  Lets the video temporal layers (b (t k) c tokens, scan over t for every (b, k)) run as
     * batch = k, seqlen = b * t on strided views with no transposing copy.  Token-major kernel only; x must be NULL. */
    int32_t reset_period;
    int32_t pad2_;
    /* optional HOST pointer to int32[2], written by the call before it returns (never by a kernel):
     * info[0] = ZIGMA_SCAN_KERNEL_* that was launched, info[1] = 1 iff `checkpoints` is being written. */
    int32_t *info;
    /* ABI 9 — dt_proj INSIDE the scan (token-major hot kernel, bf16 / fp16, whole-sequence mode only): when dt_x != NULL, `delta` is ignored and
     *   delta'[b, l, d] = softplus( sum_{r < dt_rank} dt_x[b, l, r] * dt_w[d, r] + delta_bias[d] )
     * is formed by the workgroup itself (v_mfma_f32_16x16x32_bf16 in the tile prologue) from the dt columns of the x_dbl rows it
     * already fetches B_l / C_l from — the (batch, seqlen, dim) delta tensor (reference selective_scan_interface.py:323) is
     * neither written nor read.  dt_x: rows of scan position l (row pitch dt_x_l_stride, 16-byte aligned), dt_w: (dim, dt_rank)
     * rows of pitch dt_w_row_stride (16-byte aligned); 32 <= dt_rank <= 64, dt_rank % 8 == 0, dt_x rows at least 64 wide.
     * delta_softplus must be 1.  ZIGMA_SCAN_Z_PREACTIVATED may be combined with it (round 5). */
    const void *dt_x, *dt_w;
    int64_t dt_x_batch_stride, dt_x_l_stride, dt_w_row_stride;
    int32_t dt_rank, pad3_;
} zigma_scan_params_t;

int zigma_selective_scan_fwd(const zigma_scan_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise causal conv1d (+ bias, + SiLU) forward.
 * Replaces  causal_conv1d_cuda.causal_conv1d_fwd  (reference dis_causal_conv1d/csrc/causal_conv1d.cpp:130-189,
 * kernels causal_conv1d_fwd.cu:39-130,193-298); parameter block mirrors ConvParamsBase
 * (causal_conv1d.h:9-35).
 *
 *   out[b,c,l] = act( bias[c] + sum_{w<width} weight[c,w] * x[b,c,l-(width-1-w)] ),  x[<0] = 0
 *
 * x/out logically (batch, dim, seqlen), arbitrary strides (channel-first, channel-last, views).
 * x_row_index (optional, int32[seqlen]): the conv runs over the REORDERED sequence
 * x'[k] = x[x_row_index[k]]  (zigzag gather of mamba_simple.py:362-370 fused into the loads).
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_conv_params {
    int32_t batch, dim, seqlen, width;
    int32_t silu_activation;
    int32_t io_dtype;  /* x, out */
    int32_t w_dtype;   /* weight, bias */
    int32_t flags;     /* reserved, must be 0 */
    int64_t x_batch_stride, x_c_stride, x_l_stride;
    int64_t weight_c_stride, weight_width_stride;
    int64_t out_batch_stride, out_c_stride, out_l_stride;
    const void *x, *weight;
    const void *bias;  /* or NULL */
    void *out;
    const int32_t *x_row_index;
    /* > 0: independent sequences of this many positions (a multiple of 16) concatenated along seqlen: the causal window
     * does not reach across a multiple (zero padding restarts there).  Token-major kernel only. */
    int32_t reset_period;
    int32_t pad2_;
} zigma_conv_params_t;

int zigma_causal_conv1d_fwd(const zigma_conv_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused (gated-branch add) + residual add + RMSNorm / LayerNorm (+ adaLN modulate) forward.
 * Replaces the Triton kernel `_layer_norm_fwd_1pass_kernel` and its host `_layer_norm_fwd`
 * (reference dis_mamba/mamba_ssm/ops/triton/layernorm.py:65-120,123-177) and, when the optional
 * pointers are given, the elementwise glue of Block.forward around it (model_zigma.py:53-54,388-460).
 *
 * Per row r (batch index b = r / rows_per_batch):
 *   xe  = x[r]  (+ gate[b] * branch[r]          if branch != NULL;  xe is stored to x_out if != NULL)
 *   res = xe (+ residual[r]);  residual_out[r] = res            (float statistics, layernorm.py:98-105)
 *   y   = is_rms ? res * rsqrt(mean(res^2) + eps) : (res - mean) * rsqrt(var + eps)
 *   y   = y * weight (+ bias)                                   (weight/bias may be NULL)
 *   y_out[r] = y                                                (if y_out != NULL)
 *   y_mod[r] = y * (1 + scale[b]) + shift[b]                    (if y_mod != NULL)   modulate()
 * x, branch, x_out, y_out, y_mod share x_dtype; residual/residual_out have res_dtype; weight/bias
 * w_dtype; gate/shift/scale are (batch, cols) rows of mod_dtype with pitch mod_batch_stride.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_norm_params {
    int32_t rows, cols, rows_per_batch;
    int32_t is_rms;
    int32_t x_dtype, res_dtype, w_dtype, mod_dtype;
    float eps;
    int32_t flags;  /* reserved, must be 0 */
    int64_t x_row_stride, branch_row_stride, x_out_row_stride;
    int64_t res_row_stride, res_out_row_stride;
    int64_t y_row_stride, y_mod_row_stride;
    int64_t mod_batch_stride;
    const void *x;
    const void *branch, *gate;  /* both or neither */
    void *x_out;
    const void *residual;       /* or NULL */
    void *residual_out;         /* or NULL */
    const void *weight, *bias;  /* or NULL */
    void *y_out;                /* or NULL */
    const void *shift, *scale;  /* both or neither */
    void *y_mod;                /* required iff shift != NULL */
} zigma_norm_params_t;

int zigma_add_norm_fwd(const zigma_norm_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * dt_proj + bias + softplus on the matrix cores (bf16 or fp16 in / fp32 accumulate / same type out).
 * Replaces the skinny GEMM  delta = delta_proj_weight @ x_dbl[:, :dt_rank].T  of the reference
 * (dis_mamba/mamba_ssm/ops/selective_scan_interface.py:323, K = dt_rank) together with the
 * softplus(delta + delta_bias) its scan kernel applies first (selective_scan_fwd_kernel.cuh:153-156):
 *
 *   out[m, d] = act( sum_{r<k} x[m, r] * w[d, r] + bias[d] ),   act = softplus with pass-through above 20
 *
 * x: (m, >=k) rows of pitch x_row_stride (the first k columns of x_dbl);  w: (n, k) = dt_proj.weight;
 * bias: float32 (n) or NULL;  out: (m, n).  The selective scan is then called with delta_softplus = 0 and
 * delta_bias = NULL.  Limits: dtype bf16 or fp16 (x, w, out alike), k <= 48 and a multiple of 8, n % 64 == 0, x/w rows 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_dtproj_params {
    int64_t m;              /* tokens (batch * seqlen) */
    int32_t n, k;           /* d_inner, dt_rank */
    int32_t dtype;          /* zigma_dtype_t of x, w, out */
    int32_t softplus;       /* 0: plain affine */
    int32_t flags;          /* reserved, must be 0 */
    int32_t pad_;
    int64_t x_row_stride, w_row_stride, out_row_stride;
    const void *x, *w;
    const void *bias;
    void *out;
} zigma_dtproj_params_t;

int zigma_dt_proj_softplus_fwd(const zigma_dtproj_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Selective scan backward (token-major operands, real A, variable B/C, one group).
 * Replaces  selective_scan_cuda.bwd  (reference dis_mamba/csrc/selective_scan/selective_scan.cpp:338-492, kernel
 * selective_scan_bwd_kernel.cuh:59-329, reverse_scan.cuh) for the layout the fused block uses.  Given dout = dL/d(out_z)
 * (or dL/d(out) when z == NULL) it produces (selective_scan_bwd_kernel.cuh:161-329):
 *   g = dout * silu(z);  dz = dout * out * sigmoid(z) * (1 + z (1 - sigmoid(z)))          (out = the forward's UNGATED y)
 *   dh_l = g_l C_l + a_{l+1} dh_{l+1};   dC[b,n,l] = sum_d g_l h_l;   dB[b,n,l] = sum_d dh_l delta'_l u_l
 *   du = g D + delta' sum_n dh B;   ddelta = (sum_n dh (B u + A a h_{l-1})) * softplus'(delta + bias)
 *   dA[d,n] = sum_{b,l} dh delta' a h_{l-1};   dD[d] = sum g u;   ddelta_bias[d] = sum ddelta
 * u, delta, z, out, dout, du, ddelta, dz: (batch, seqlen, dim), channel stride 1, io_dtype; B, C: (batch, dstate, seqlen)
 * logical with arbitrary strides, io_dtype; dB, dC: float32, same logical shape, arbitrary strides (e.g. columns of a
 * float32 d(x_dbl) buffer); dA (dim, dstate), dD (dim), ddelta_bias (dim): float32 contiguous, WRITTEN (not accumulated).
 * The reverse sweep re-creates the states from checkpoints every 16 steps, which the kernel writes itself in a first
 * forward phase: the caller provides `workspace` of zigma_selective_scan_bwd_workspace_bytes() bytes (the library
 * never allocates).  All sums are formed in a fixed order: results are bit-reproducible run to run.
 * Limits: dim % 64 == 0, dstate 16 or 8.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_scan_bwd_params {
    int32_t batch, dim, seqlen, dstate;
    int32_t delta_softplus;
    int32_t io_dtype;
    int32_t flags;           /* reserved, must be 0 */
    int32_t reset_period;    /* > 0 (multiple of 16): every batch row is a concatenation of independent sequences of that many steps,
                              * as in zigma_scan_params_t: the state restarts there and no gradient crosses the boundary */
    int64_t u_batch_stride, u_l_stride;
    int64_t delta_batch_stride, delta_l_stride;
    int64_t z_batch_stride, z_l_stride;
    int64_t out_batch_stride, out_l_stride;
    int64_t dout_batch_stride, dout_l_stride;
    int64_t du_batch_stride, du_l_stride;
    int64_t ddelta_batch_stride, ddelta_l_stride;
    int64_t dz_batch_stride, dz_l_stride;
    int64_t A_d_stride, A_dstate_stride;
    int64_t B_batch_stride, B_dstate_stride, B_l_stride;
    int64_t C_batch_stride, C_dstate_stride, C_l_stride;
    int64_t dB_batch_stride, dB_dstate_stride, dB_l_stride;
    int64_t dC_batch_stride, dC_dstate_stride, dC_l_stride;
    const void *u, *delta, *A, *B, *C;
    const void *D;           /* float32 (dim) or NULL */
    const void *delta_bias;  /* float32 (dim) or NULL */
    const void *z;           /* or NULL */
    const void *out;         /* ungated forward output; required iff z != NULL */
    const void *dout;
    void *du, *ddelta;
    void *dz;                /* required iff z != NULL */
    float *dA, *dB, *dC;
    float *dD;               /* required iff D != NULL */
    float *ddelta_bias;      /* required iff delta_bias != NULL */
    void *workspace;
    int64_t workspace_bytes;
    /* optional int32[seqlen] row tables, the forward's own (zigma_scan_params_t): scan position k reads z from / writes dz
     * to row z_row_index[k], and reads out / dout from row out_row_index[k].  NULL = row k. */
    const int32_t *z_row_index;
    const int32_t *out_row_index;
    /* optional: the checkpoints the forward wrote (zigma_scan_params_t.checkpoints); NULL = recompute them here */
    const float *checkpoints;
} zigma_scan_bwd_params_t;

int64_t zigma_selective_scan_bwd_workspace_bytes(const zigma_scan_bwd_params_t *p);
int zigma_selective_scan_bwd(const zigma_scan_bwd_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise causal conv1d (+ bias, + SiLU) backward, token-major operands.
 * Replaces  causal_conv1d_cuda.causal_conv1d_bwd  (reference dis_causal_conv1d/csrc/causal_conv1d.cpp:191-283,
 * kernels causal_conv1d_bwd.cu:46-240,301-470).  x, dout, dx: (batch, seqlen, dim), channel stride 1, io_dtype;
 * dout is in SCAN order (the order the forward wrote `out` in); x is read through x_row_index exactly as in the
 * forward and dx is scattered through the same table (dx[row[k]] = dx'[k]; the table must be a permutation).
 * dweight (dim, width), dbias (dim): float32 contiguous, WRITTEN.  Sums are formed in a fixed order.
 * workspace: zigma_causal_conv1d_bwd_workspace_bytes() bytes.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_conv_bwd_params {
    int32_t batch, dim, seqlen, width;
    int32_t silu_activation;
    int32_t io_dtype;  /* x, dout, dx */
    int32_t w_dtype;   /* weight, bias */
    int32_t flags;     /* reserved, must be 0 */
    int64_t x_batch_stride, x_l_stride;
    int64_t dout_batch_stride, dout_l_stride;
    int64_t dx_batch_stride, dx_l_stride;
    int64_t weight_c_stride, weight_width_stride;
    const void *x, *weight;
    const void *bias;  /* or NULL */
    const void *dout;
    void *dx;
    float *dweight;
    float *dbias;      /* required iff bias != NULL */
    const int32_t *x_row_index;
    void *workspace;
    int64_t workspace_bytes;
    int32_t reset_period;   /* > 0 (multiple of 16): independent sequences of that many positions along seqlen (zigma_conv_params_t) */
    int32_t pad_;
} zigma_conv_bwd_params_t;

int64_t zigma_causal_conv1d_bwd_workspace_bytes(const zigma_conv_bwd_params_t *p);
int zigma_causal_conv1d_bwd(const zigma_conv_bwd_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * RMSNorm / LayerNorm (+ residual add, prenorm) backward.
 * Replaces `_layer_norm_bwd` + `_layer_norm_bwd_kernel` (reference dis_mamba/mamba_ssm/ops/triton/layernorm.py:196-377).
 * xsum = the tensor that was normalised in the forward (x, or the forward's residual_out = x + residual), res_dtype;
 * mean / rstd are recomputed from it.  dy: gradient of the normalised output (x_dtype); dresidual_out (optional,
 * res_dtype): gradient arriving at the prenorm residual output.  Writes dx (x_dtype) and / or dresidual (res_dtype)
 * — both carry  (wdy - xhat*mean(xhat*wdy) - mean(wdy)) * rstd + dresidual_out  — and dweight / dbias (float32 (cols),
 * WRITTEN, fixed summation order).  workspace: zigma_add_norm_bwd_workspace_bytes() bytes.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_norm_bwd_params {
    int32_t rows, cols;
    int32_t is_rms;
    int32_t x_dtype, res_dtype, w_dtype;
    float eps;
    int32_t flags;           /* reserved, must be 0 */
    int64_t xsum_row_stride, dy_row_stride, dres_out_row_stride, dx_row_stride, dres_row_stride;
    const void *xsum;
    const void *weight;      /* or NULL */
    const void *dy;
    const void *dresidual_out;  /* or NULL */
    void *dx;                /* or NULL */
    void *dresidual;         /* or NULL (at least one of dx / dresidual) */
    float *dweight;          /* or NULL */
    float *dbias;            /* or NULL */
    void *workspace;
    int64_t workspace_bytes;
} zigma_norm_bwd_params_t;

int64_t zigma_add_norm_bwd_workspace_bytes(const zigma_norm_bwd_params_t *p);
int zigma_add_norm_bwd(const zigma_norm_bwd_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the block's elementwise glue (modulate, gated branch add; reference model_zigma.py:53-54,441-458) in one pass:
 *   out[r, :]   = dy[r, :] * (s[r / rows_per_batch, :] + s_add)                       (out may be NULL)
 *   r1[b, c, :] = sum over the 64 rows of chunk c of sample b of dy[r, :] * a[r, :]
 *   r2[b, c, :] = the same sum of dy[r, :]                                              (r2 may be NULL)
 * modulate backward: a = x, s = scale, s_add = 1 (out = dx, sum_c r1 = dscale, sum_c r2 = dshift); gated add backward: a = branch,
 * s = gate, s_add = 0 (out = dbranch, sum_c r1 = dgate).  dy, a, out: (rows, cols) bf16 rows; s: (batch, cols) bf16 rows;
 * r1, r2: float32 [batch][rows_per_batch / 64][cols], summed over the chunks by the caller (fixed order, no float atomics).
 * Limits and refusals: plan_scale_reduce_bwd() of csrc/attn_plan.h (zigma_scale_reduce_bwd_plan below).
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_glue_bwd_params {
    int64_t rows;
    int32_t cols, rows_per_batch;
    int32_t dtype;           /* ZIGMA_BF16 */
    int32_t flags;           /* reserved, must be 0 */
    float s_add;
    int32_t pad_;
    int64_t dy_row_stride, a_row_stride, out_row_stride, s_batch_stride;
    const void *dy, *a, *s;
    void *out;
    void *r1, *r2;
} zigma_glue_bwd_params_t;

int zigma_scale_reduce_bwd(const zigma_glue_bwd_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Cross-attention core over a short context:  out = softmax(scale * Q K^T) V  per (sample, head), no mask.
 * Replaces the scaled_dot_product_attention / xformers call of CrossAttention.forward (reference model_zigma.py:113-127;
 * ZigMa: 8 heads x 64, 77 text tokens).  q, out: (batch, seqlen, heads*head_dim) rows; k, v: (batch, n_ctx, heads*head_dim)
 * rows (any row / batch pitch: e.g. slices of one batched K/V projection); head h = columns [h*head_dim, (h+1)*head_dim).
 * Limits: bf16 or fp16 (q, k, v, out alike), head_dim 64, n_ctx <= 128, rows 16-byte aligned.  Every refusal and the launch geometry, of the forward
 * and of the backward below: plan_cross_attn() / plan_cross_attn_bwd(), csrc/attn_plan.h.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_xattn_params {
    int32_t batch, seqlen, n_ctx, heads, head_dim;
    int32_t dtype;
    int32_t flags;   /* reserved, must be 0 */
    float scale;     /* head_dim^-0.5 in the reference; must be finite and > 0 (else ZIGMA_ERR_UNSUPPORTED) */
    int64_t q_batch_stride, q_row_stride;
    int64_t k_batch_stride, k_row_stride;
    int64_t v_batch_stride, v_row_stride;
    int64_t o_batch_stride, o_row_stride;
    const void *q, *k, *v;
    void *out;
} zigma_xattn_params_t;

int zigma_cross_attn_fwd(const zigma_xattn_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward of zigma_cross_attn_fwd (what autograd derives for the scaled_dot_product_attention call of the reference,
 * model_zigma.py:113-127, when it trains; nothing of the forward is saved — the probabilities are recomputed):
 *   dq (batch, seqlen, heads*head_dim) bf16;  dk_part, dv_part: fp32 partial sums, contiguous
 *   (chunks, batch, n_ctx, heads*head_dim) with chunks = zigma_cross_attn_bwd_chunks(seqlen) — the caller adds the chunks
 *   (deterministic: no atomics).  Same operand layout and limits as the forward; dout has the layout of out.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_xattn_bwd_params {
    int32_t batch, seqlen, n_ctx, heads, head_dim;
    int32_t dtype;
    int32_t flags;   /* reserved, must be 0 */
    float scale;     /* the forward's; must be finite and > 0 (else ZIGMA_ERR_UNSUPPORTED) */
    int32_t chunks;  /* zigma_cross_attn_bwd_chunks(seqlen) */
    int32_t pad_;
    int64_t q_batch_stride, q_row_stride;
    int64_t k_batch_stride, k_row_stride;
    int64_t v_batch_stride, v_row_stride;
    int64_t do_batch_stride, do_row_stride;
    int64_t dq_batch_stride, dq_row_stride;
    const void *q, *k, *v, *dout;
    void *dq, *dk_part, *dv_part;
} zigma_xattn_bwd_params_t;

int zigma_cross_attn_bwd_chunks(int seqlen);
int zigma_cross_attn_bwd(const zigma_xattn_bwd_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * x_proj: out[m, n] = sum_k x[m, k] * w[n, k]  for the skinny projection of the Mamba block (n = dt_rank + 2 d_state).
 * Replaces F.linear(conv1d_out, x_proj_weight) (reference dis_mamba/mamba_ssm/ops/selective_scan_interface.py:318-322).
 * x: (m, k) rows (the conv output u, token-major); w: (n, k) = x_proj.weight; out: (m, n).  bf16 or fp16 in, fp32 accumulate,
 * same type out.  Limits: n <= 96, k % 256 == 0, x / w rows 16-byte aligned.  Below 16 384 rows (and k <= 1536) the library splits K over the
 * waves of 32-row workgroups and adds the partial tiles in a fixed order (round 5); from 16 384 rows on a workgroup streams 256 rows.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_xproj_params {
    int64_t m;
    int32_t n, k;
    int32_t dtype;
    int32_t flags;           /* reserved, must be 0 */
    int64_t x_row_stride, w_row_stride, out_row_stride;
    const void *x, *w;
    void *out;
} zigma_xproj_params_t;

int zigma_x_proj_fwd(const zigma_xproj_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * conv_x_proj: the depthwise causal conv1d (+ bias, SiLU) over the reordered sequence AND x_proj of its result in one pass:
 *   u[b, k, c]   = silu(conv_bias[c] + sum_{w<4} conv_weight[c, w] * x[b, x_row_index[k - 3 + w], c])     (x[<0] = 0)
 *   out[b*L + k, n] = sum_c u[b, k, c] * w[n, c]
 * Replaces causal_conv1d_fn(..., activation="silu") + F.linear(conv1d_out, x_proj_weight) of MambaInnerFn.forward
 * (reference selective_scan_interface.py:307-322) with the gather of mamba_simple.py:362-370 in the loads.  u (needed by
 * the scan) is written once and not read back.  bf16 or fp16 throughout (one dtype), fp32 accumulation; u is rounded to it BEFORE the
 * projection, as in the reference.  x: (batch, seqlen, dim) channel-contiguous rows; conv_weight: (dim, 4) contiguous;
 * conv_bias: (dim); w: (n, dim) rows; u: (batch, seqlen, dim) in scan order; out: (batch * seqlen, n) rows.
 * Limits: width 4, bias required, seqlen % 32 == 0, batch * seqlen % 256 == 0, dim % 64 == 0, n <= 96 and n % 8 == 0, 16-byte
 * aligned rows (x, u, w, out).
 * flags: 0; probes: 1 = three LDS stages, 2 = eight-wave workgroups, 4 / 8 = phases skipped (results wrong).
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_conv_xproj_params {
    int32_t batch, seqlen, dim, n;
    int32_t dtype;           /* ZIGMA_BF16 */
    int32_t flags;
    int64_t x_batch_stride, x_l_stride;
    int64_t u_batch_stride, u_l_stride;
    int64_t w_row_stride, out_row_stride;
    const void *x, *conv_weight, *conv_bias, *w;
    void *u, *out;
    const int32_t *x_row_index;   /* or NULL */
} zigma_conv_xproj_params_t;

int zigma_conv_x_proj_fwd(const zigma_conv_xproj_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dense projection on the matrix cores:  out = x @ w^T (+ bias) (+ SiLU on a column range), bf16 or fp16 in / fp32 accumulate / same type out.
 * Replaces the cuBLAS GEMMs behind F.linear at Mamba.in_proj (reference mamba_simple.py:290-294), out_proj
 * (selective_scan_interface.py:365) and CrossAttention.to_q / to_out (model_zigma.py:104-135).
 * x: (m, k) rows; w: (n, k) rows (nn.Linear layout); out: (m, n) rows; bias: (n) in the operand dtype or NULL.
 * silu_from_col: output columns >= this value leave as silu(value) (in_proj writes silu(z) for the gate half, consumed by
 * the scan under ZIGMA_SCAN_Z_PREACTIVATED); pass n for a plain projection.  Must be a multiple of 32.
 * Limits: bf16 or fp16 (every operand of a call in the one dtype); k % 64 == 0; n % 128 == 0; x / w rows 16-byte aligned, out rows 8-byte aligned.
 * ZIGMA_LINEAR_WS (flags): the weight-stationary kernel (csrc/linear_ws.hip — a panel of w lives in the registers of a workgroup, only
 * the rows of x stream; the in_proj of the default path).  Same result bit for bit.  Limits, else ZIGMA_ERR_UNSUPPORTED: no bias /
 * residual; k = 512 or 640 with 256-feature panels (pw = 256), or — since round 5 — k = 1280 or 1536 with 128-feature panels (pw = 128:
 * out_proj below the tiled kernel's token floor); n % pw == 0 and n <= 8192, m % 512 == 0 with m / 512 >= 32 / (n / pw), x rows a
 * multiple of 128 elements apart, out rows 16-byte aligned.  silu_from_col < n (round 5, pw = 256 only): a multiple of 128 — whole
 * 128-column groups leave as silu(.) of the fp32 accumulator.
 * ZIGMA_LINEAR_SM (flags; round 5): the few-token tiled kernel (csrc/linear_sm.hip: tiles of 128 rows x n / 4 columns, one per workgroup —
 * 8192 rows x 640 columns are exactly 256 tiles).  Same result bit for bit; takes the bias (on an 8-byte boundary) and the gated residual.
 * Limits, else ZIGMA_ERR_UNSUPPORTED: no activation (silu_from_col == n), k % 64 == 0 and k >= 128, m % 128 == 0 (n % 128 == 0: tiles of 160,
 * 192 or 128 columns), out rows 16-byte aligned.
 * Without a selector the library chooses between the 4-wave and the 8-wave tiled kernel.  Every refusal and choice: plan_linear(), csrc/linear_plan.h.
 * ------------------------------------------------------------------------------------------ */
#define ZIGMA_LINEAR_WS 0x4000
#define ZIGMA_LINEAR_SM 0x8000
typedef struct zigma_linear_params {
    int64_t m;
    int32_t n, k;
    int32_t dtype;           /* ZIGMA_BF16 or ZIGMA_F16 */
    int32_t flags;           /* 0, ZIGMA_LINEAR_WS or ZIGMA_LINEAR_SM (other bits: probes of tools/; the shipped library answers them with the 8-wave kernel or refuses them) */
    int32_t silu_from_col;
    int32_t pad_;
    int64_t x_row_stride, w_row_stride, out_row_stride;
    const void *x, *w;
    const void *bias;        /* or NULL */
    void *out;
    /* optional gated residual in the epilogue (ABI 4) — CrossAttention's `hidden + gate_msa * to_out(...)` (model_zigma.py:447-449):
     *   out[m, :] = residual[m, :] + gate[m / rows_per_batch, :] * r16(x @ w^T + bias)[m, :]     (r16: rounded to the operand dtype)
     * residual: (m, n) rows of pitch res_row_stride; gate: (m / rows_per_batch, n) rows of pitch gate_batch_stride, both in the operand dtype;
     * rows_per_batch % 256 == 0.  residual == NULL: plain projection.  The sum is ONE fp32 fma rounded to the operand dtype, r16(fl32(fma(gate, r16(.), residual))),
     * in both dtypes (the 4-wave kernel forms residual + gate * (x @ w^T + bias) from its fp32 accumulator without the inner rounding). */
    const void *residual, *gate;
    int64_t res_row_stride, gate_batch_stride;
    int32_t rows_per_batch, pad2_;
} zigma_linear_params_t;

int zigma_linear_fwd(const zigma_linear_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (no affine weight) + adaLN modulate + dense projection in one pass over x:
 *   y[r, :]   = r16((x[r, :] - mean_r) * rstd_r)                                   (statistics in fp32, two-pass variance over k)
 *   xa[r, :]  = r16(y[r, :] * (1 + scale[b, :]) + shift[b, :]),  b = r / rows_per_batch       (r16: rounded to the I/O type)
 *   out[r, :] = xa[r, :] @ w^T                                                     (fp32 accumulation, rounded once)
 * Replaces the pre-attention `modulate(norm_msa(h), shift_mca, scale_mca)` of the reference's Block (model_zigma.py:441-446) together with
 * CrossAttention.to_q (model_zigma.py:104-128): the arithmetic and the two rounding points of zigma_add_norm_fwd (y_mod) followed by zigma_linear_fwd, but xa
 * is formed in registers as the MFMA operand and never reaches memory.  x: (m, k) rows; w: (n, k) rows; shift / scale: (m / rows_per_batch, k)
 * rows of pitch mod_batch_stride (column slices of a wider tensor pass as they are); out: (m, n) rows of pitch out_row_stride.  The batch index
 * is per row: tiles that straddle a sample boundary are served.  bf16 or fp16 throughout (one dtype).
 * Limits, else ZIGMA_ERR_SHAPE: n = 512, k = 512 / 640 / 768, m % 128 == 0; 16-byte aligned rows of x, w, shift, scale and out, else ZIGMA_ERR_STRIDE.
 * Every refusal and the launch geometry: plan_norm_linear(), csrc/norm_linear_plan.h.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_norm_linear_params {
    int64_t m;
    int32_t n, k;
    int32_t dtype;           /* ZIGMA_BF16 or ZIGMA_F16 */
    int32_t flags;           /* 0 */
    int32_t rows_per_batch;
    float eps;
    int64_t x_row_stride, w_row_stride, out_row_stride, mod_batch_stride;
    const void *x, *w, *shift, *scale;
    void *out;
} zigma_norm_linear_params_t;

int zigma_norm_linear_fwd(const zigma_norm_linear_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Weight gradient of a dense projection:  out[n][k] = sum_m dy[m][n] * x[m][k]  (dW = dY^T X), bf16 or fp16 in / fp32 accumulate.
 * Replaces the GEMM that autograd's linear backward runs for the weight of F.linear at the call sites of zigma_linear_fwd and at
 * x_proj / dt_proj (reference selective_scan_interface.py:318-323).  dy: (m, n) rows of pitch dy_row_stride; x: (m, k) rows of pitch
 * x_row_stride (column views of wider rows pass as they are); out: (n, k) rows of pitch out_row_stride, of the operand type or float32.
 * The tokens are split into `slabs` slabs (0 = the library's choice from the shape); the fp32 slab partials go through the caller's
 * `workspace` of zigma_linear_wgrad_workspace_bytes() bytes (0 when one slab serves; private layout) and are added in ascending slab order,
 * rounded once: no atomics, the result is bit-reproducible.  Nothing outside out[:n, :k] is written.
 * Limits: m >= 1; n, k multiples of 8 up to 8192; row strides multiples of 8 elements; dy, x, out, workspace 16-byte aligned, out rows a
 * multiple of 16 bytes apart.  Every refusal, the slab count and the workspace size: plan_wgrad(), csrc/wgrad_plan.h.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_linear_wgrad_params {
    int64_t m;               /* tokens: the contraction length */
    int32_t n, k;            /* columns of dy, columns of x */
    int32_t dtype;           /* zigma_dtype_t of dy and x: ZIGMA_BF16 or ZIGMA_F16 */
    int32_t out_dtype;       /* `dtype` or ZIGMA_F32 */
    int32_t slabs;           /* 0: chosen by the library; > 0: forced (tests, probes) */
    int32_t flags;           /* reserved, must be 0 */
    int64_t dy_row_stride, x_row_stride, out_row_stride;
    const void *dy, *x;
    void *out;
    void *workspace;
    int64_t workspace_bytes;
} zigma_linear_wgrad_params_t;

int64_t zigma_linear_wgrad_workspace_bytes(const zigma_linear_wgrad_params_t *p);
int zigma_linear_wgrad(const zigma_linear_wgrad_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * fp32 projection on the bf16 matrix cores by splitting:  out = x @ W^T (+ bias), x / bias / out float32, W as two bf16 planes.
 * split(a) of a finite fp32 a: hi = bf16_rne(a) (clamped to the largest finite bf16, never infinite), lo = bf16_rne(a - float(hi)); a
 * non-finite a: hi = bf16(a), lo = 0.  The caller splits the (static) weight once into w_hi / w_lo; x is split inside the kernel on its way
 * from global memory to LDS.
 *   passes == 3 ("high", bf16 x 3):  out = sum_k (x_hi w_hi + x_lo w_hi + x_hi w_lo) + bias   (lo x lo is omitted)
 *   passes == 1 ("medium"):          out = sum_k x_hi w_hi + bias                             (w_lo is not read, may be NULL)
 * All products are v_mfma_f32_32x32x16_bf16 with fp32 accumulators: one for hi x hi, a second one for the two cross terms, added at the end.
 * Consequences of the definition at the ends of the range (tests/test_gpu_matmul_sweep.py holds them bit for bit):
 *   - float(hi) + float(lo) is formed exactly in fp32 for every finite a below the clamp, so with a unit weight "high" returns hi + lo itself
 *     and "medium" returns float(hi);
 *   - from the largest finite bf16 (0x7f7f0000) upwards hi stays 0x7f7f and lo takes the rest: split(FLT_MAX) is hi = 0x7f7f, lo = 2^120, whose
 *     sum is 2^128: "high" with a unit weight returns +inf for an x of FLT_MAX (-inf for -FLT_MAX), although no plane holds an infinity.
 *     Every product whose true value stays inside fp32 is unaffected (a weight of 1/2 returns 2^127);
 *   - below 2^-117 lo lies on the bf16 subnormal grid (spacing 2^-133), below 2^-126 hi does too: hi + lo misses a by up to 2^-134 whatever
 *     its size, and an fp32 subnormal keeps about 7 significant bits.  Subnormals are not flushed: the planes, the products and the fp32
 *     accumulators hold them (measured on the MI355X with selection weights).
 * x: (m, k) rows of pitch x_row_stride; w_hi / w_lo: (n, k) rows of pitch w_*_row_stride; out: (m, n) rows of pitch out_row_stride (views of
 * wider rows pass as they are); bias (n) or NULL.  Nothing outside out[:m, :n] is written; a partly filled last token tile is predicated.
 * Errors, decided before anything touches the device: NULL block / x / w_hi / out (w_lo with passes == 3) -> ZIGMA_ERR_NULL; flags != 0 or
 * passes not 1 or 3 -> ZIGMA_ERR_UNSUPPORTED; m < 0, m % 8, n % 128, k % 64, n or k < 1 or > 65536, a row stride below the width ->
 * ZIGMA_ERR_SHAPE; pointers or rows not 16-byte aligned -> ZIGMA_ERR_STRIDE; m == 0 -> ZIGMA_OK without a launch.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_linear_split_params {
    int64_t m;               /* tokens */
    int32_t n, k;            /* output features (rows of W), input features */
    int32_t passes;          /* 3: bf16 x 3 ("high");  1: hi x hi only ("medium") */
    int32_t flags;           /* reserved, must be 0 */
    int64_t x_row_stride, w_hi_row_stride, w_lo_row_stride, out_row_stride;   /* in elements */
    const void *x;           /* float32 */
    const void *w_hi, *w_lo; /* bf16 */
    const void *bias;        /* float32 or NULL */
    void *out;               /* float32 */
} zigma_linear_split_params_t;

int zigma_linear_f32_split(const zigma_linear_split_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * The small per-forward operators around the blocks (bf16 models; each replaces a chain of library GEMM + ATen elementwise launches):
 *
 * zigma_patch_embed_fwd: PatchEmbed (a conv with kernel == stride; timm, call site model_zigma.py:608-614,924) + bias, and the
 *   position table of model_zigma.py:939-940:  out[b, l, :] = bf16(bf16(W x_patch(b, l) + bias) + pos[l, :]).
 *   x (batch, in_chans, height, width) with element strides (w stride 1); weight (embed_dim, in_chans * patch * patch) contiguous;
 *   bias (embed_dim) or NULL; pos (L, embed_dim) rows of pitch pos_row_stride or NULL; out (batch, L, embed_dim), L = (h / p)(w / p).
 *   Limits: embed_dim % 8 == 0, in_chans * patch^2 * embed_dim * 4 <= 64 KB, out / pos / bias 16-byte aligned.
 * zigma_timestep_embed_fwd: TimestepEmbedder.timestep_embedding (model_zigma.py:247-268): out[b] = [cos(t_b f), sin(t_b f)] with t and the
 *   dim / 2 frequencies f in the model dtype, product and functions in fp32.
 * zigma_final_layer_fwd: FinalLayer without conditioning (model_zigma.py:313-337): out = Linear(LayerNorm(x, no affine, eps)), n_out <= 16,
 *   cols % 8 == 0, cols <= 2048; x rows 16-byte aligned; out (rows, n_out) rows of pitch out_row_stride.
 * zigma_skinny_linear_fwd: out = act(x) W^T + bias for m <= 64 rows (the timestep MLP :232-275 and the adaLN modulation :441, :447 of all
 *   blocks in one call); flags bit 0: act = SiLU (rounded to bf16 like the reference's module), else identity.
 *   Limits: n % 16 == 0, k % 128 == 0, k <= 1024; x, w rows 16-byte aligned, out rows 8-byte aligned, bias 8-byte aligned.
 * Every refusal of the four, in its order, and the launch geometry: plan_patch_embed() ... plan_skinny_linear(), csrc/outer_plan.h.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_patch_embed_params {
    int32_t batch, in_chans, height, width, patch, embed_dim;
    int32_t dtype;   /* ZIGMA_BF16 */
    int32_t flags;   /* reserved, must be 0 */
    int64_t x_batch_stride, x_chan_stride, x_row_stride;
    int64_t pos_row_stride, out_batch_stride, out_row_stride;
    const void *x, *weight, *bias, *pos;
    void *out;
} zigma_patch_embed_params_t;

typedef struct zigma_timestep_embed_params {
    int32_t batch, dim;
    int32_t dtype;   /* ZIGMA_BF16 */
    int32_t flags;   /* reserved, must be 0 */
    int64_t out_row_stride;
    const void *t, *freqs;
    void *out;
} zigma_timestep_embed_params_t;

typedef struct zigma_final_layer_params {
    int64_t rows;
    int32_t cols, n_out;
    int32_t dtype;   /* ZIGMA_BF16 */
    int32_t flags;   /* reserved, must be 0 */
    float eps;
    int32_t pad_;
    int64_t x_row_stride, out_row_stride;
    const void *x, *weight, *bias;
    void *out;
} zigma_final_layer_params_t;

typedef struct zigma_skinny_params {
    int32_t m, n, k;
    int32_t dtype;   /* ZIGMA_BF16 */
    int32_t flags;   /* bit 0: SiLU on x */
    int32_t pad_;
    int64_t x_row_stride, w_row_stride, out_row_stride;
    const void *x, *w, *bias;
    void *out;
} zigma_skinny_params_t;

int zigma_patch_embed_fwd(const zigma_patch_embed_params_t *p, void *stream);
int zigma_timestep_embed_fwd(const zigma_timestep_embed_params_t *p, void *stream);
int zigma_final_layer_fwd(const zigma_final_layer_params_t *p, void *stream);
int zigma_skinny_linear_fwd(const zigma_skinny_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * The final layer of a GUIDED evaluation (classifier-free guidance; csrc/embed.hip).  (ABI 11, no block changed.)  The reference has no such
 * entry: its forward_with_cfg is a stub (model_zigma.py:992-993).  For every row pair (x_cond[r], x_uncond[r]), r < rows:
 *
 *   y_c, y_u = bf16(LayerNorm(x, no affine, eps))                      statistics, rounding and dot product exactly as zigma_final_layer_fwd
 *   vc = w y_c + bias,  vu = w y_u + bias                              fp32 accumulators
 *   out = round_to(out_dtype, fma(scale[n], vc - vu, vu))              ONE rounding; n = r / rows_per_sample
 *
 * stored in the unpatchified latent layout (the index map of unpatchify / unpatchify_video, model_zigma.py:585-598): row r is token (h, w) of
 * frame f of sample n (f = (r % rows_per_sample) / tokens_per_frame, h = token / grid_w, w = token % grid_w), and its output
 * o = (i * patch + j) * chans + c goes to out[n * out_sample_stride + f * out_frame_stride + c * out_chan_stride + (h * patch + i) * out_row_stride
 * + w * patch + j] (element strides, 64-bit offsets; images are one frame).  Neither a 16-bit velocity tensor, nor the permuting copy, the cast, the
 * split or the combination exist as launches.
 *   x_cond, x_uncond  bf16 (rows, cols), rows of pitch x_row_stride: the two halves of one (2B, L, E) tensor; the same pointer twice is legal
 *   weight, bias      bf16 (n_out, cols) contiguous, (n_out) or NULL
 *   scale             DEVICE pointer, fp32, rows / rows_per_sample values (one per sample): a captured graph follows a value changed in place
 *   out               out_dtype: ZIGMA_F32 or ZIGMA_BF16
 *   y_out             NULL, or bf16 (2 rows, cols) contiguous, 16-byte aligned: receives the bf16 LayerNorm rows, cond rows first (a test hook)
 * Limits: those of zigma_final_layer_fwd (cols % 8 == 0, cols <= 2048, n_out <= 16, x rows and weight 16-byte aligned).
 * Checked in this order, before any launch: NULL block ZIGMA_ERR_NULL; rows < 0, cols < 8, n_out < 1 ZIGMA_ERR_SHAPE; flags != 0
 * ZIGMA_ERR_UNSUPPORTED; dtype other than ZIGMA_BF16, out_dtype other than ZIGMA_F32 / ZIGMA_BF16 ZIGMA_ERR_DTYPE; cols % 8, cols > 2048,
 * n_out > 16, a geometry field < 1, n_out != patch^2 chans, rows % rows_per_sample, rows_per_sample % tokens_per_frame, tokens_per_frame % grid_w
 * ZIGMA_ERR_SHAPE; rows == 0 ZIGMA_OK, nothing touched; NULL x_cond / x_uncond / weight / scale / out ZIGMA_ERR_NULL; alignment ZIGMA_ERR_STRIDE:
 * plan_final_layer_cfg(), csrc/outer_plan.h.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_final_layer_cfg_params {
    int64_t rows;            /* rows of EACH half */
    int32_t cols, n_out;
    int32_t dtype;           /* ZIGMA_BF16: x_cond, x_uncond, weight, bias, y_out */
    int32_t out_dtype;       /* ZIGMA_F32 or ZIGMA_BF16 */
    int32_t flags;           /* reserved, must be 0 */
    float eps;
    int32_t rows_per_sample, tokens_per_frame, grid_w, patch, chans;
    int32_t pad_;
    int64_t x_row_stride;
    int64_t out_sample_stride, out_frame_stride, out_chan_stride, out_row_stride;   /* the pixel column stride is 1 */
    const void *x_cond, *x_uncond, *weight, *bias;
    const float *scale;
    void *out;
    void *y_out;
} zigma_final_layer_cfg_params_t;

int zigma_final_layer_cfg_fwd(const zigma_final_layer_cfg_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Box calibration (bench.py `box_calib`; csrc/calib.hip).  NOT part of the drop-in surface: no reference interface maps to it.  Two fixed
 * kernels whose times tell a slower box from slower code between rounds: mode 0 copies `bytes` (a multiple of 4096, 16-byte aligned
 * pointers) from src to dst; mode 1 / 2 run `iters` x 16 v_fma_f32 / `iters` x 8 v_exp_f32 per wave on 1280 workgroups of 4 waves (5 waves
 * per SIMD on 256 CUs) and write one float per thread to dst (`bytes` >= 1280 * 256 * 4 is the size of that buffer).
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_calib_params {
    int32_t mode, iters;
    int64_t bytes;
    const void *src;
    void *dst;
} zigma_calib_params_t;
int zigma_calib_launch(const zigma_calib_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rounding of MANY float32 tensors to one 16-bit type in ONE launch (csrc/multi_cast.hip): the 16-bit copies of an fp32 model's matrix
 * weights that mixed-precision training (torch.autocast) refreshes once per optimizer step — the work of the reference's per-op autocast
 * casts (`custom_fwd(cast_inputs=...)`, selective_scan_interface.py:295-312), table-driven.  (ABI 10, no block changed.)
 *
 *   table      n_entries x {src, dst, numel} in DEVICE memory: dst[i] = round_to_nearest_even(src[i]), i < numel.  numel == 0 is legal.
 *              Only the natural alignment of the element types is assumed (4 bytes for src, 2 for dst).
 *   chunk_map  n_chunks x {entry, offset} in DEVICE memory: workgroup w converts elements [offset, min(offset + chunk, numel)) of table[entry].
 *              The host splits every tensor into pieces of `chunk` elements; a map row whose entry or offset lies outside the table is skipped.
 *   chunk      elements per workgroup: a multiple of 8 in 8 ... 65536.
 * A workgroup whose source and destination pieces both start on 16-byte boundaries moves 8 elements per lane and access (two 16-byte loads,
 * one 16-byte store) and finishes the last numel % 8 elements one by one; any other piece goes element by element.  The choice is uniform
 * over the workgroup.  NaN stays NaN; every other input gives the bits of the other kernels' roundings (zigma_common.h from_float).
 * Checked in this order, before any launch: negative counts (or more than 2^31 - 1 chunks) ZIGMA_ERR_SHAPE; out_dtype other than ZIGMA_BF16 /
 * ZIGMA_F16 ZIGMA_ERR_DTYPE; non-zero flags ZIGMA_ERR_UNSUPPORTED; n_entries == 0 or n_chunks == 0: nothing is launched, ZIGMA_OK (table and
 * chunk_map may then be NULL); NULL table / chunk_map ZIGMA_ERR_NULL; a chunk outside its range ZIGMA_ERR_SHAPE.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_multi_cast_entry {
    const float *src;
    void *dst;
    int64_t numel;
} zigma_multi_cast_entry_t;

typedef struct zigma_multi_cast_chunk {
    int64_t entry;    /* index into the table */
    int64_t offset;   /* first element of the piece */
} zigma_multi_cast_chunk_t;

typedef struct zigma_multi_cast_params {
    const zigma_multi_cast_entry_t *table;
    const zigma_multi_cast_chunk_t *chunk_map;
    int64_t n_entries, n_chunks;
    int32_t out_dtype;   /* ZIGMA_BF16 or ZIGMA_F16 */
    int32_t chunk;       /* elements per workgroup */
    int32_t flags;       /* reserved, must be 0 */
    int32_t pad_;
} zigma_multi_cast_params_t;
int zigma_multi_cast_fwd(const zigma_multi_cast_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * The tail of a training step over MANY float32 parameters in one pass (csrc/optim_step.hip): global-norm gradient clipping, AdamW with
 * decoupled weight decay, the exponential moving average of the parameters and the refresh of their 16-bit copies — the work of the
 * reference's `opt.step()`, `grad_clip(...)`, `update_ema(...)` (train_acc.py:443-448, utils/train_utils.py:103-133) and of one
 * zigma_multi_cast_fwd.  Table-driven like the cast; three launches on ONE parameter block.  (ABI 11, no block changed.)
 *
 *   table      n_entries x zigma_optim_row_t in DEVICE memory.  p, g, m, v are float32 and required per row; ema (float32) and shadow
 *              (elements of shadow_dtype) may be NULL per row.  Only natural alignment is assumed.  numel == 0 is legal.
 *   chunk_map  n_chunks x {entry, offset} in DEVICE memory, the rows of zigma_multi_cast_chunk_t: workgroup w owns elements
 *              [offset, min(offset + chunk, numel)) of table[entry].  A map row whose entry or offset lies outside the table is skipped:
 *              no pointer of the table is followed for it (the sum-of-squares pass stores 0 as that workgroup's partial sum).
 *   partials   n_chunks floats in DEVICE memory: the per-workgroup sums of squares.  NULL for the prepare call means that no
 *              sum-of-squares pass ran: there is no norm (grad_norm reads NaN), nothing is clipped, and only found_inf can skip the step.
 *   state      one zigma_optim_state_t in DEVICE memory; `step` is read and written, the rest written by the prepare call.
 *   grad_scale, found_inf   optional DEVICE float scalars (what torch.amp.GradScaler hands an optimizer): the gradients are divided by
 *              *grad_scale, and a non-zero *found_inf skips the step.
 *
 * zigma_optim_grad_sumsq   grid n_chunks: partials[w] = the float32 sum of g[i]^2 over workgroup w's piece; each lane sums its elements, then
 *              the wave, then the four waves through LDS, in a fixed order and without atomics: bit-identical from run to run.
 * zigma_optim_prepare      one workgroup: sum = partials summed in double in a fixed order; norm = sqrt(sum) / grad_scale;
 *              skipped = (found_inf && *found_inf != 0) || !isfinite(norm).  If not skipped: step += 1;
 *              clip = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1; grad_mult = clip / grad_scale;
 *              step_size = lr / (1 - beta1^step); bc2_sqrt = sqrt(1 - beta2^step), both formed in double.  If skipped, step keeps its
 *              value and grad_mult = step_size = 0, bc2_sqrt = 1.
 * zigma_optim_adamw        grid n_chunks: returns before any store if state->skipped; else per element, in float32 and in this order:
 *                  g = grad * grad_mult;  p -= (lr * weight_decay) * p;  m += (g - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g * g;
 *                  p -= step_size * m / (sqrt(v) / bc2_sqrt + eps);  ema += (p - ema) * (1 - ema_decay);  shadow = round_to_nearest_even(p)
 *              (the constants rounded to float32 from their double values; the bits of the cast kernel for the shadow).  The gradient is
 *              never written.  A workgroup whose present streams all start on 16-byte boundaries moves 8 elements per lane and
 *              iteration and finishes the last numel % 8 one by one; any other piece goes element by element.
 *
 * Checked in this order by all three, before any launch: negative counts (or more than 2^31 - 1 chunks) ZIGMA_ERR_SHAPE; shadow_dtype other
 * than ZIGMA_BF16 / ZIGMA_F16 / -1 (no shadows) ZIGMA_ERR_DTYPE; non-zero flags ZIGMA_ERR_UNSUPPORTED; n_entries == 0 or n_chunks == 0:
 * nothing is launched, ZIGMA_OK; a NULL pointer among those the call uses (sumsq: table, chunk_map, partials; prepare: state; adamw: table,
 * chunk_map, state) ZIGMA_ERR_NULL; a chunk that is not a multiple of 8 in 8 ... 65536 ZIGMA_ERR_SHAPE; beta1 or beta2 outside [0, 1),
 * eps <= 0, a non-finite lr (or weight_decay, max_grad_norm, ema_decay; NaN anywhere) ZIGMA_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
typedef struct zigma_optim_row {
    float *p;            /* parameter                          */
    const float *g;      /* gradient: read only                */
    float *m;            /* exp_avg                            */
    float *v;            /* exp_avg_sq                         */
    float *ema;          /* moving average of p, or NULL       */
    void *shadow;        /* 16-bit copy of p, or NULL          */
    int64_t numel;
    int64_t pad_;        /* rows are 64 bytes                  */
} zigma_optim_row_t;

typedef struct zigma_optim_state {
    float step;          /* steps taken (a float, like the step tensors of torch's fused / capturable optimizers) */
    int32_t skipped;     /* 1: the last step changed nothing   */
    float grad_norm;     /* global L2 norm of the unscaled gradients before clipping (NaN: not computed) */
    float grad_mult;     /* clip / grad_scale                  */
    float step_size;     /* lr / (1 - beta1^step)              */
    float bc2_sqrt;      /* sqrt(1 - beta2^step)               */
    int32_t pad_[2];
} zigma_optim_state_t;

typedef struct zigma_optim_params {
    const zigma_optim_row_t *table;
    const zigma_multi_cast_chunk_t *chunk_map;
    int64_t n_entries, n_chunks;
    float *partials;
    zigma_optim_state_t *state;
    const float *grad_scale;
    const float *found_inf;
    double lr, beta1, beta2, eps, weight_decay;
    double max_grad_norm;   /* <= 0: no clipping */
    double ema_decay;
    int32_t shadow_dtype;   /* ZIGMA_BF16, ZIGMA_F16, or -1: no row has a shadow (the column is ignored) */
    int32_t chunk;          /* elements per workgroup */
    int32_t flags;          /* reserved, must be 0 */
    int32_t pad_;
} zigma_optim_params_t;
int zigma_optim_grad_sumsq(const zigma_optim_params_t *p, void *stream);
int zigma_optim_prepare(const zigma_optim_params_t *p, void *stream);
int zigma_optim_adamw(const zigma_optim_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * The same tail for a pure bfloat16 model (csrc/optim_step.hip).  (ABI 11, no block changed.)  Parameters and gradients are bf16; both moments
 * and the optional moving average are float32; the update is formed in float32 and the parameter written back with STOCHASTIC ROUNDING drawn
 * inside the kernel, so that the expectation of the stored bf16 value is the float32 value (round-to-nearest drops every update below half
 * an ulp: at lr = 1e-4 a weight of 1.0 never moves).  Three launches: zigma_optim16_grad_sumsq, the EXISTING zigma_optim_prepare (the
 * caller fills a zigma_optim_params_t with the same partials, n_chunks, state and hyperparameters), zigma_optim16_adamw.
 *
 *   table      n_entries x zigma_optim16_row_t in DEVICE memory.  p and g are bf16, m and v float32, all four required; ema (float32) may
 *              be NULL per row.  Only natural alignment is assumed.  numel == 0 is legal.  dbg_x32 / dbg_bits are test hooks, NULL in
 *              production: numel floats that receive the float32 value of every element before its rounding, and numel uint16 that receive
 *              the 16 random bits every element's rounding used (not written with ZIGMA_OPTIM16_NEAREST).  Neither is written on a skipped step.
 *   chunk_map  as for zigma_optim_*: rows of zigma_multi_cast_chunk_t.  A map row whose entry or offset lies outside the table, or whose
 *              offset is no multiple of 8, is skipped; so is every map row of a table row that has a NULL p, g, m or v, or whose numel is
 *              above max_numel.  The table lives in device memory, where the host cannot read it without waiting for the device: these two
 *              refusals are the kernels' (no pointer of such a row is followed, the sum-of-squares pass stores 0 for it), not a status.
 *   max_numel  the largest numel of the table, as the host that built it states it.  Needed because an element's random bits are addressed
 *              by a 32-bit octet index: 2^35 elements or more are refused.
 *   partials, state   as for zigma_optim_*; the state block is the same zigma_optim_state_t.
 *   seed_lo, seed_hi, stream   the Philox key and counter word 3.
 *   flags      ZIGMA_OPTIM16_NEAREST: the parameter is stored as round_to_nearest_even(x) (from_float<BF16>), and no Philox work is done.
 *
 * zigma_optim16_grad_sumsq   multi_sumsq_kernel over bf16 gradients: 8 elements per 16-byte load where the piece starts on a 16-byte boundary,
 *              element by element otherwise; lane, then wave, then the four waves, in a fixed order and without atomics.  Writes `partials` in
 *              the layout zigma_optim_prepare reads.
 * zigma_optim16_adamw        grid n_chunks: returns before any store if state->skipped; else per element, in float32:
 *                  p32 = widen(p), g32 = widen(g)          (exact)
 *                  the arithmetic of zigma_optim_adamw on (p32, g32, m, v), in its order (the decay as two roundings, m, v, then p) -> x
 *                  ema += (x - ema) * (1 - ema_decay)      (the float32 x, not its rounding)
 *                  p = SR(x)
 *              The gradient is never written.  A workgroup whose present streams all start on 16-byte boundaries moves 8 elements per lane and
 *              iteration (one 16-byte load each for p and g, two for each float32 stream) and finishes the last numel % 8 one by one; any other
 *              piece goes element by element.  16 bytes read and 14 written per element with the moving average.
 *
 * The rounding.  Let u be the bits of the float32 x.  If the exponent field of u is all ones (inf, NaN), p = from_float<BF16>(x) and no random
 * bits are used.  Otherwise p = (u + r) >> 16 with r uniform in [0, 65535].  In sign-magnitude this rounds AWAY from zero with probability
 * (u & 0xffff) / 65536 and towards zero otherwise: E[p] = x exactly, and a bf16-representable x is kept for every r.  A carry out of the largest
 * finite value gives +-inf, as round-to-nearest would.
 *
 * The random bits.  Element i of a tensor (its index in the TENSOR, not in the workgroup's piece) belongs to octet o = i >> 3.
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (o, pid, step, stream), key = (seed_lo, seed_hi))          (the generator of zigma_sde_step_fwd)
 * and element j = i & 7 takes word j >> 1: its low half if j is even, its high half if j is odd.  `pid` is the row's parameter id (its low 32
 * bits); `step` is state->step after the prepare launch's increment, converted to uint32.  The counter of the state block is a float32 scalar:
 * it is exact, and the bits of successive steps distinct, below 2^24 steps.  Chunk offsets are multiples of 8, so the 8-per-lane loop (one
 * Philox call per lane and iteration), its tail and the element-by-element path draw the same bits for the same element.
 *
 * Checked in this order by both, before any launch: NULL block ZIGMA_ERR_NULL; a NULL pointer among those the call uses (sumsq: table,
 * chunk_map, partials; adamw: table, chunk_map, state) ZIGMA_ERR_NULL; negative counts (or more than 2^31 - 1 chunks) ZIGMA_ERR_SHAPE;
 * max_numel < 0 or >= 2^35 ZIGMA_ERR_SHAPE; a chunk that is not a multiple of 8 in 8 ... 65536 ZIGMA_ERR_SHAPE; flag bits other than
 * ZIGMA_OPTIM16_NEAREST ZIGMA_ERR_UNSUPPORTED; beta1 or beta2 outside [0, 1), eps <= 0, a non-finite lr (or weight_decay, max_grad_norm,
 * ema_decay; NaN anywhere) ZIGMA_ERR_UNSUPPORTED; then n_entries == 0 or n_chunks == 0: nothing is launched, ZIGMA_OK.
 * ------------------------------------------------------------------------------------------ */
#define ZIGMA_OPTIM16_NEAREST 1    /* zigma_optim16_params_t.flags: round to nearest even, no random bits */

typedef struct zigma_optim16_row {
    void *p;             /* parameter, bf16                    */
    const void *g;       /* gradient, bf16: read only          */
    float *m;            /* exp_avg                            */
    float *v;            /* exp_avg_sq                         */
    float *ema;          /* moving average of p, or NULL       */
    int64_t numel;
    int64_t pid;         /* parameter id: counter word 1       */
    float *dbg_x32;      /* test hook or NULL                  */
    uint16_t *dbg_bits;  /* test hook or NULL                  */
    int64_t pad_;        /* rows are 80 bytes                  */
} zigma_optim16_row_t;

typedef struct zigma_optim16_params {
    const zigma_optim16_row_t *table;
    const zigma_multi_cast_chunk_t *chunk_map;
    int64_t n_entries, n_chunks;
    int64_t max_numel;
    float *partials;
    zigma_optim_state_t *state;
    double lr, beta1, beta2, eps, weight_decay;
    double max_grad_norm;   /* <= 0: no clipping (read by zigma_optim_prepare from ITS block; checked here) */
    double ema_decay;
    uint32_t seed_lo, seed_hi;   /* the Philox key                  */
    uint32_t stream;             /* counter word 3                  */
    int32_t chunk;               /* elements per workgroup          */
    int32_t flags;               /* ZIGMA_OPTIM16_NEAREST           */
    int32_t pad_;
} zigma_optim16_params_t;
int zigma_optim16_grad_sumsq(const zigma_optim16_params_t *p, void *stream);
int zigma_optim16_adamw(const zigma_optim16_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * One launch of an SDE sampler's step on the device (csrc/sde_step.hip).  (ABI 11, no block changed.)  The reference draws every Wiener
 * increment with the CPU generator and copies it to the device (transport/integrators.py:24,38); here the noise is a counter-based function
 * of (seed, stream, step, element) evaluated inside the kernel, and every host value of a step lives in device memory, so one captured graph
 * replays for every step of a trajectory.  Over n contiguous elements:
 *
 *   out[i] = c0 a[i] + c1 b[i] + c2 c[i] + cn xi[i]            (c0, c1, c2, cn) = coef[4 r .. 4 r + 3]
 *
 * evaluated in fp32 as  acc = +0;  acc = fma(cn, xi, acc);  acc = fma(c2, c, acc);  acc = fma(c1, b, acc);  acc = fma(c0, a, acc)  (a missing
 * term is skipped; with none present out = 0), rounded once to `dtype` on the store.
 *   a, b, c     `dtype` (ZIGMA_F32 / ZIGMA_BF16 / ZIGMA_F16), n elements; each may be NULL: its term is skipped, its coefficient is never read
 *               as a factor and the operand never loaded
 *   out         `dtype`, n elements.  out == a is legal (the in-place update: every lane loads its own elements before it stores them); any
 *               OTHER overlap of out with a, b or c is the caller's error and is not detected
 *   coef        DEVICE table, coef_rows rows of four fp32.  The row r is  state->step * rows_per_step + row,  or `row` itself with
 *               ZIGMA_SDE_ROW_ABSOLUTE; a relative row past the table is clamped to the last row (a replay too many reads memory that exists)
 *   state       one zigma_sde_state_t in DEVICE memory: the Philox key (seed_lo, seed_hi), the stream and the step counter.  Read only.
 *               May be NULL with ZIGMA_SDE_ROW_ABSOLUTE and bits_out == NULL: the caller then promises cn == 0, and the kernel adds no noise
 *               whatever the row says (NULL is never followed)
 *   bits_out    NULL, or uint32, 4 * ceil(n / 4) words: receives the raw Philox words of every quad the call touches (a test hook).  Not
 *               written when cn == 0, since no Philox work is done then
 *   elem_offset the index of element 0 in the logical noise field: a multiple of 4, >= 0.  Several calls can share one field
 *
 * The noise.  Element i belongs to quad q = (elem_offset + i) / 4 and takes normal number (elem_offset + i) % 4 of it.  The quad's four words are
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = (q & 0xffffffff, q >> 32, step, stream), key = (seed_lo, seed_hi))
 * (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds).  Words (r0, r1) give normals
 * 0 and 1, words (r2, r3) normals 2 and 3, each pair by Box-Muller on
 *   u = ((ra >> 8) + 1) * 2^-24     in (0, 1], never 0, exact in fp32
 *   x = (rb >> 8) * 2^-23           in [0, 2), exact in fp32: the angle is pi x
 *   rho = sqrtf(-2 logf(u));   (s, k) = sincospif(x);   normal_even = rho * k,   normal_odd = rho * s
 * with the accurate library logf / sqrtf / sincospif.  u >= 2^-24 bounds |normal| by sqrt(48 ln 2) = 5.768; u == 1 gives exactly 0.
 * With cn == 0 in the selected row no Philox work is done.
 *
 * Access: every lane owns 8 consecutive elements: one 16-byte access per operand in the 16-bit types, two in fp32; the last n % 8 elements of
 * a call go one by one.  Nothing is read or written past element n - 1, except that bits_out always receives whole quads.
 * Checked in this order, before any launch: NULL block ZIGMA_ERR_NULL; n < 0 (or more than 2^31 - 1 workgroups of 2048 elements)
 * ZIGMA_ERR_SHAPE; elem_offset < 0, elem_offset % 4 or elem_offset + n past 2^63 - 1 ZIGMA_ERR_SHAPE; rows_per_step < 1 ZIGMA_ERR_SHAPE; row < 0 ZIGMA_ERR_SHAPE; coef_rows < 1, or an
 * absolute row >= coef_rows ZIGMA_ERR_SHAPE; unknown flags ZIGMA_ERR_UNSUPPORTED; a dtype outside the three ZIGMA_ERR_DTYPE; n == 0 ZIGMA_OK,
 * nothing touched; NULL out or coef ZIGMA_ERR_NULL; NULL state where it is needed (a relative row, or bits_out given) ZIGMA_ERR_NULL; a, b, c,
 * out, coef, state or bits_out not 16-byte aligned ZIGMA_ERR_STRIDE.
 *
 * zigma_sde_advance: one workgroup, stream-ordered after the step's launches.  state->step += 1; then, with r = min(step, n_rows - 1),
 *   t_out[j * batch + b] = times[r * n_t + j]        j < n_t, b < batch
 * `times` has one row of n_t fp32 per step (n_t = 1: Euler-Maruyama; 2: Heun's two evaluations) and the last step's time in its last row; a call
 * past the table keeps writing the last row (the clamp).  Plain vector stores; nothing past t_out[n_t * batch - 1] is written.
 * Checked in this order: NULL block ZIGMA_ERR_NULL; n_t other than 1 / 2, batch < 1, n_rows < 1 ZIGMA_ERR_SHAPE; flags != 0
 * ZIGMA_ERR_UNSUPPORTED; NULL state, times or t_out ZIGMA_ERR_NULL; state not 16-byte aligned ZIGMA_ERR_STRIDE.
 * ------------------------------------------------------------------------------------------ */
#define ZIGMA_SDE_ROW_ABSOLUTE 1   /* zigma_sde_step_params_t.flags: the coefficient row is `row`, not state->step * rows_per_step + row */

typedef struct zigma_sde_state {
    uint32_t seed_lo, seed_hi;   /* the Philox key                      */
    uint32_t stream;             /* counter word 3                      */
    uint32_t step;               /* counter word 2; zigma_sde_advance increments it */
} zigma_sde_state_t;

typedef struct zigma_sde_step_params {
    int64_t n;
    int64_t elem_offset;
    int64_t coef_rows;
    int32_t dtype;               /* zigma_dtype_t of a, b, c and out */
    int32_t flags;               /* ZIGMA_SDE_ROW_ABSOLUTE */
    int32_t rows_per_step, row;
    const void *a, *b, *c;
    void *out;
    const float *coef;
    const zigma_sde_state_t *state;
    uint32_t *bits_out;
} zigma_sde_step_params_t;

typedef struct zigma_sde_advance_params {
    zigma_sde_state_t *state;
    const float *times;
    float *t_out;
    int64_t n_rows;
    int32_t n_t, batch;
    int32_t flags;               /* reserved, must be 0 */
    int32_t pad_;
} zigma_sde_advance_params_t;

int zigma_sde_step_fwd(const zigma_sde_step_params_t *p, void *stream);
int zigma_sde_advance(const zigma_sde_advance_params_t *p, void *stream);

/* ------------------------------------------------------------------------------------------
 * Host-only plan queries of the Mamba inner's five forward entry points (ABI 11): what the launch would do with this parameter block,
 * asked before anything is allocated or launched.  Each runs the same plan_*() (csrc/scan_plan.h, csrc/front_plan.h) as its launcher.
 *
 *   returns   the status the launch would return for this block (never ZIGMA_ERR_LAUNCH);
 *   *kernel   the name zigma_last_kernel() would report after the launch, or NULL where nothing would launch (a refusal, an empty call).
 *             For a call the launcher runs in batch slices: the first refusing slice's status, else the last slice's kernel.
 *
 * A query makes no HIP call, reads the block's sizes, strides, flags and pointer VALUES only (no operand is dereferenced, so the
 * addresses of tensors yet to be allocated may be placeholders with the alignment the allocator guarantees), writes neither p->info nor
 * the last-kernel record, and may be called with no device present and during stream capture.
 */
int zigma_selective_scan_fwd_plan(const zigma_scan_params_t *p, const char **kernel);
int zigma_causal_conv1d_fwd_plan(const zigma_conv_params_t *p, const char **kernel);
int zigma_conv_x_proj_fwd_plan(const zigma_conv_xproj_params_t *p, const char **kernel);
int zigma_x_proj_fwd_plan(const zigma_xproj_params_t *p, const char **kernel);
int zigma_dt_proj_softplus_fwd_plan(const zigma_dtproj_params_t *p, const char **kernel);
/* ... and of the dense projections (ABI 11, no block changed): plan_linear() / plan_linear_split() of csrc/linear_plan.h, plan_norm_linear() of
 * csrc/norm_linear_plan.h, under the same rules. */
int zigma_linear_fwd_plan(const zigma_linear_params_t *p, const char **kernel);
int zigma_norm_linear_fwd_plan(const zigma_norm_linear_params_t *p, const char **kernel);
int zigma_linear_f32_split_plan(const zigma_linear_split_params_t *p, const char **kernel);
/* ... and of the operators around the blocks (csrc/outer_plan.h), cross-attention and the glue backward (csrc/attn_plan.h) and the weight
 * gradient (csrc/wgrad_plan.h) (ABI 11, no block changed), under the same rules: every refusal of these entry points is a clause of its plan_*(). */
int zigma_patch_embed_fwd_plan(const zigma_patch_embed_params_t *p, const char **kernel);
int zigma_timestep_embed_fwd_plan(const zigma_timestep_embed_params_t *p, const char **kernel);
int zigma_skinny_linear_fwd_plan(const zigma_skinny_params_t *p, const char **kernel);
int zigma_final_layer_fwd_plan(const zigma_final_layer_params_t *p, const char **kernel);
int zigma_final_layer_cfg_fwd_plan(const zigma_final_layer_cfg_params_t *p, const char **kernel);
int zigma_cross_attn_fwd_plan(const zigma_xattn_params_t *p, const char **kernel);
int zigma_cross_attn_bwd_plan(const zigma_xattn_bwd_params_t *p, const char **kernel);
int zigma_scale_reduce_bwd_plan(const zigma_glue_bwd_params_t *p, const char **kernel);
int zigma_linear_wgrad_plan(const zigma_linear_wgrad_params_t *p, const char **kernel);
/* ... and of add-norm in both directions (csrc/norm_plan.h) and the scan and conv backward (csrc/bwd_plan.h) (ABI 11, no block changed), under the same
 * rules: with these every compute entry point the model's forward or backward calls answers a query.  The three *_workspace_bytes() are the `need` of
 * the same plans. */
int zigma_add_norm_fwd_plan(const zigma_norm_params_t *p, const char **kernel);
int zigma_add_norm_bwd_plan(const zigma_norm_bwd_params_t *p, const char **kernel);
int zigma_selective_scan_bwd_plan(const zigma_scan_bwd_params_t *p, const char **kernel);
int zigma_causal_conv1d_bwd_plan(const zigma_conv_bwd_params_t *p, const char **kernel);

/* ------------------------------------------------------------------------------------------ */
const char *zigma_strerror(int status);
int zigma_abi_version(void);
/* Name of the kernel variant the last dispatch on this thread selected (for tests / profiling). */
const char *zigma_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* ZIGMA_HIP_H_ */
