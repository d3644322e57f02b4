"""Selective-scan op layer on the HIP kernels.

Mirrors the reference's `dis_mamba/mamba_ssm/ops/selective_scan_interface.py` (same names, argument
order and error behaviour) for the FORWARD path:

    selective_scan_cuda_fwd   <-> selective_scan_cuda.fwd            (selective_scan.cpp:226-336)
    selective_scan_fn         <-> selective_scan_fn                  (selective_scan_interface.py:77-83)
    mamba_inner_fn            <-> mamba_inner_fn / MambaInnerFn.forward        (:296-365, :606-614)
    mamba_inner_fn_no_out_proj<-> MambaInnerFnNoOutProj.forward                (:155-224)

plus `mamba_inner_tok`, the token-major fused form the ZigMa block uses on MI355X: conv, scan and
the zigzag gather/scatter run on (B, L, C) activations straight out of / into the projection GEMMs,
so none of the reference's transposes, `index_select`s or `cat`s exist.  `plan_inner` is the one place that chooses its kernels (conv +
x_proj front, where dt_proj runs, the sequence split, the accumulating epilogue); `mamba_inner_tok` and `MambaInnerTokFn` carry the plan out.
What a kernel takes is the library's to say: every binding here is a builder of its parameter block and a launch, and the eligibility predicates
hand the block the launch would get to the library's host-only plan queries (`_lib.plan`: plan_scan() of csrc/scan_plan.h, the plans of
csrc/front_plan.h).  Only what a block cannot say, and policy (where a kernel that would serve is not the one to take), is decided in Python.

Backward: `scan_bwd_tok` binds zigma_selective_scan_bwd; `MambaInnerTokFn` is the autograd
form of `mamba_inner_tok` (MambaInnerFn.backward, :367-434) that the blocks use when autograd is recording.  The
(B, D, L)-layout entry points (`selective_scan_fn`, `mamba_inner_fn`) stay forward-only.
"""

from collections import namedtuple

import math

import torch
import torch.nn.functional as F

from . import _knobs, _lib, amp
from .causal_conv1d_interface import causal_conv1d_raw, conv_bwd_tok
from .wgrad import plan_wgrad, wgrad


SPLIT_SMALL_BATCH = True             # tools/latency_probe.py flips this to measure the effect of the small-batch sequence split
SPLIT_MAX_WGS = 200                  # ... and sweeps this: split when batch * d_inner / 64 is at most this many workgroups (tools/split_threshold_probe.py)
USE_CONV_X_PROJ = True               # conv + SiLU + x_proj in one kernel (u written once, never read back); False: the two kernels
CONV_X_PROJ_MIN_POSITIONS = 16384    # below: too few workgroups (128 positions each)
USE_X_PROJ_KERNEL = True             # own MFMA kernel for the skinny x_proj instead of the library GEMM (same speed stand-alone)
DT_PROJ_FLAGS = 0                    # 1: four-byte stores (A/B probe of dt_proj.hip)
DT_PROJ_IN_SCAN = True               # dt_proj + softplus in the scan's tile prologue (MFMA) instead of a kernel of its own
DT_PROJ_IN_SPLIT = True              # sequence-split mode: dt_proj + softplus inside the split's first pass, which writes delta for the second (round 6)
ACCUMULATE_IN_SCAN = True            # `v2`: the second sweep's add in its scan epilogue (False: the in-place add; A/B in tests / tools)
_knobs.apply(globals(), "selective_scan_interface")      # the knobs above: tools/ and tests/ set them directly, ZIGMA_KNOBS at import


def split_chunk_len(batch, d_inner, seqlen, reset_period=0):
    """Chunk length (a multiple of 16) for the sequence-split mode of the token-major scan, or 0 for a single pass.
    The plain grid is batch * d_inner / 64 workgroups; the split pays (it runs the recurrence twice) only when that
    leaves most of the 256 CUs idle: small batches at L >= 256 (threshold from tools/split_threshold_probe.py), or
    long sequences (L >= 4096: chunks of at most the reference's 2048 steps, sized for ~5 workgroups per CU)."""
    wgs = batch * (d_inner // 64)
    if reset_period or wgs < 1:
        return 0
    if seqlen >= 4096:                                            # long sequences: ~1280 workgroups = 5 per CU, all resident
        if wgs >= 768:
            return 0
        per = -(-seqlen // -(-1280 // wgs))
        return min(2048, max(256, (per + 15) // 16 * 16))
    if not (SPLIT_SMALL_BATCH and wgs <= SPLIT_MAX_WGS and seqlen >= 256):
        return 0
    per = -(-seqlen // -(-768 // wgs))                            # steps per chunk that give ~768 workgroups
    chunk = min(2048, max(32, (per + 15) // 16 * 16))
    return chunk if -(-seqlen // chunk) >= 2 else 0


_Desc = _lib.Desc          # what the block builders read of a tensor, for the plan queries (of / fresh / scan_view / columns)


def _as_bgnl(M, name):
    """(B, N, L) -> (B, 1, N, L) like SelectiveScanFn.forward (:30-35)."""
    if M.dim() == 3:
        return M.unsqueeze(1)
    if M.dim() != 4:
        raise RuntimeError(f"{name} must be (D, N), (B, N, L) or (B, G, N, L)")
    return M


def _scan_flags(z_preactivated, accumulate, probe_flags=0):
    return (_lib.SCAN_Z_PREACTIVATED if z_preactivated else 0) | (_lib.SCAN_ACCUMULATE if accumulate else 0) | int(probe_flags)


def scan_block(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, *, out=None, out_z=None, x=None, z_row_index=None,
               out_row_index=None, checkpoints=None, reset_period=0, chunk_len=2048, z_preactivated=False, _probe_flags=0, dt_x=None, dt_w=None,
               accumulate=False):
    """The parameter block of zigma_selective_scan_fwd from the operands of scan_raw (checked here; outputs as scan_raw allocates them).  Reads
    shapes, strides, dtypes and addresses only, so a description of a tensor that is yet to be allocated (_Desc) serves as well as the tensor;
    B / C that vary with the input come as (batch, groups, dstate, seqlen) then."""
    if delta is None:
        if dt_x is None or dt_w is None or not delta_softplus:
            raise RuntimeError("delta=None needs dt_x, dt_w and delta_softplus=True")
    elif dt_x is not None or dt_w is not None:
        # (ABI 10) with the carry tensor x — the sequence split — delta is a WORKSPACE: the first pass forms softplus(dt_proj + bias) itself and
        # writes it there for the second pass; without x the two are alternatives
        if x is None or dt_x is None or dt_w is None or not delta_softplus:
            raise RuntimeError("pass either delta or (dt_x, dt_w); both only with x (sequence split: delta is the workspace the first pass fills)")
    shape = tuple(u.shape)
    if len(shape) != 3 or (delta is not None and tuple(delta.shape) != shape):
        raise RuntimeError("u and delta must both be (batch, dim, seqlen)")
    if A.dtype.is_complex:
        raise RuntimeError("zigma_amd: complex A is out of scope (ZigMa's A is real, mamba_simple.py:298)")
    if A.dtype != torch.float32:
        raise RuntimeError("A must be float32")
    if delta is not None and delta.dtype != u.dtype:
        raise RuntimeError("delta must have the dtype of u")
    batch, dim, L = shape
    N = A.shape[1]
    if A.shape[0] != dim:
        raise RuntimeError("A must be (dim, dstate)")
    if N > 256:
        raise RuntimeError("selective_scan only supports state dimension <= 256")
    if accumulate and (dt_x is None or out_z is None):
        raise RuntimeError("accumulate=True is served by the in-kernel dt_proj form only (dt_x / dt_w) and needs the out_z to add to")
    var_b, var_c = B.dim() >= 3, C.dim() >= 3
    P = _lib.ScanParams()
    P.batch, P.dim, P.seqlen, P.dstate = batch, dim, L, N
    P.delta_softplus, P.io_dtype = int(bool(delta_softplus)), _lib.dtype_id(u)
    P.chunk_len, P.flags = int(chunk_len), _scan_flags(z_preactivated, accumulate, _probe_flags)
    P.is_variable_B, P.is_variable_C = int(var_b), int(var_c)
    P.reset_period = int(reset_period)       # > 0: independent sequences of that many steps along seqlen
    groups, bc = {}, None
    for name, M, var in (("B", B, var_b), ("C", C, var_c)):
        if var:
            if M.dim() != 4:
                raise RuntimeError(f"{name} must be (D, N), (B, N, L) or (B, G, N, L)")
            if M.shape[0] != batch or M.shape[2] != N or M.shape[3] != L:
                raise RuntimeError(f"{name} must be (batch, groups, dstate, seqlen)")
            groups[name] = M.shape[1]
            if bc is not None and M.dtype != bc.dtype:
                raise RuntimeError("variable B and C must share a dtype")
            bc = M
        elif tuple(M.shape) != (dim, N) or M.dtype != torch.float32:
            raise RuntimeError(f"constant {name} must be float32 (dim, dstate)")
    if var_b:
        P.B_batch_stride, P.B_group_stride, P.B_dstate_stride, P.B_l_stride = B.stride(0), B.stride(1), B.stride(2), B.stride(3)
    else:
        P.B_d_stride, P.B_dstate_stride = B.stride(0), B.stride(1)
    if var_c:
        P.C_batch_stride, P.C_group_stride, P.C_dstate_stride, P.C_l_stride = C.stride(0), C.stride(1), C.stride(2), C.stride(3)
    else:
        P.C_d_stride, P.C_dstate_stride = C.stride(0), C.stride(1)
    if var_b and var_c and groups["B"] != groups["C"]:
        raise RuntimeError("B and C must have the same number of groups")
    P.n_groups = groups.get("C", groups.get("B", 1))
    if dim % P.n_groups != 0:
        raise RuntimeError("dim must be divisible by the number of B/C groups")
    P.bc_dtype = _lib.dtype_id(u if bc is None else bc)
    for name, t in (("z", z), ("out", out), ("out_z", out_z)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != u.dtype):
            raise RuntimeError(f"{name} must match u in shape and dtype")
    P.u_batch_stride, P.u_d_stride, P.u_l_stride = u.stride(0), u.stride(1), u.stride(2)
    if delta is not None:
        P.delta_batch_stride, P.delta_d_stride, P.delta_l_stride = delta.stride(0), delta.stride(1), delta.stride(2)
    if z is not None:
        P.z_batch_stride, P.z_d_stride, P.z_l_stride = z.stride(0), z.stride(1), z.stride(2)
    if out is not None:
        P.out_batch_stride, P.out_d_stride, P.out_l_stride = out.stride(0), out.stride(1), out.stride(2)
    if out_z is not None:
        P.out_z_batch_stride, P.out_z_d_stride, P.out_z_l_stride = out_z.stride(0), out_z.stride(1), out_z.stride(2)
    if x is not None:
        n_chunks = (L + int(chunk_len) - 1) // int(chunk_len)
        if tuple(x.shape) != (batch, dim, n_chunks, 2 * N) or x.dtype != torch.float32 or not x.is_contiguous():
            raise RuntimeError("x must be contiguous float32 (batch, dim, n_chunks, 2*dstate)")
    if dt_x is not None:
        if (dt_x.dim() != 3 or dt_x.shape[0] != batch or dt_x.shape[1] != L or dt_x.dtype != u.dtype or dt_x.stride(2) != 1
                or dt_w.dim() != 2 or dt_w.shape[0] != dim or dt_w.dtype != u.dtype or dt_w.stride(1) != 1 or dt_x.shape[2] < dt_w.shape[1]):
            raise RuntimeError("dt_x must be (batch, seqlen, >= dt_rank) rows and dt_w (dim, dt_rank), both in the dtype of u")
        P.dt_rank, P.dt_x_batch_stride, P.dt_x_l_stride, P.dt_w_row_stride = dt_w.shape[1], dt_x.stride(0), dt_x.stride(1), dt_w.stride(0)
    return _scan_addresses(P, u, delta, A, B, C, D, z, delta_bias, out, out_z, x, z_row_index, out_row_index, checkpoints, dt_x, dt_w)


def _scan_addresses(P, u, delta, A, B, C, D, z, delta_bias, out, out_z, x, z_row_index, out_row_index, checkpoints, dt_x, dt_w):
    """every address of a scan block (scan_block ends with it)"""
    P.u, P.delta, P.z, P.out, P.out_z = _lib.ptr(u), _lib.ptr(delta), _lib.ptr(z), _lib.ptr(out), _lib.ptr(out_z)
    P.B, P.C, P.x, P.dt_x, P.dt_w = _lib.ptr(B), _lib.ptr(C), _lib.ptr(x), _lib.ptr(dt_x), _lib.ptr(dt_w)
    return _scan_side_operands(P, A, D, delta_bias, z_row_index, out_row_index, checkpoints)


def _scan_side_operands(P, A, D, delta_bias, z_row_index, out_row_index, checkpoints=None):
    """the operands a scan block holds little but the address of, checked and set: A with its two strides, D, delta_bias, the row tables, the
    checkpoints.  (The dt decision builds its block without them: scan_planned sets them.)"""
    for v, name in ((D, "D"), (delta_bias, "delta_bias")):
        if v is not None and (v.dtype != torch.float32 or tuple(v.shape) != (P.dim,) or v.stride(0) != 1):
            raise RuntimeError(f"{name} must be contiguous float32 (dim,)")
    for idx, name in ((z_row_index, "z_row_index"), (out_row_index, "out_row_index")):
        if idx is not None and (idx.dtype != torch.int32 or tuple(idx.shape) != (P.seqlen,) or not idx.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous int32 tensor of length seqlen")
    if checkpoints is not None and (checkpoints.dtype != torch.float32 or not checkpoints.is_contiguous()):
        raise RuntimeError("checkpoints must be a contiguous float32 buffer")
    P.A, P.A_d_stride, P.A_dstate_stride = _lib.ptr(A), A.stride(0), A.stride(1)
    P.D, P.delta_bias, P.z_row_index, P.out_row_index = _lib.ptr(D), _lib.ptr(delta_bias), _lib.ptr(z_row_index), _lib.ptr(out_row_index)
    P.checkpoints = _lib.ptr(checkpoints)
    return P


def scan_planned(P, u, x_dbl, delta, xc, y, z, A, D, delta_bias, z_row_index, out_row_index, z_preactivated, accumulate):
    """Launch the scan block plan_inner's dt decision built and the library accepted (dt_in_scan_eligible(keep=)): the block of the in-kernel
    dt_proj call on u, x_dbl (dt_x; B and C its columns behind dt_rank), the gate z and the result y (all (B, L, .) rows), with delta and xc the
    split's workspace and carries or None.  Layout, sizes, reset_period and chunk_len stand as planned; the addresses — placeholders where the
    tensor was yet to be allocated —, the side operands and the flags are set here.  The caller passes tensors of the planned layout: fresh
    contiguous u, x_dbl, delta, xc; z and y as the decision saw them (y: fresh rows where it saw none)."""
    dev = _lib.require_device(u, x_dbl, delta, xc, y, z, A, D, delta_bias, z_row_index, out_row_index)
    es, rows = u.element_size(), x_dbl.data_ptr()
    P.u, P.delta, P.z, P.out_z, P.x = u.data_ptr(), _lib.ptr(delta), z.data_ptr(), y.data_ptr(), _lib.ptr(xc)
    P.dt_x, P.B, P.C = rows, rows + P.dt_rank * es, rows + (P.dt_rank + P.dstate) * es
    P.flags = _scan_flags(z_preactivated, accumulate)
    _lib.call("zigma_selective_scan_fwd", _scan_side_operands(P, A, D, delta_bias, z_row_index, out_row_index), dev)


def scan_raw(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, *, out=None, out_z=None,
             x=None, z_row_index=None, out_row_index=None, want_out=True, checkpoints=None, reset_period=0,
             chunk_len=2048, z_preactivated=False, info=None, _probe_flags=0, dt_x=None, dt_w=None, accumulate=False):
    """Launch zigma_selective_scan_fwd.  All tensors are logical (batch, dim, seqlen) VIEWS with arbitrary
    strides (token-major tensors come in as `.transpose(1, 2)`); B/C are (D, N) f32 or (B, G, N, L) views.
    Outputs that are None are allocated here with the reference's conventions (out like delta, out_z like z).
    z_preactivated: z already holds silu(z) (ZIGMA_SCAN_Z_PREACTIVATED; hot token-major kernel only).
    info: optional list; receives [kernel family (_lib.SCAN_KERNEL_*), 1 if `checkpoints` is being written].
    dt_x, dt_w (ABI 9, with delta=None): dt_proj + bias + softplus inside the token-major hot kernel — dt_x (batch, seqlen, >= dt_rank)
    bf16 rows in SCAN order (x_dbl as x_proj wrote it), dt_w (dim, dt_rank); delta' = softplus(dt_x[..., :dt_rank] @ dt_w.T + delta_bias).
    dt_x, dt_w AND delta AND x (ABI 10): the sequence split with dt_proj inside its first pass — delta (uninitialised, shape of u) receives the step sizes.
    accumulate (with dt_x / dt_w only): out_z += y * silu(z) — the second sweep of `v2` adds itself to the first one's result (ZIGMA_SCAN_ACCUMULATE)."""
    dev = _lib.require_device(u, delta, A, B, C, D, z, delta_bias, out, out_z, x, z_row_index, out_row_index, dt_x, dt_w)
    B, C = (_as_bgnl(M, name) if M.dim() >= 3 else M for M, name in ((B, "B"), (C, "C")))
    D, delta_bias = (v.contiguous() if v is not None and v.dim() == 1 and v.stride(0) != 1 else v for v in (D, delta_bias))
    if z is not None and out_z is None:
        out_z = torch.empty_like(z)
    if out is None and (want_out or z is None):
        out = torch.empty_like(delta if delta is not None else u)
    P = scan_block(u, delta, A, B, C, D, z, delta_bias, delta_softplus, out=out, out_z=out_z, x=x, z_row_index=z_row_index,
                   out_row_index=out_row_index, checkpoints=checkpoints, reset_period=reset_period, chunk_len=chunk_len,
                   z_preactivated=z_preactivated, _probe_flags=_probe_flags, dt_x=dt_x, dt_w=dt_w, accumulate=accumulate)
    status = (_lib.C.c_int32 * 2)(0, 0)
    P.info = status                          # host out-field: which kernel family ran, whether it writes the checkpoints
    _lib.call("zigma_selective_scan_fwd", P, dev)
    if info is not None:
        info[:] = [int(status[0]), int(status[1])]
    return out, out_z


def _served(fn_name, block, *kernels):
    """the library's plan serves this block with one of these kernels (a name ending in * stands for every kernel that begins so)"""
    status, kernel = _lib.plan(fn_name, block)
    return status == 0 and kernel is not None and any(kernel.startswith(k[:-1]) if k.endswith("*") else kernel == k for k in kernels)


def x_proj_block(u, weight, out):
    """the parameter block of zigma_x_proj_fwd: u (..., k) rows one pitch apart, weight (n, k), out (..., n)"""
    P = _lib.XProjParams()
    P.m, P.n, P.k, P.dtype, P.flags = math.prod(u.shape[:-1]), weight.shape[0], u.shape[-1], _lib.dtype_id(u), 0
    P.x_row_stride, P.w_row_stride, P.out_row_stride = u.stride(-2), weight.stride(0), out.stride(-2)
    P.x, P.w, P.out = _lib.ptr(u), _lib.ptr(weight), _lib.ptr(out)
    return P


def x_proj_eligible(u, weight):
    """zigma_x_proj_fwd takes u @ weight.T: what plan_x_proj() (csrc/front_plan.h) serves, asked through the library, and on top of it
    - the device, one dtype for both operands and contiguous weight columns (the block has one dtype and row pitches only);
    - policy: contiguous u (the plan takes any row pitch it can load);
    - policy: from 16 384 tokens on, where a workgroup streams 256 token rows over the whole K; below, from 256 tokens on (fewer stay with the
      library GEMM) and only where the plan takes the split-K form (x_proj_splitk_kernel, round 5: the streaming form was 32 workgroups and
      31 us at 8192 tokens against 21 for the library)."""
    tokens = math.prod(u.shape[:-1])
    if not (u.is_cuda and weight.dtype == u.dtype and weight.stride(1) == 1 and u.is_contiguous() and tokens >= 256):
        return False
    out = _Desc.fresh(u, (tokens, weight.shape[0]), 1)
    return _served("zigma_x_proj_fwd", x_proj_block(u, weight, out), "x_proj_mfma" if tokens >= 16384 else "x_proj_splitk")


def x_proj(u, weight):
    """x_dbl = u @ weight.T on the matrix cores with a kernel shaped for the skinny output (zigma_x_proj_fwd)."""
    dev = _lib.require_device(u, weight)
    lead, K = u.shape[:-1], u.shape[-1]
    u2 = u.reshape(-1, K)
    n = weight.shape[0]
    out = torch.empty(u2.shape[0], n, device=u.device, dtype=u.dtype)
    _lib.call("zigma_x_proj_fwd", x_proj_block(u2, weight, out), dev)
    return out.reshape(*lead, n)


def conv_x_proj_block(x_half, conv_w, conv_b, x_proj_weight, perm, u, x_dbl, _flags=0):
    """the parameter block of zigma_conv_x_proj_fwd: x_half (B, L, d_inner) rows, contiguous (d_inner, 4) taps and bias, x_proj_weight (n, d_inner),
    a contiguous int32 row table or None; u (B, L, d_inner) and x_dbl (B, L, n) receive the results"""
    P = _lib.ConvXProjParams()
    P.batch, P.seqlen, P.dim = x_half.shape
    P.n, P.dtype, P.flags = x_proj_weight.shape[0], _lib.dtype_id(x_half), _flags
    P.x_batch_stride, P.x_l_stride = x_half.stride(0), x_half.stride(1)
    P.u_batch_stride, P.u_l_stride = u.stride(0), u.stride(1)
    P.w_row_stride, P.out_row_stride = x_proj_weight.stride(0), x_dbl.stride(1)
    P.x, P.conv_weight, P.conv_bias, P.w = _lib.ptr(x_half), _lib.ptr(conv_w), _lib.ptr(conv_b), _lib.ptr(x_proj_weight)
    P.u, P.out, P.x_row_index = _lib.ptr(u), _lib.ptr(x_dbl), _lib.ptr(perm)
    return P


def conv_x_proj_eligible(x_half, conv_w, conv_b, x_proj_weight, perm, reset_period=0):
    """zigma_conv_x_proj_fwd takes the front in one kernel: what plan_conv_x_proj() (csrc/front_plan.h) serves, asked through the library, and on
    top of it
    - the device, a bias, one sequence per batch row (the entry point has neither a bias-free form nor a reset_period);
    - what the block cannot say: one dtype for all four operands, width-4 taps, taps / bias / row table contiguous (it carries no pitch for them),
      contiguous channels and weight columns, an int32 row table;
    - policy: at least CONV_X_PROJ_MIN_POSITIONS positions."""
    if conv_b is None or reset_period or not x_half.is_cuda:
        return False
    Bsz, L, Di = x_half.shape
    if not (conv_w.dtype == x_half.dtype and conv_b.dtype == x_half.dtype and x_proj_weight.dtype == x_half.dtype
            and tuple(conv_w.shape) == (Di, 4) and conv_w.is_contiguous() and conv_b.is_contiguous()
            and x_half.stride(2) == 1 and x_proj_weight.stride(1) == 1
            and (perm is None or (perm.dtype == torch.int32 and perm.is_contiguous()))
            and Bsz * L >= CONV_X_PROJ_MIN_POSITIONS):                              # policy: fewer than ~64 workgroups of 256 positions leave the chip idle
        return False
    u, x_dbl = _Desc.fresh(x_half, (Bsz, L, Di), 1), _Desc.fresh(x_half, (Bsz, L, x_proj_weight.shape[0]), 2)
    return _served("zigma_conv_x_proj_fwd", conv_x_proj_block(x_half, conv_w, conv_b, x_proj_weight, perm, u, x_dbl), "conv_x_proj_mfma")


def conv_x_proj(x_half, conv_w, conv_b, x_proj_weight, perm=None, _flags=0):
    """u = silu(causal_conv1d(x_half[:, perm])) and x_dbl = u @ x_proj_weight.T in one pass over x (zigma_conv_x_proj_fwd).
    x_half: (B, L, d_inner) bf16 / fp16 view with contiguous channels (the first half of the in_proj output, as is); conv_w: (d_inner, 4);
    returns u (B, L, d_inner) in SCAN order and x_dbl (B, L, n).  Replaces causal_conv1d_fn + F.linear of reference
    selective_scan_interface.py:307-322."""
    dev = _lib.require_device(x_half, conv_w, conv_b, x_proj_weight, perm)
    Bsz, L, Di = x_half.shape
    u = torch.empty(Bsz, L, Di, device=x_half.device, dtype=x_half.dtype)
    x_dbl = torch.empty(Bsz, L, x_proj_weight.shape[0], device=x_half.device, dtype=x_half.dtype)
    _lib.call("zigma_conv_x_proj_fwd", conv_x_proj_block(x_half, conv_w, conv_b, x_proj_weight, perm, u, x_dbl, _flags), dev)
    return u, x_dbl


def dt_in_scan_eligible(u, x_dbl, weight, reset_period=0, out=None, dstate=16, z=None, *, chunk_len=0, keep=None):
    """scan_tok2_kernel takes dt_proj + softplus into the scan (zigma_scan_params_t.dt_x): what plan_scan() (csrc/scan_plan.h) serves with a
    scan_tok2_n16_dtproj* kernel — chunk_len > 0: with scan_tok2_n16_split_dtproj, the sequence split of that chunk length, whose first pass
    writes delta — asked through the library on the block mamba_inner_tok launches: u (B, L, d_inner) and x_dbl (B, L, >= dt_rank + 2 * dstate)
    rows, B / C columns of x_dbl, the gate z and the result `out` as given or fresh rows like u.  A caller that gets False keeps the dt_proj
    kernel (or F.linear) + the ordinary scan call, which serves every shape the reference does.  On top of the plan: the device, one dtype for
    u, x_dbl and weight, contiguous weight columns and x_dbl rows (the block has one dtype and pitches only), and x_dbl wide enough to hold B and C.
    keep: a dict that receives the served block as keep["scan"], for scan_planned to launch."""
    R = weight.shape[1]
    if not (u.is_cuda and x_dbl.dtype == u.dtype and weight.dtype == u.dtype and u.dim() == 3 and x_dbl.dim() == 3
            and x_dbl.shape[2] >= R + 2 * dstate and x_dbl.stride(2) == 1 and weight.stride(1) == 1):
        return False
    Bsz, L, Di = u.shape
    u, x_dbl = _Desc.of(u), _Desc.of(x_dbl)
    z, y = (_Desc.fresh(u, u.shape, k) if t is None else _Desc.of(t) for t, k in ((z, 1), (out, 2)))             # (None: rows like u)
    A = _Desc.fresh(u, (Di, dstate), 3, torch.float32)
    delta = xc = None
    if chunk_len:                                                   # the split: delta is the workspace its first pass fills, xc its carries
        delta, xc = _Desc.fresh(u, u.shape, 4), _Desc.fresh(u, (Bsz, Di, -(-L // chunk_len), 2 * dstate), 5, torch.float32)
    P = scan_block(u.scan_view(), None if delta is None else delta.scan_view(), A, x_dbl.columns(R, dstate), x_dbl.columns(R + dstate, dstate), None,
                   z.scan_view(), None, True, out_z=y.scan_view(), x=xc, reset_period=reset_period, chunk_len=chunk_len or 2048, dt_x=x_dbl, dt_w=weight)
    served = _served("zigma_selective_scan_fwd", P, "scan_tok2_n16_split_dtproj" if chunk_len else "scan_tok2_n16_dtproj*")
    if served and keep is not None:
        keep["scan"] = P
    return served


def dt_proj_block(x_dbl, dt_rank, weight, bias, softplus, out):
    """the parameter block of zigma_dt_proj_softplus_fwd: x_dbl (..., >= dt_rank) rows one pitch apart, weight (d_inner, dt_rank), float32 bias or
    None, out (..., d_inner)"""
    P = _lib.DtProjParams()
    P.m, P.n, P.k = math.prod(x_dbl.shape[:-1]), weight.shape[0], dt_rank
    P.dtype, P.softplus, P.flags = _lib.dtype_id(x_dbl), int(bool(softplus)), DT_PROJ_FLAGS
    P.x_row_stride, P.w_row_stride, P.out_row_stride = x_dbl.stride(-2), weight.stride(0), out.stride(-2)
    P.x, P.w, P.out = _lib.ptr(x_dbl), _lib.ptr(weight), _lib.ptr(out)
    if bias is not None:
        if bias.dtype != torch.float32 or tuple(bias.shape) != (weight.shape[0],) or bias.stride(0) != 1:
            raise RuntimeError("bias must be contiguous float32 (d_inner,)")
        P.bias = _lib.ptr(bias)
    return P


def dt_proj_eligible(x_dbl, dt_rank, weight):
    """zigma_dt_proj_softplus_fwd takes dt_proj: what plan_dt_proj() (csrc/front_plan.h) serves, asked through the library; on top of it only the
    device, one dtype for both operands and contiguous x_dbl rows / weight columns (the block has one dtype and row pitches only).  No policy."""
    if not (x_dbl.is_cuda and weight.dtype == x_dbl.dtype and x_dbl.stride(-1) == 1 and weight.stride(1) == 1):
        return False
    out = _Desc.fresh(x_dbl, (math.prod(x_dbl.shape[:-1]), weight.shape[0]), 1)
    return _served("zigma_dt_proj_softplus_fwd", dt_proj_block(x_dbl, dt_rank, weight, None, True, out), "dt_proj_softplus_mfma")


def dt_proj_softplus(x_dbl, dt_rank, weight, bias=None, softplus=True):
    """delta' = softplus(x_dbl[..., :dt_rank] @ weight.T + bias) on the matrix cores (zigma_dt_proj_softplus_fwd).
    x_dbl: (..., >= dt_rank) bf16 / fp16 rows; weight: (d_inner, dt_rank) in the same dtype; bias: float32 (d_inner) or None.
    Returns (..., d_inner) in that dtype.  Fuses reference selective_scan_interface.py:323 with the softplus(delta + bias)
    at the top of its scan kernel; the scan is then called with delta_softplus=False, delta_bias=None."""
    dev = _lib.require_device(x_dbl, weight, bias)
    lead = x_dbl.shape[:-1]
    x2 = x_dbl.reshape(-1, x_dbl.shape[-1])
    if x2.stride(-1) != 1:
        raise RuntimeError("x_dbl rows must be contiguous")
    n = weight.shape[0]
    out = torch.empty(x2.shape[0], n, device=x_dbl.device, dtype=x_dbl.dtype)
    _lib.call("zigma_dt_proj_softplus_fwd", dt_proj_block(x2, dt_rank, weight, bias, softplus, out), dev)
    return out.reshape(*lead, n)


def scan_bwd_block(u, delta, A, B, C, D, z, delta_bias, dout, out, delta_softplus, du, ddelta, dA, dB, dC, dD, dz, dbias, *, z_row_index=None,
                   out_row_index=None, checkpoints=None, reset_period=0):
    """The parameter block of zigma_selective_scan_bwd but for its workspace, from the operands and the outputs of scan_bwd_tok (checked here).  Reads
    shapes, strides, dtypes and addresses only, so a description of a tensor that is yet to be allocated serves as well as the tensor."""
    Bsz, L, Dm = u.shape
    N = A.shape[1]
    for t, nm in ((u, "u"), (delta, "delta"), (z, "z"), (out, "out"), (dout, "dout")):
        if t is not None and (tuple(t.shape) != (Bsz, L, Dm) or t.stride(2) != 1 or t.dtype != u.dtype):
            raise RuntimeError(f"{nm} must be (batch, seqlen, dim) with channel stride 1 and the dtype of u")
    if tuple(B.shape) != (Bsz, L, N) or tuple(C.shape) != (Bsz, L, N) or B.dtype != u.dtype or C.dtype != u.dtype:
        raise RuntimeError("B, C must be (batch, seqlen, dstate) views in the dtype of u")
    if A.dtype != torch.float32:
        raise RuntimeError("A must be float32")
    if z is not None and out is None:
        raise RuntimeError("the gated backward needs the forward's ungated `out`")
    if dz is not None and (tuple(dz.shape) != tuple(u.shape) or dz.stride(2) != 1 or dz.dtype != u.dtype):
        raise RuntimeError("dz must be (batch, seqlen, dim) with channel stride 1 and the dtype of u")
    P = _lib.ScanBwdParams()
    P.batch, P.dim, P.seqlen, P.dstate = Bsz, Dm, L, N
    P.delta_softplus, P.io_dtype, P.flags = int(bool(delta_softplus)), _lib.dtype_id(u), 0
    P.reset_period = int(reset_period)       # > 0: independent sequences of that many steps along seqlen (as in the forward)
    for name, t in (("u", u), ("delta", delta), ("z", z), ("out", out), ("dout", dout), ("du", du), ("ddelta", ddelta),
                    ("dz", dz)):
        if t is not None:
            setattr(P, name, _lib.ptr(t))
            setattr(P, name + "_batch_stride", t.stride(0))
            setattr(P, name + "_l_stride", t.stride(1))
    P.A, P.A_d_stride, P.A_dstate_stride = _lib.ptr(A), A.stride(0), A.stride(1)
    for name, t in (("B", B), ("C", C), ("dB", dB), ("dC", dC)):
        setattr(P, name, _lib.ptr(t))
        setattr(P, name + "_batch_stride", t.stride(0))
        setattr(P, name + "_l_stride", t.stride(1))
        setattr(P, name + "_dstate_stride", t.stride(2))
    for t, nm in ((D, "D"), (delta_bias, "delta_bias")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"{nm} must be contiguous float32")
    P.D, P.delta_bias, P.dA, P.dD, P.ddelta_bias = _lib.ptr(D), _lib.ptr(delta_bias), _lib.ptr(dA), _lib.ptr(dD), _lib.ptr(dbias)
    for name, tab in (("z_row_index", z_row_index), ("out_row_index", out_row_index)):
        if tab is not None:
            if tab.dtype != torch.int32 or tuple(tab.shape) != (L,) or not tab.is_contiguous():
                raise RuntimeError(f"{name} must be a contiguous int32 (seqlen,) table")
            setattr(P, name, _lib.ptr(tab))
    if checkpoints is not None:            # written by the forward kernel (scan_raw(..., checkpoints=)): skip phase 1
        shape = _lib.checkpoint_shape(Bsz, Dm, L, N)           # (None: the library refuses the shape itself)
        if checkpoints.dtype != torch.float32 or not checkpoints.is_contiguous() or (shape and checkpoints.numel() != math.prod(shape)):
            raise RuntimeError("checkpoints: float32 [batch][dim/64][ceil(seqlen/16)][dstate][64]")
        P.checkpoints = _lib.ptr(checkpoints)
    return P


def scan_bwd_tok(u, delta, A, B, C, D, z, delta_bias, dout, out, delta_softplus, *, dB=None, dC=None, dz=None,
                 z_row_index=None, out_row_index=None, checkpoints=None, reset_period=0):
    """Backward of the token-major selective scan (zigma_selective_scan_bwd; reference selective_scan_cuda.bwd,
    selective_scan.cpp:338-492).

    u, delta, z, out, dout: (batch, seqlen, dim), channel stride 1; out = the forward's UNGATED y (only with z).
    B, C: (batch, seqlen, dstate)-shaped views (any strides), same dtype.  A (dim, dstate) f32, D / delta_bias f32.
    dB, dC: optional preallocated float32 (batch, seqlen, dstate) views to write into (e.g. columns of d(x_dbl)).
    dz: optional preallocated (batch, seqlen, dim) view (e.g. the z half of d(xz)).
    z_row_index / out_row_index: the forward's int32 row tables — z / dz live at row z_row_index[k], out / dout at row
    out_row_index[k] of their tensors (token order) while u, delta, B, C, du, ddelta, dB, dC are in scan order.
    Returns du, ddelta, dA, dB, dC, dD, dz, ddelta_bias (None where the input was None); du/ddelta/dz in the input dtype,
    the rest float32."""
    dev = _lib.require_device(u, delta, A, B, C, D, z, delta_bias, dout, out)
    Bsz, L, Dm = u.shape
    N = A.shape[1]
    du, ddelta = torch.empty_like(u, memory_format=torch.contiguous_format), torch.empty_like(u, memory_format=torch.contiguous_format)
    if z is not None and dz is None:
        dz = torch.empty_like(u, memory_format=torch.contiguous_format)
    f32 = dict(device=u.device, dtype=torch.float32)
    dB = torch.empty(Bsz, L, N, **f32) if dB is None else dB
    dC = torch.empty(Bsz, L, N, **f32) if dC is None else dC
    if Bsz > _lib.GRID_DIM_MAX:
        # larger batches (the differentiable video temporal path reshapes to batch * tokens-per-frame rows) go in slices
        sl = lambda t, a, b: None if t is None else t[a:b]

        def run(a, b):
            r = scan_bwd_tok(u[a:b], delta[a:b], A, B[a:b], C[a:b], D, sl(z, a, b), delta_bias, dout[a:b], sl(out, a, b), delta_softplus,
                             dB=dB[a:b], dC=dC[a:b], dz=sl(dz, a, b), z_row_index=z_row_index, out_row_index=out_row_index,
                             checkpoints=sl(checkpoints, a, b), reset_period=reset_period)
            du[a:b].copy_(r[0]); ddelta[a:b].copy_(r[1])
            return r[2], r[5], r[7]
        dA, dD, dbias = _lib.sum_over_batch_slices(Bsz, run)
        return du, ddelta, dA, dB, dC, dD, dz, dbias
    dA = torch.zeros(Dm, N, **f32)
    dD = torch.zeros(Dm, **f32) if D is not None else None
    dbias = torch.zeros(Dm, **f32) if delta_bias is not None else None
    P = scan_bwd_block(u, delta, A, B, C, D, z, delta_bias, dout, out, delta_softplus, du, ddelta, dA, dB, dC, dD, dz, dbias,
                       z_row_index=z_row_index, out_row_index=out_row_index, checkpoints=checkpoints, reset_period=reset_period)
    ws = _lib.workspace("zigma_selective_scan_bwd", P, dev)
    _lib.call("zigma_selective_scan_bwd", P, dev)
    del ws
    return du, ddelta, dA, dB, dC, dD, dz, dbias


def differentiable(*tensors):
    """grad mode on and any of the tensors requires grad: the call must record autograd (MambaInnerTokFn)"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def z_preactivated_eligible(batch, seqlen, d_state):
    """scan-side limits of a gate in_proj pre-activated (ZIGMA_SCAN_Z_PREACTIVATED): the hot kernel's inference form, 16 states, whole tiles, one grid
    (plan_scan() of csrc/scan_plan.h: tok2_layout_ok() without `out`, no batch slices).  Stated here and not asked of the library: the choice is made
    before in_proj runs, when xz — and with it every operand of the scan's block — does not exist yet, and it only gates an in_proj epilogue
    (a scan the plan then does not serve pre-activated is refused by the library, never computed wrongly)."""
    return d_state == 16 and seqlen % 16 == 0 and batch <= _lib.GRID_DIM_MAX and not torch.is_grad_enabled()


InnerPlan = namedtuple("InnerPlan", "front dt chunk_len accumulate")


def plan_inner(x_half, z_half, conv_w, conv_b, x_proj_w, dt_proj_w, A, delta_bias, *, perm=None, reset_period=0, z_preactivated=False, out=None,
               add_to=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True, train=False, blocks=None):
    """The one place that chooses the kernels of the Mamba inner, from mamba_inner_tok's arguments (xz as its two halves, conv_w as
    (d_inner, width)); knobs and predicates are looked up as module globals at call time.  Returns InnerPlan:
    front       "conv_x_proj" (one kernel) | "conv+x_proj" (conv kernel, x_proj kernel) | "conv+linear" (conv kernel, library GEMM)
    dt          "in_scan" (dt_proj + softplus in the scan's tile prologue) | "in_split" (in the split's first pass, which writes delta)
                | "kernel" (zigma_dt_proj_softplus_fwd) | "linear" (library GEMM; the scan adds the bias and applies softplus)
    chunk_len   0: the scan takes the whole sequence; else the chunk length of the sequence split
    accumulate  add_to rides in the scan's epilogue (ZIGMA_SCAN_ACCUMULATE); else an in-place add behind the scan
    blocks: a dict that receives the parameter blocks the decision built and the library accepted ("scan": with dt "in_scan" / "in_split"), so that
    the launch completes them instead of building them again"""
    Bsz, L, Di = x_half.shape
    R, N = dt_proj_w.shape[1], A.shape[1]
    u, x_dbl = _Desc.fresh(x_half, (Bsz, L, Di), 6), _Desc.fresh(x_half, (Bsz, L, x_proj_w.shape[0]), 7)     # every u and x_dbl is a new allocation in xz's dtype
    front = ("conv_x_proj" if USE_CONV_X_PROJ and conv_x_proj_eligible(x_half, conv_w, conv_b, x_proj_w, perm, reset_period)
             else "conv+x_proj" if not train and USE_X_PROJ_KERNEL and x_proj_eligible(u, x_proj_w)
             else "conv+linear")     # training never takes the x_proj kernel (the rule as it has always been; no measurement either way)
    if train:                        # the training scan: whole sequence (it writes the backward's checkpoints), delta from the GEMM
        return InnerPlan(front, "linear", 0, False)
    chunk = split_chunk_len(Bsz, Di, L, reset_period)
    # policy: the split's first pass forms delta only with a bias and a gate it activates itself
    inside = (delta_softplus and B_proj_bias is None and C_proj_bias is None
              and (DT_PROJ_IN_SPLIT and delta_bias is not None and not z_preactivated if chunk else DT_PROJ_IN_SCAN)
              and dt_in_scan_eligible(u, x_dbl, dt_proj_w, reset_period, out if add_to is None else add_to, dstate=N, z=z_half, chunk_len=chunk, keep=blocks))
    dt = ("in_split" if chunk else "in_scan") if inside else "kernel" if delta_softplus and dt_proj_eligible(x_dbl, R, dt_proj_w) else "linear"
    return InnerPlan(front, dt, chunk, add_to is not None and dt == "in_scan" and ACCUMULATE_IN_SCAN)


def _run_front(plan, x_half, conv_w, conv_b, x_proj_w, perm, reset_period):
    """u = silu(conv(x_half)) in SCAN order and x_dbl = u @ x_proj_w.T, as plan.front says"""
    if plan.front == "conv_x_proj":
        return conv_x_proj(x_half, conv_w, conv_b, x_proj_w, perm)      # one pass: read x, write u and x_dbl
    u = torch.empty(x_half.shape, device=x_half.device, dtype=x_half.dtype)
    causal_conv1d_raw(x_half.transpose(1, 2), conv_w, conv_b, True, out=u.transpose(1, 2), x_row_index=perm, reset_period=reset_period)
    return u, (x_proj(u, x_proj_w) if plan.front == "conv+x_proj" else F.linear(u, x_proj_w))


class MambaInnerTokFn(torch.autograd.Function):
    """Autograd form of the token-major Mamba inner (conv + SiLU -> x_proj -> dt_proj -> gated selective scan) with the
    zigzag reordering fused into the kernels' row tables in BOTH directions (no index_select / index_add / cat):
    forward  = conv (x_row_index) -> GEMMs -> scan (z_row_index, out_row_index), saving u, x_dbl, delta and the ungated y;
    backward = scan bwd (same tables; dz lands in token order) -> the two skinny GEMM pairs -> conv bwd (dx scattered
    through x_row_index).  Mirrors MambaInnerFn (selective_scan_interface.py:296-434) without its out_proj.
    Under torch.autocast with a 16-bit xz and fp32 parameters (the reference's custom_fwd, :295-312): x_proj_w and dt_proj_w are replaced by their
    16-bit shadows (zigma_amd/amp.py) — the shadows are what is saved —, the conv taps, A, D and delta_bias stay fp32 (the kernels take them so);
    the backward runs with autocast off on operands of one type and returns every parameter gradient in the parameter's own type, the two GEMM
    weight gradients in fp32 straight from the fp32 sums."""

    @staticmethod
    def forward(ctx, xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias, perm, out_rows, reset_period, plan, *shadows):
        # shadows: (x_proj_w, dt_proj_w) in xz's type when the caller (mamba_inner_tok) already holds them for its plan
        ctx.amp = amp.mixed(xz, x_proj_w) and amp.mixed(xz, dt_proj_w)
        ctx.w_dtypes, ctx.n_extra = (x_proj_w.dtype, dt_proj_w.dtype), len(shadows)
        if ctx.amp:
            x_proj_w, dt_proj_w = shadows if shadows else (amp.shadow(x_proj_w, xz.dtype), amp.shadow(dt_proj_w, xz.dtype))
            with torch.autocast("cuda", enabled=False):
                return MambaInnerTokFn._forward(ctx, xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias, perm, out_rows, reset_period, plan)
        return MambaInnerTokFn._forward(ctx, xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias, perm, out_rows, reset_period, plan)

    @staticmethod
    def _forward(ctx, xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias, perm, out_rows, reset_period, plan):
        # reset_period > 0 (the video temporal layers): xz is the (k, b * t, 2 Di) strided VIEW of the (b * t, k, 2 Di) projection output —
        # batch = pixel, sequence = the frames of every sample one after the other, conv window and state restart every t steps; the
        # result and d(xz) are views of (b * t, k, .) allocations, so neither direction pays a transposing copy
        Bsz, L, C2 = xz.shape
        Di, R, N = C2 // 2, dt_proj_w.shape[1], A.shape[1]
        u, x_dbl = _run_front(plan, xz[:, :, :Di], conv_w.reshape(Di, -1), conv_b, x_proj_w, perm, reset_period)   # the backward takes both as saved
        delta = F.linear(x_dbl[:, :, :R], dt_proj_w)                     # (plan.dt is "linear" and plan.chunk_len 0 in training)
        Bm, Cm = x_dbl[:, :, R:R + N], x_dbl[:, :, R + N:R + 2 * N]
        out = torch.empty(Bsz, L, Di, device=xz.device, dtype=xz.dtype)
        # (strided input = a transposed view: hand the result back as the same kind of view of an (L, Bsz, Di) allocation)
        y = torch.empty(L, Bsz, Di, device=xz.device, dtype=xz.dtype).transpose(0, 1) if not xz.is_contiguous() else torch.empty_like(out)
        # the states before every 16-step tile, for the backward's reverse sweep (the token-major kernel writes them on
        # its way: 4 * Di * N * L / 16 bytes per sample; anything else leaves the buffer alone and the backward recomputes)
        ck_shape = _lib.checkpoint_shape(Bsz, Di, L, N)
        ck = torch.empty(*ck_shape, device=xz.device, dtype=torch.float32) if ck_shape else None
        info = []
        scan_raw(u.transpose(1, 2), delta.transpose(1, 2), A, Bm.transpose(1, 2).unsqueeze(1),
                 Cm.transpose(1, 2).unsqueeze(1), D, xz[:, :, Di:].transpose(1, 2), delta_bias, True,
                 out=out.transpose(1, 2), out_z=y.transpose(1, 2), z_row_index=perm, out_row_index=out_rows, checkpoints=ck,
                 info=info, reset_period=reset_period)
        if ck is not None and info[1] != 1:          # the kernel that served the call does not write checkpoints
            ck = None
        ctx.save_for_backward(xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias, u, x_dbl, delta, out)
        ctx.perm, ctx.out_rows, ctx.ck, ctx.reset_period = perm, out_rows, ck, reset_period
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.amp:
            with torch.autocast("cuda", enabled=False):
                return MambaInnerTokFn._backward(ctx, dy)
        return MambaInnerTokFn._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias, u, x_dbl, delta, out = ctx.saved_tensors
        # mixed precision: the fp32 sums of the two weight gradients, not rounded to the operand type
        wg = (lambda dy2, x2: wgrad(dy2, x2, out_dtype=torch.float32)) if ctx.amp else wgrad
        Bsz, L, C2 = xz.shape
        Di, R, N = C2 // 2, dt_proj_w.shape[1], A.shape[1]
        x_half, z_half = xz[:, :, :Di], xz[:, :, Di:]
        if dy.stride(2) != 1:
            dy = dy.contiguous()
        rp = ctx.reset_period
        dxz = torch.empty(L, Bsz, C2, device=xz.device, dtype=xz.dtype).transpose(0, 1) if not xz.is_contiguous() else torch.empty_like(xz)
        dx_dbl = torch.empty(Bsz, L, R + 2 * N, device=xz.device, dtype=torch.float32)
        du, ddelta, dA, _, _, dD, _, dbias = scan_bwd_tok(
            u, delta, A, x_dbl[:, :, R:R + N], x_dbl[:, :, R + N:R + 2 * N], D, z_half, delta_bias, dy, out, True,
            dB=dx_dbl[:, :, R:R + N], dC=dx_dbl[:, :, R + N:], dz=dxz[:, :, Di:], z_row_index=ctx.perm,
            out_row_index=ctx.out_rows, checkpoints=ctx.ck, reset_period=rp)
        ctx.ck = None
        dd2 = ddelta.reshape(-1, Di)
        dx_dbl[:, :, :R] = (dd2 @ dt_proj_w).reshape(Bsz, L, R)                  # d(x_dbl[:, :R]) = ddelta @ W_dt
        x_dt = x_dbl.reshape(-1, R + 2 * N)[:, :R]
        if plan_wgrad(dd2, x_dt) != "own":                                          # (the own kernel takes the 72-pitch column view as it is)
            x_dt = x_dt.contiguous()
        d_dt_w = wg(dd2, x_dt)                                                      # (Di, R)  zigma_linear_wgrad or token-slab GEMMs (zigma_amd/wgrad.py)
        dxd = dx_dbl.to(xz.dtype).reshape(-1, R + 2 * N)
        du = torch.addmm(du.reshape(-1, Di), dxd, x_proj_w).reshape(Bsz, L, Di)    # x_dbl = u @ W_x^T
        d_x_w = wg(dxd, u.reshape(-1, Di))                                         # (R + 2N, Di)
        _, d_cw, d_cb = conv_bwd_tok(x_half, conv_w, conv_b, du, True, ctx.perm, dx=dxz[:, :, :Di], reset_period=rp)
        return (dxz, d_cw.to(conv_w.dtype).reshape(conv_w.shape), None if d_cb is None else d_cb.to(conv_b.dtype),
                d_x_w.to(ctx.w_dtypes[0]), d_dt_w.to(ctx.w_dtypes[1]), dA.to(A.dtype), dD.to(D.dtype),
                None if dbias is None else dbias.to(delta_bias.dtype), None, None, None, None) + (None,) * ctx.n_extra


def selective_scan_cuda_fwd(u, delta, A, B, C, D_, z_, delta_bias_, delta_softplus):
    """Drop-in for the extension entry `selective_scan_cuda.fwd` -> [out, x] (+ [out_z] if z).
    Callee allocates: out = empty_like(delta), x (B, D, ceil(L/2048), 2N) f32, out_z = empty_like(z)."""
    batch, dim, L = u.shape
    x = torch.empty(batch, dim, (L + 2047) // 2048, 2 * A.shape[1], device=u.device, dtype=torch.float32)
    out, out_z = scan_raw(u, delta, A, B, C, D_, z_, delta_bias_, delta_softplus, x=x)
    return [out, x] if z_ is None else [out, x, out_z]


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                      return_last_state=False):
    """if return_last_state is True, returns (out, last_state); last_state is (batch, dim, dstate)."""
    batch, dim, L = u.shape
    x = None
    if return_last_state:
        x = torch.empty(batch, dim, (L + 2047) // 2048, 2 * A.shape[1], device=u.device, dtype=torch.float32)
    out, out_z = scan_raw(u, delta, A, B, C, D, z, delta_bias, delta_softplus, x=x, want_out=z is None)
    res = out if z is None else out_z
    return (res, x[:, :, -1, 1::2]) if return_last_state else res


def _inner_common(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B, C, D, delta_bias,
                  B_proj_bias, C_proj_bias, delta_softplus):
    """Reference-layout inner: xz (batch, 2*d_inner, seqlen).  Runs on the token-major kernels internally
    (one transposing copy in, none out)."""
    if B is not None or C is not None:
        raise RuntimeError("zigma_amd: only input-dependent B and C are supported (ZigMa always passes None)")
    xz_tok = xz.transpose(1, 2).contiguous()                      # (B, L, 2Di)
    return mamba_inner_tok(xz_tok, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, D, delta_bias,
                           B_proj_bias=B_proj_bias, C_proj_bias=C_proj_bias, delta_softplus=delta_softplus)


def mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias,
                   A, B=None, C=None, D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None,
                   delta_softplus=True):
    """xz: (batch, 2*dim, seqlen) -> (batch, seqlen, d_model)."""
    y = _inner_common(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B, C, D, delta_bias,
                      B_proj_bias, C_proj_bias, delta_softplus)
    return F.linear(y, out_proj_weight, out_proj_bias)


def mamba_inner_fn_no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B=None, C=None,
                               D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True):
    """xz: (batch, 2*dim, seqlen) -> out_z (batch, dim, seqlen)."""
    y = _inner_common(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B, C, D, delta_bias,
                      B_proj_bias, C_proj_bias, delta_softplus)
    return y.transpose(1, 2)


def mamba_inner_tok(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, D, delta_bias, *,
                    perm=None, out_rows=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True, out=None,
                    reset_period=0, z_preactivated=False, add_to=None):
    """Token-major Mamba inner (no out_proj).

    xz: (batch, seqlen, 2*d_inner), token order, channel contiguous (the in_proj GEMM output as is).
    perm: optional int32 (seqlen,) device table; the recurrence runs over tokens perm[0], perm[1], ...
          (zigzag / Hilbert order, reversed order for the backward sweep of `v2`); the result comes back
          in TOKEN order.  Semantics of mamba_simple.py:362-395: x'[k] = x[perm[k]], out[perm[k]] = out'[k].
    out_rows: optional int32 (seqlen,) table for the write-back when it is NOT the inverse of the gather:
          out[out_rows[k]] = out'[k] (defaults to perm).  The reference pairs its temporal table [0..T-1] with
          the "reverse" table [T-1..0] (model_zigma.py:765-772), i.e. out = out'[:, perm_rev] with perm_rev not
          the inverse of perm; the caller passes out_rows = inverse(perm_rev) to reproduce exactly that.
    reset_period: > 0 = every batch row is a concatenation of independent sequences of that many steps (multiple of 16):
          conv window and SSM state restart there (the video temporal layers: batch = k, seqlen = b * t on strided views).
    z_preactivated: the z half of xz already holds silu(z) (an in_proj epilogue wrote it; where z_preactivated_eligible holds).
    add_to: optional (batch, seqlen, d_inner) tensor y0 in token order (inference only): the result is y0 + y, written INTO y0 and returned — the second
          sweep of `v2` (mamba_simple.py:335-339), in the scan's epilogue or in place behind it (plan_inner: accumulate).
    Returns y (batch, seqlen, d_inner) in token order = out_z of the reference's scan, before out_proj.
    """
    if xz.dim() != 3 or xz.stride(2) != 1:
        raise RuntimeError("xz must be (batch, seqlen, 2*d_inner) with contiguous channels")
    train = differentiable(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, D, delta_bias)
    if train:
        if B_proj_bias is not None or C_proj_bias is not None or not delta_softplus or out is not None or z_preactivated or add_to is not None:
            raise NotImplementedError("differentiable mamba_inner_tok: no B/C projection bias, softplus on, no out= / add_to=, no pre-activated gate")
        if D is None or delta_bias is None:
            raise RuntimeError("the differentiable path expects D and delta_bias (ZigMa always has them)")
    elif add_to is not None and out is not None:
        raise RuntimeError("mamba_inner_tok: pass out= or add_to=, not both")
    Bsz, L, C2 = xz.shape
    Di, R, N = C2 // 2, delta_proj_weight.shape[1], A.shape[1]
    w, x_half, z_half = conv1d_weight.reshape(Di, -1), xz[:, :, :Di], xz[:, :, Di:]
    params, shadows = (x_proj_weight, delta_proj_weight), ()          # what MambaInnerTokFn differentiates; what its kernels read instead
    if amp.mixed(xz, x_proj_weight) and amp.mixed(xz, delta_proj_weight):
        # mixed precision: the kernels (and the plan) read the 16-bit shadows of the two GEMM weights; conv taps, A, D, delta_bias stay fp32
        x_proj_weight, delta_proj_weight = shadows = (amp.shadow(x_proj_weight, xz.dtype), amp.shadow(delta_proj_weight, xz.dtype))
    blocks = {}
    plan = plan_inner(x_half, z_half, w, conv1d_bias, x_proj_weight, delta_proj_weight, A, delta_bias, perm=perm, reset_period=reset_period,
                      z_preactivated=z_preactivated, out=out, add_to=add_to, B_proj_bias=B_proj_bias, C_proj_bias=C_proj_bias,
                      delta_softplus=delta_softplus, train=train, blocks=blocks)
    out_rows = perm if out_rows is None else out_rows
    if train:
        return MambaInnerTokFn.apply(xz, conv1d_weight, conv1d_bias, *params, A, D, delta_bias, perm, out_rows,
                                     int(reset_period), plan, *shadows)
    u, x_dbl = _run_front(plan, x_half, w, conv1d_bias, x_proj_weight, perm, reset_period)
    delta = None                     # "in_scan": dt_proj + bias + softplus inside the scan kernel's tile prologue, delta never exists
    if plan.dt == "in_split":        # the split's first pass forms delta and writes it into this workspace for the second
        delta = torch.empty(Bsz, L, Di, device=u.device, dtype=u.dtype)
    elif plan.dt == "kernel":        # K = dt_rank GEMM + bias + softplus in one write-bound MFMA kernel; the scan skips its softplus
        delta = dt_proj_softplus(x_dbl, R, delta_proj_weight, delta_bias, True)
        delta_bias, delta_softplus = None, False
    elif plan.dt == "linear":
        delta = F.linear(x_dbl[:, :, :R], delta_proj_weight)
    dt_inside = plan.dt in ("in_scan", "in_split")
    y = add_to if plan.accumulate else out if out is not None else torch.empty(Bsz, L, Di, device=u.device, dtype=u.dtype)
    xc = torch.empty(Bsz, Di, -(-L // plan.chunk_len), 2 * N, device=u.device, dtype=torch.float32) if plan.chunk_len else None   # split carries
    if dt_inside and "scan" in blocks and (add_to is None or plan.accumulate):
        # the block the dt decision asked the library about describes this very call (the result where the decision saw it: `out` / fresh rows,
        # or add_to when the scan adds to it): it gets its addresses and is launched, not built a second time
        scan_planned(blocks["scan"], u, x_dbl, delta, xc, y, z_half, A, D, delta_bias, perm, out_rows, z_preactivated, plan.accumulate)
        return y
    Bm, Cm = (M if b is None else M + b.to(M.dtype) for M, b in ((x_dbl[:, :, R:R + N], B_proj_bias), (x_dbl[:, :, R + N:R + 2 * N], C_proj_bias)))
    scan_raw(u.transpose(1, 2), None if delta is None else delta.transpose(1, 2), A, Bm.transpose(1, 2).unsqueeze(1),
             Cm.transpose(1, 2).unsqueeze(1), D, z_half.transpose(1, 2), delta_bias, delta_softplus,
             out_z=y.transpose(1, 2), z_row_index=perm, out_row_index=out_rows, want_out=False, x=xc, reset_period=reset_period,
             chunk_len=plan.chunk_len or 2048, z_preactivated=z_preactivated, dt_x=x_dbl if dt_inside else None,
             dt_w=delta_proj_weight if dt_inside else None, accumulate=plan.accumulate)
    return y if (add_to is None or plan.accumulate) else add_to.add_(y)
