"""Dense projections on the hand-written MFMA kernel (zigma_linear_fwd): in_proj / out_proj of the Mamba mixer and
to_q / to_out of the cross-attention (reference call sites mamba_simple.py:290-294, selective_scan_interface.py:365,
model_zigma.py:104-135, all `F.linear`), the text projections and the training path's forward product and dX (wgrad.LinearTrainFn, whose plan()
runs with autograd off); linear_eligible itself refuses tensors that require grad.  Which kernel serves which call: plan() and zigma_amd/routing.py.
The library's own refusals and kernel choice are plan_linear() (csrc/linear_plan.h), and nothing here restates them: every predicate builds the parameter
block the launch would get (linear_block, a fresh descriptor for the output) and asks the library (zigma_linear_fwd_plan).  What a block cannot say stays
here: _outside_the_block and _gate_outside_the_block."""
import torch

from . import _lib
from . import amp
from . import fp32_matmul
from . import routing


LINEAR_WS_FLAG, LINEAR_SM_FLAG = _lib.LINEAR_WS, _lib.LINEAR_SM
FAMILY_FLAG = routing.SELECTOR          # the kernel selector of each family one launch serves


def linear_block(x, weight, bias=None, out=None, residual=None, gate=None, silu_from_col=None, flags=0):
    """The parameter block of zigma_linear_fwd: x (m, k) rows one pitch apart or contiguous (..., k), weight (n, k), out (m, n) rows (None: fresh contiguous
    rows, a placeholder address — a block to ask about), residual (B, rows, n) rows of all samples in one pitch + gate (B, n).  Reads shapes, strides, dtypes
    and addresses only, so descriptors (_lib.Desc) serve as well as tensors."""
    n, k = weight.shape[0], x.shape[-1]
    m = x.numel() // k
    P = _lib.LinearParams()
    P.m, P.n, P.k, P.dtype, P.flags = m, n, k, _lib.dtype_id(x), flags
    P.silu_from_col = n if silu_from_col is None else int(silu_from_col)
    P.x_row_stride, P.w_row_stride, P.out_row_stride = x.stride(-2), weight.stride(0), n if out is None else out.stride(-2)
    P.x, P.w, P.bias, P.out = x.data_ptr(), weight.data_ptr(), _lib.ptr(bias), _lib.FRESH_ADDRESS if out is None else out.data_ptr()
    return P if residual is None else _with_gated_residual(P, residual, gate)


def _with_gated_residual(P, residual, gate):
    P.residual, P.gate = _lib.ptr(residual), _lib.ptr(gate)
    P.res_row_stride, P.gate_batch_stride, P.rows_per_batch = residual.stride(1), gate.stride(0), residual.shape[1]
    return P


def _without_gated_residual(P):
    P.residual = P.gate = None
    P.res_row_stride = P.gate_batch_stride = P.rows_per_batch = 0
    return P


def _served(P):
    status, kernel = _lib.plan("zigma_linear_fwd", P)
    return status == 0 and kernel is not None


def _outside_the_block(x, weight, bias):
    """what the parameter block cannot say of a call: the device, ONE dtype for all operands (the block has one), unit channel strides and bias stride (it has
    row pitches only), a > 2-D x that is one sequence of rows (the reshape would copy otherwise), and the autograd rule (the kernels have no backward)"""
    if not (x.is_cuda and x.dim() >= 2 and x.dtype in _lib._DT and weight.dtype == x.dtype and len(weight.shape) == 2):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return False
    if x.shape[-1] != weight.shape[1] or x.stride(-1) != 1 or weight.stride(1) != 1 or (bias is not None and (bias.dtype != x.dtype or bias.stride(0) != 1)):
        return False
    return x.dim() == 2 or x.is_contiguous()


def linear_eligible(x, weight, bias=None, _flags=0, _block=None):
    """zigma_linear_fwd's tiled kernels take x @ weight.T (+ bias) on these tensors (no policy — which projection runs where is zigma_amd/routing.py): what
    plan_linear() serves without a kernel selector, and _outside_the_block.  _block (plan(), which asks nobody else): the call's block as a route would
    launch it — the refusals all kernels share come first in plan_linear(), so a block it serves with a selector or an epilogue is also served plain."""
    P = _block if _block is not None else linear_block(x, weight, bias, flags=_flags) if _outside_the_block(x, weight, bias) else None
    return P is not None and _served(P)


def linear_ws_eligible(x, weight, bias=None):
    """... under ZIGMA_LINEAR_WS: the weight-stationary kernel (csrc/linear_ws.hip: a W panel lives in a workgroup's registers, only the tokens stream)"""
    return linear_eligible(x, weight, bias, LINEAR_WS_FLAG)


def linear_sm_eligible(x, weight, bias=None):
    """... under ZIGMA_LINEAR_SM: the few-token kernel (csrc/linear_sm.hip: 128 tokens x n / 4 features per workgroup; the gated residual: gated_residual_eligible)"""
    return linear_eligible(x, weight, bias, LINEAR_SM_FLAG)


def linear(x, weight, bias=None, silu_from_col=None, out=None, _probe_flags=0, residual=None, gate=None, weight_stationary=False, few_tokens=False):
    """out = x @ weight.T (+ bias); output columns >= silu_from_col (a multiple of 32) leave as silu(.).
    residual (same shape as the result) + gate (batch, n): out = residual + gate[b] * r16(x @ weight.T + bias) (r16: rounded to the I/O type) in the kernel's
    epilogue (the gated branch add of the reference's Block, model_zigma.py:447-449); x must then be (batch, rows, k) with
    rows % 256 == 0.  weight_stationary: the csrc/linear_ws.hip kernel (linear_ws_eligible shapes only; fails otherwise); few_tokens: the
    csrc/linear_sm.hip kernel (linear_sm_eligible shapes only)."""
    dev = _lib.require_device(x, weight, bias, out, residual, gate)
    lead, k = x.shape[:-1], x.shape[-1]
    x2 = x.reshape(-1, k)
    n = weight.shape[0]
    if out is None:
        out = torch.empty(x2.shape[0], n, device=x.device, dtype=x.dtype)
    o2 = out if out.dim() == 2 else out.view(-1, n)            # a view: the kernel writes through the row pitch
    if residual is not None and (gate is None or x.dim() != 3 or residual.shape != (*lead, n) or residual.dtype != x.dtype or gate.dtype != x.dtype
                                 or gate.shape != (x.shape[0], n) or gate.stride(1) != 1 or residual.stride(-1) != 1 or not residual_rows_ok(residual)):
        raise RuntimeError("linear: residual (B, rows, n) with uniform row pitch and gate (B, n) rows in the dtype of x")
    flags = int(_probe_flags) | (LINEAR_WS_FLAG if weight_stationary else LINEAR_SM_FLAG if few_tokens else 0)
    _lib.call("zigma_linear_fwd", linear_block(x2, weight, bias, o2, residual, gate, silu_from_col, flags), dev)
    return out if out.dim() == len(lead) + 1 and out.shape[:-1] == lead else out.view(*lead, n)


def linear_planned(P, x, weight, bias=None, residual=None, gate=None, silu_from_col=None):
    """Launch the block plan() built and the library accepted, on the tensors plan() saw (or, for its stand-ins, the tensors they stood for): layout, sizes
    and flags stand as planned; the addresses — the output's a placeholder so far — and the SiLU range are set here."""
    dev = _lib.require_device(x, weight, bias, residual, gate)
    lead = x.shape[:-1]
    x2 = x if x.dim() == 2 else x.reshape(-1, P.k)
    if (x2.shape[0], x2.stride(0), weight.stride(0), bias is None, residual is None) != (P.m, P.x_row_stride, P.w_row_stride, P.bias is None, P.residual is None) \
            or (residual is not None and (residual.stride(1), gate.stride(0)) != (P.res_row_stride, P.gate_batch_stride)):
        raise RuntimeError("linear.run: not the tensors this route was planned on")
    out = torch.empty(P.m, P.n, device=x.device, dtype=x.dtype)
    P.x, P.w, P.bias, P.out, P.residual, P.gate = x2.data_ptr(), weight.data_ptr(), _lib.ptr(bias), out.data_ptr(), _lib.ptr(residual), _lib.ptr(gate)
    if silu_from_col is not None:
        P.silu_from_col = int(silu_from_col)
    _lib.call("zigma_linear_fwd", P, dev)
    return out.view(*lead, P.n)


def residual_rows_ok(residual):
    """(B, rows, n) whose rows of all samples form ONE sequence of rows of the same pitch"""
    return residual.dim() == 3 and residual.stride(0) == residual.shape[1] * residual.stride(1)


def _gate_outside_the_block(x, residual, gate):
    """what the block cannot say of the gated-residual operands: (B, rows, k) input, one dtype, residual rows of all samples in one pitch, unit channel strides"""
    return (x.dim() == 3 and x.dtype in _lib._DT and residual.dtype == x.dtype and gate.dtype == x.dtype and residual_rows_ok(residual) and residual.stride(-1) == 1
            and gate.dim() == 2 and gate.stride(1) == 1)


def gated_residual_eligible(x, residual, gate):
    """the gated-residual epilogue takes these operands: what plan_linear() serves for the product of x with an aligned contiguous weight of residual's width
    into fresh rows with residual and gate attached, and _gate_outside_the_block"""
    if not _gate_outside_the_block(x, residual, gate):
        return False
    weight = _lib.Desc.fresh(x, (residual.shape[-1], x.shape[-1]), 2)
    return _served(linear_block(x, weight, None, None, residual, gate))


class _Planned(routing.Route):
    """the Route of a call one launch of zigma_linear_fwd serves, carrying the parameter block the library accepted for it (run launches it: linear_planned).
    Compares, unpacks and _replaces as the Route it is."""
    block = None


def plan(role, x, weight, bias=None, residual=None, gate=None):
    """The ONE decision which kernel serves a projection (routing.ROLES) on these tensors: the first route of the table (routing.candidates) whose
    kernel the library's plan serves the call's parameter block with (that family's selector set); a route the library refuses is logged in routing.REFUSED and
    the walk goes on.  Calls no own kernel can take (mixed dtypes, CPU tensors, autograd, fp32 models unless fp32_matmul.PRECISION opts them into the bf16-split
    kernel) are the library's.  fuse_add: the kernel carries residual + gate[:, None] * (.) in its epilogue (the route fuses, residual / gate are given and
    the plan serves the block with them attached, no autograd).  Under torch.autocast a 16-bit activation beside an fp32 weight is planned on the weight's
    16-bit shadow (zigma_amd/amp.py): the same rows as for a model of that type.  The route of a single launch carries its accepted block to run()."""
    if torch.is_autocast_enabled():
        w0, b0 = weight, bias
        weight, bias = amp.planned(x, weight, bias)          # (stand-ins of the shadows: a plan casts nothing)
        if weight is not w0 and torch.is_grad_enabled() and (w0.requires_grad or (b0 is not None and b0.requires_grad)):
            return routing.Route("library", False, "autograd")        # (the shadows require no grad; the parameters do: wgrad.linear_train)
    P = linear_block(x, weight, bias) if _outside_the_block(x, weight, bias) else None
    fuse = P is not None and residual is not None and not torch.is_grad_enabled() and _gate_outside_the_block(x, residual, gate)
    if P is not None:           # the usual call in one question: the table's first route as it would launch (a refusal is sorted out one question at a time below)
        r = routing.route(role, P.m, P.n, P.k)
        if r.kernel in FAMILY_FLAG:
            P.flags = FAMILY_FLAG[r.kernel]
            if fuse and r.fuse_add:
                _with_gated_residual(P, residual, gate)
            if linear_eligible(x, weight, bias, _block=P):
                return _planned(r, P)
            _without_gated_residual(P).flags = 0
        elif r.kernel == "library" and linear_eligible(x, weight, bias, _block=P):
            return r
    if P is None or not linear_eligible(x, weight, bias, _block=P):
        # fp32 tensors of an inference call, opted in by fp32_matmul.PRECISION: the bf16-split kernel, for every role; its gated add stays where the
        # library route leaves it (project's addcmul, or the next norm kernel)
        mode = fp32_matmul.PRECISION
        if mode != "highest" and x.dtype == torch.float32 and routing.POLICY != "off" and fp32_matmul.split_eligible(x, weight, bias):
            return routing.Route(fp32_matmul.ROUTE_KERNEL[mode], False, "fp32." + mode)
        return routing.Route("library", False, "not-16bit-inference")
    for r in routing.candidates(role, P.m, P.n, P.k):
        if r.kernel == "library":
            return r
        if r.kernel == "tiled_halves":          # each half is a tiled call on half of the weight rows into its columns of a 3-D result, without a bias: the table
            if bias is None and x.dim() == 3:    # asked the plan about a half's shape, and the halves' pitches and alignments are those of the block just served
                return r
        else:                                   # (the table took family and panel width from the plan's answer for the shape: routing.serves)
            P.flags = FAMILY_FLAG[r.kernel]
            if not P.flags or linear_eligible(x, weight, bias, _block=P):          # (without a selector: the block the library has just served)
                if fuse and r.fuse_add and not linear_eligible(x, weight, bias, _block=_with_gated_residual(P, residual, gate)):
                    _without_gated_residual(P)
                return _planned(r, P)
        routing.REFUSED.append((role, P.m, P.n, P.k, r.kernel))
        del routing.REFUSED[:-64]


def _planned(r, P):
    planned = _Planned(r.kernel, P.residual is not None, r.row)
    planned.block = P
    return planned


def run(r, x, weight, bias=None, residual=None, gate=None, silu_from_col=None):
    """x @ weight.T (+ bias) on the kernel of plan()'s route r — with residual + gate[:, None] * (.) in its epilogue if r.fuse_add; a library route
    is wgrad.linear_train (F.linear; under autograd with the slab-wise weight gradient).  silu_from_col: the weight-stationary kernel's SiLU epilogue."""
    if r.kernel == "library":
        from .wgrad import linear_train
        return linear_train(x, weight, bias)
    if torch.is_autocast_enabled():                  # (the operands plan() judged; the library route above takes the parameters themselves: autograd)
        weight, bias = amp.operands(x, weight, bias)
    if r.kernel in ("split3", "split1"):
        return fp32_matmul.linear_split(x, weight, bias, mode="high" if r.kernel == "split3" else "medium")
    if r.kernel == "tiled_halves":
        n = weight.shape[0]
        y = torch.empty(*x.shape[:-1], n, device=x.device, dtype=x.dtype)
        o2 = y.view(-1, n)
        linear(x, weight[:n // 2], out=o2[:, :n // 2])
        linear(x, weight[n // 2:], out=o2[:, n // 2:])
        return y
    residual, gate = (residual, gate) if r.fuse_add else (None, None)
    if getattr(r, "block", None) is not None:             # plan()'s route: the block the library accepted, not built again
        return linear_planned(r.block, x, weight, bias, residual, gate, silu_from_col)
    return linear(x, weight, bias, silu_from_col=silu_from_col, residual=residual, gate=gate, weight_stationary=r.kernel in ("ws", "ws128"),
                  few_tokens=r.kernel == "sm")


def project(role, x, weight, bias=None, residual=None, gate=None):
    """The projections through ONE dispatch (plan, then run).  residual (B, L, n) + gate (B, n): the result is residual + gate[:, None] * (x @ weight.T
    + bias) — in the serving kernel's epilogue where plan() fuses the add, as an addcmul behind the product otherwise."""
    r = plan(role, x, weight, bias, residual, gate)
    y = run(r, x, weight, bias, residual, gate)
    return y if residual is None or r.fuse_add else torch.addcmul(residual, gate.unsqueeze(1), y)
