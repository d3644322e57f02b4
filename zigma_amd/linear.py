"""Dense projections on the hand-written MFMA kernel (zigma_linear_fwd): in_proj / out_proj of the Mamba mixer and
to_q / to_out of the cross-attention (reference call sites mamba_simple.py:290-294, selective_scan_interface.py:365,
model_zigma.py:104-135, all `F.linear`), the text projections and the training path's forward product and dX (wgrad.LinearTrainFn, whose plan()
runs with autograd off); linear_eligible itself refuses tensors that require grad.  Which kernel serves which call: plan() and zigma_amd/routing.py.
The library's own refusals and kernel choice are plan_linear() (csrc/linear_plan.h); linear_eligible, _TENSOR_LIMITS and routing.serves_* restate its limits
for tensors and shapes, and tests/test_host_cpu.py checks them against the compiled header."""
import torch

from . import _lib
from . import amp
from . import fp32_matmul
from . import routing


MFMA_DTYPES = (torch.bfloat16, torch.float16)      # the I/O types of the matrix-core kernels; all operands of a call share one


def linear_eligible(x, weight, bias=None):
    """LIMITS of zigma_linear_fwd's tiled kernels on these tensors (no policy — which projection runs where is zigma_amd/routing.py): bf16 or fp16
    (x, weight and bias in ONE of them) on the device, k % 64 == 0, n % 128 == 0, tokens % 8 == 0, aligned contiguous rows, no autograd"""
    if not (x.is_cuda and x.dtype in MFMA_DTYPES and weight.dtype == x.dtype):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return False
    n, k = weight.shape
    if k % 64 or n % 128 or x.shape[-1] != k or x.stride(-1) != 1 or weight.stride(1) != 1:
        return False
    if bias is not None and (bias.dtype != x.dtype or bias.stride(0) != 1 or n > 4096 or bias.data_ptr() % 4):
        return False                                     # (the kernel stages the bias vector in 8 KB of LDS)
    m = x.numel() // k
    if m % 8 or m == 0:
        return False
    if x.dim() > 2 and not x.is_contiguous():
        return False
    if x.stride(-2) % 8 or weight.stride(0) % 8 or x.data_ptr() % 16 or weight.data_ptr() % 16:
        return False
    return m * x.stride(-2) * 2 < 2 ** 31 and n * weight.stride(0) * 2 < 2 ** 31 and 256 * n * 2 < 2 ** 31


LINEAR_WS_FLAG = 0x4000          # zigma_linear_params_t.flags: ZIGMA_LINEAR_WS (csrc/linear_ws.hip)


def linear_ws_eligible(x, weight, bias=None):
    """limits of the weight-stationary kernel (csrc/linear_ws.hip: a W panel lives in the registers of a workgroup, only the tokens stream):
    linear_eligible's, the shape limits of routing.serves_ws (k = 512 / 640 with 256-feature panels, k = 1280 / 1536 with 128-feature panels, at
    most 32 panels, whole 512-token tiles for every workgroup of an XCD) and the tensor limits of _TENSOR_LIMITS["ws"] (no bias, x rows a multiple
    of 128 elements apart)."""
    n, k = weight.shape
    return linear_eligible(x, weight, bias) and routing.serves_ws(x.numel() // k, n, k) and _TENSOR_LIMITS["ws"](x, bias)


LINEAR_SM_FLAG = 0x8000          # zigma_linear_params_t.flags: ZIGMA_LINEAR_SM (csrc/linear_sm.hip)


def linear_sm_eligible(x, weight, bias=None):
    """limits of the few-token tiled kernel (csrc/linear_sm.hip: tiles of 128 tokens x n / 4 features, one per workgroup — 8192 tokens x 640
    features are exactly 256 tiles): linear_eligible's, the shape limits of routing.serves_sm (k >= 128, whole 128-token tiles) and the tensor
    limits of _TENSOR_LIMITS["sm"] (a bias on an 8-byte boundary).  The gated residual epilogue: gated_residual_eligible, as for the tiled kernels."""
    n, k = weight.shape
    return linear_eligible(x, weight, bias) and routing.serves_sm(x.numel() // k, n, k) and _TENSOR_LIMITS["sm"](x, bias)


# What each kernel family asks of the tensors on top of linear_eligible and its shape limits (routing._SERVES)
_TENSOR_LIMITS = {
    "ws": lambda x, bias: bias is None and x.stride(-2) % 128 == 0,         # (no epilogue operands in this kernel)
    "sm": lambda x, bias: bias is None or bias.data_ptr() % 8 == 0,
    "tiled": lambda x, bias: True,
    "tiled_halves": lambda x, bias: bias is None and x.dim() == 3,          # (each half is a tiled call on half of the weight rows)
    "library": lambda x, bias: True,
}
_TENSOR_LIMITS["ws128"] = _TENSOR_LIMITS["ws"]


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
    P = _lib.LinearParams()
    P.m, P.n, P.k, P.dtype, P.flags = x2.shape[0], n, k, _lib.dtype_id(x), int(_probe_flags) | (LINEAR_WS_FLAG if weight_stationary else LINEAR_SM_FLAG if few_tokens else 0)
    P.silu_from_col = n if silu_from_col is None else int(silu_from_col)
    P.x_row_stride, P.w_row_stride, P.out_row_stride = x2.stride(0), weight.stride(0), o2.stride(0)
    P.x, P.w, P.bias, P.out = _lib.ptr(x2), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(o2)
    if residual is not None:
        if gate is None or x.dim() != 3 or residual.shape != (*lead, n) or residual.dtype != x.dtype or gate.dtype != x.dtype \
                or gate.shape != (x.shape[0], n) or gate.stride(1) != 1 or residual.stride(-1) != 1 or not residual_rows_ok(residual):
            raise RuntimeError("linear: residual (B, rows, n) with uniform row pitch and gate (B, n) rows in the dtype of x")
        P.residual, P.gate = _lib.ptr(residual), _lib.ptr(gate)
        P.res_row_stride, P.gate_batch_stride, P.rows_per_batch = residual.stride(1), gate.stride(0), x.shape[1]
    _lib.call("zigma_linear_fwd", P, dev)
    return out if out.dim() == len(lead) + 1 and out.shape[:-1] == lead else out.view(*lead, n)


def residual_rows_ok(residual):
    """(B, rows, n) whose rows of all samples form ONE sequence of rows of the same pitch"""
    return residual.dim() == 3 and residual.stride(0) == residual.shape[1] * residual.stride(1)


def gated_residual_eligible(x, residual, gate):
    """limits of the gated-residual epilogue: (B, rows % 256 == 0, k) bf16 or fp16 input, residual rows of the same dtype 16-byte aligned in
    one pitch, gate rows of the same dtype 16-byte aligned"""
    return (x.dtype in MFMA_DTYPES and x.dim() == 3 and x.shape[1] % 256 == 0 and residual.dtype == x.dtype and gate.dtype == x.dtype and residual_rows_ok(residual)
            and residual.stride(-1) == 1 and residual.stride(1) % 8 == 0 and residual.data_ptr() % 16 == 0
            and gate.dim() == 2 and gate.stride(1) == 1 and gate.stride(0) % 8 == 0 and gate.data_ptr() % 16 == 0
            and 256 * residual.stride(1) * 2 < 2 ** 31)


def plan(role, x, weight, bias=None, residual=None, gate=None):
    """The ONE decision which kernel serves a projection (routing.ROLES) on these tensors: the first route of the table (routing.candidates) whose
    kernel's shape and tensor limits the call meets; a route the tensors refuse is logged in routing.REFUSED and the walk goes on.  Calls no own kernel
    can take (mixed dtypes, CPU tensors, autograd, fp32 models unless fp32_matmul.PRECISION opts them into the bf16-split kernel) are the library's.  fuse_add: the kernel carries residual + gate[:, None] * (.) in its
    epilogue (the route fuses, residual / gate are given and meet the epilogue's limits, no autograd).  Under torch.autocast a 16-bit activation beside an fp32
    weight is planned on the weight's 16-bit shadow (zigma_amd/amp.py): the same rows as for a model of that type."""
    if torch.is_autocast_enabled():
        w0, b0 = weight, bias
        weight, bias = amp.planned(x, weight, bias)          # (stand-ins of the shadows: a plan casts nothing)
        if weight is not w0 and torch.is_grad_enabled() and (w0.requires_grad or (b0 is not None and b0.requires_grad)):
            return routing.Route("library", False, "autograd")        # (the shadows require no grad; the parameters do: wgrad.linear_train)
    n, k = weight.shape
    if not linear_eligible(x, weight, bias):
        # fp32 tensors of an inference call, opted in by fp32_matmul.PRECISION: the bf16-split kernel, for every role; its gated add stays where the
        # library route leaves it (project's addcmul, or the next norm kernel)
        mode = fp32_matmul.PRECISION
        if mode != "highest" and x.dtype == torch.float32 and routing.POLICY != "off" and fp32_matmul.split_eligible(x, weight, bias):
            return routing.Route(fp32_matmul.ROUTE_KERNEL[mode], False, "fp32." + mode)
        return routing.Route("library", False, "not-16bit-inference")
    tokens = x.numel() // k
    for r in routing.candidates(role, tokens, n, k):
        if _TENSOR_LIMITS[r.kernel](x, bias):
            fuse = r.fuse_add and residual is not None and not torch.is_grad_enabled() and gated_residual_eligible(x, residual, gate)
            return r._replace(fuse_add=fuse)
        routing.REFUSED.append((role, tokens, n, k, r.kernel))
        del routing.REFUSED[:-64]


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
    return linear(x, weight, bias, silu_from_col=silu_from_col, residual=residual if r.fuse_add else None, gate=gate if r.fuse_add else None,
                  weight_stationary=r.kernel in ("ws", "ws128"), few_tokens=r.kernel == "sm")


def project(role, x, weight, bias=None, residual=None, gate=None):
    """The projections through ONE dispatch (plan, then run).  residual (B, L, n) + gate (B, n): the result is residual + gate[:, None] * (x @ weight.T
    + bias) — in the serving kernel's epilogue where plan() fuses the add, as an addcmul behind the product otherwise."""
    r = plan(role, x, weight, bias, residual, gate)
    y = run(r, x, weight, bias, residual, gate)
    return y if residual is None or r.fuse_add else torch.addcmul(residual, gate.unsqueeze(1), y)
