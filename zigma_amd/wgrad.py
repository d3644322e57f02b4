"""Weight gradients of the block's projections for the training path: dW = dY^T X with the TOKENS as the contraction dimension
(M = batch x seqlen = 65 536 at the headline shape against outputs of 72 x 1280 ... 2560 x 640 elements).

The reference leaves these to autograd's linear backward (one GEMM each); as ONE library GEMM they are 5 ... 100 output tiles for 256
CUs and run at 0.03 ... 0.5 PFLOP/s (tools/wgrad_split_probe.py: in_proj 450 us, to_q 259 us, x_proj 227 us).  Split along the tokens
into S slabs as a BATCHED GEMM (the slab index is the library's batch dimension) the same products fill the chip; the S partial
results (bf16, like a GEMM output) are added in fp32: in_proj 332 us, out_proj 303 -> 149, to_q 259 -> 76, to_out 271 -> 66,
x_proj 227 -> 72, dt_proj 205 -> 64 us — 17 ms of a 122 ms training step.  `LinearTrainFn` is F.linear with that backward; since round 4 its forward product and dX run on the hand-written projection kernels
(zigma_linear_fwd) where one serves the shape — the "train" rows of zigma_amd/routing.py (routing.POLICY="off": the library for both).

The same products have an own entry point, zigma_linear_wgrad (csrc/wgrad.hip: split-K over token slabs, MFMA operands by transposed LDS reads, fp32 partials
added in slab order, row-strided operands): wgrad_own() launches it, own_serves() asks the library's plan of it (csrc/wgrad_plan.h) about the block wgrad_block() builds, plan_wgrad() decides per product between it and the slab bmm (PLAN_TABLE; knob OWN_WGRAD)."""
import ctypes
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import _knobs, _lib, amp
from .linear import plan, run

SPLIT_WGRAD = True        # False: one GEMM (A/B in tools/train_probe.py)
OWN_WGRAD = True          # True: PLAN_TABLE decides between zigma_linear_wgrad and the slab bmm;  False: never the own kernel (the A/B partner);
#                           "all": the own kernel wherever its tensor-level limits hold (tools/wgrad_split_probe.py measures the table's rows with it)


_BMM_OUT_DTYPE = {}      # (device type, index, dtype) -> bool


def _bmm_takes_out_dtype(x):
    """does torch.bmm accept out_dtype=float32 for x's dtype ON x's device?  Probed lazily, once per (device, dtype), with a 1 x 1 x 1 product there (an
    import-time probe on the CPU says nothing about the GPU backend).  Only the two answers that mean "no" are caught — a missing keyword (TypeError) and a
    backend that declines the combination (RuntimeError naming it); anything else (e.g. out of memory) propagates."""
    key = (x.device.type, x.device.index, x.dtype)
    hit = _BMM_OUT_DTYPE.get(key)
    if hit is None:
        a = torch.zeros(1, 1, 1, device=x.device, dtype=x.dtype)
        try:
            torch.bmm(a, a, out_dtype=torch.float32)
            hit = True
        except TypeError:
            hit = False
        except RuntimeError as e:
            msg = str(e).lower()
            if not any(w in msg for w in ("out_dtype", "not implemented", "not supported", "unsupported", "expected")):
                raise
            hit = False
        _BMM_OUT_DTYPE[key] = hit
    return hit


def _ContiguousLike(weight):
    """Stand-in for `weight.t().contiguous()` in linear.plan, which reads device, dtype, shape, strides and the address's alignment (a fresh allocation is
    aligned: a placeholder address) — so the kernel is chosen before the copy is made, and the copy is only made for a kernel."""
    return _lib.Desc.fresh(weight, (weight.shape[1], weight.shape[0]), 2)


def _slabs(m, n, k):
    """number of token slabs: enough (128 x 128)-tile workgroups for ~2 per CU, a power of two dividing m, slabs of >= 256 rows"""
    tiles = max(1, -(-n // 128) * -(-k // 128))
    s = 8
    while s < 64 and s * tiles < 512:
        s *= 2
    while s > 1 and (m % s or (m // s) < 256 or (m // s) % 8):
        s //= 2
    return s


# ---- the own split-K kernel (csrc/wgrad.hip, zigma_linear_wgrad) ------------------------------------------------------------------------------
INF = 1 << 40
WgradRow = namedtuple("WgradRow", "id n k tokens path why")
# n / k / tokens: (lo, hi) inclusive; the first matching row wins.  n = columns of dY = rows of dW, k = columns of X.
# `why` carries the measurement that decided the row (tools/wgrad_split_probe.py --own-ab, profiles/wgrad_own_vs_bmm.jsonl).
PLAN_TABLE = (
    WgradRow("few_tokens", (8, 8192), (8, 8192), (1, 255), "bmm",
             "not measured: below 256 tokens one GEMM of the library is a single small launch and the kernel has at most four 64-token steps per workgroup to hide its prologue under"),
    WgradRow("skinny_n", (8, 128), (8, 8192), (256, INF), "bmm",
             "x_proj (72 x 1280): one 128-row tile covers n, X streams exactly once (168 MB at 65 536 tokens; the slab bmm: 72 us, round 4).  own vs bmm NOT MEASURED on the MI355X yet "
             "(tools/wgrad_split_probe.py --own-ab): the row stays on the measured path until it is"),
    WgradRow("skinny_k", (136, 8192), (8, 64), (256, INF), "bmm",
             "dt_proj (1280 x 40): one 64-column tile covers k, dY streams exactly once and the 72-pitch view of x_dbl needs no copy (the slab bmm: 64 us + the copy, round 4).  own vs bmm "
             "NOT MEASURED on the MI355X yet: the row stays on the measured path until it is"),
    WgradRow("dense", (136, 8192), (72, 8192), (256, INF), "bmm",
             "in_proj / out_proj / to_q / to_out (slab bmm: 332 / 149 / 76 / 66 us at 65 536 tokens, round 4): compute-bound; the kernel stages one 64-token step through registers behind two "
             "barriers, the form that measured 4 x behind the library in round 3 (tools/experiments/wgrad_tr_r03.hip: in_proj 1260 vs 332 us).  own vs bmm of THIS kernel NOT MEASURED yet"),
)


def wgrad_block(dy2, x2, out_dtype=None, slabs=0, out=None, workspace=None):
    """The parameter block of zigma_linear_wgrad: dy2 (m, n) rows, x2 (m, k) rows, out (n, k) rows of out_dtype (None: fresh rows, a placeholder address —
    a block to ask about), the workspace the library asks for at this shape (None: a placeholder of that size).  Reads shapes, strides, dtypes and
    addresses only."""
    (m, n), k = dy2.shape, x2.shape[1]
    out_dtype = out_dtype or (out.dtype if out is not None else dy2.dtype)
    if out is None:
        out = _lib.Desc.fresh(dy2, (n, k), 1, out_dtype)
    P = _lib.LinearWgradParams()
    P.m, P.n, P.k, P.slabs, P.flags = m, n, k, int(slabs), 0
    # (a mixed pair has no representation in the block: it goes in as an unknown operand type and comes back as ZIGMA_ERR_DTYPE)
    P.dtype = _lib._DT.get(dy2.dtype, -1) if x2.dtype == dy2.dtype else -1
    P.out_dtype = _lib._DT.get(out_dtype, -1)
    P.dy_row_stride, P.x_row_stride, P.out_row_stride = dy2.stride(0), x2.stride(0), out.stride(0)
    P.dy, P.x, P.out = _lib.ptr(dy2), _lib.ptr(x2), _lib.ptr(out)
    if workspace is None:
        P.workspace, P.workspace_bytes = 2 * _lib.FRESH_ADDRESS, _lib.lib().zigma_linear_wgrad_workspace_bytes(ctypes.byref(P))
    else:
        P.workspace, P.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return P


def own_serves(dy2, x2):
    """zigma_linear_wgrad takes these tensors: what plan_wgrad() (csrc/wgrad_plan.h) serves, asked through the library, and what the block cannot say —
    two matrices with the same rows on the device, unit channel strides"""
    if not (dy2.is_cuda and x2.is_cuda) or len(dy2.shape) != 2 or len(x2.shape) != 2 or dy2.shape[0] != x2.shape[0]:
        return False
    return dy2.stride(1) == 1 and x2.stride(1) == 1 and _lib.served("zigma_linear_wgrad", wgrad_block(dy2, x2))


def plan_row(dy2, x2):
    """the PLAN_TABLE row a product falls on (None: the tensors are outside the kernel's limits, or the knob is off)"""
    if OWN_WGRAD is False or torch.is_autocast_enabled() or not own_serves(dy2, x2):
        return None
    m, n, k = dy2.shape[0], dy2.shape[1], x2.shape[1]
    for row in PLAN_TABLE:
        if row.n[0] <= n <= row.n[1] and row.k[0] <= k <= row.k[1] and row.tokens[0] <= m <= row.tokens[1]:
            return row
    return None


def plan_wgrad(dy2, x2):
    """"own" (zigma_linear_wgrad) or "bmm" (the slab-wise library product below) for dW = dy2^T x2 — the ONE place that decides.  Two layers: the
    tensor-level limits of the entry point, then PLAN_TABLE.  Independent of routing.POLICY (the own-vs-library tests of the forward kernels
    compare w.grad bit for bit across its settings)."""
    row = plan_row(dy2, x2)
    if row is None:
        return "bmm"
    return "own" if OWN_WGRAD == "all" else row.path


def wgrad_own(dy2, x2, out_dtype=None, slabs=0, out=None, workspace=None):
    """dy2 (m, n), x2 (m, k) -> dy2^T x2 (n, k) by zigma_linear_wgrad: fp32 slab partials in a workspace, added in slab order, one rounding to
    `out_dtype` (the operand dtype, or torch.float32).  Row-strided operands (column views) pass as they are.  slabs = 0: the library's choice.
    out / workspace: caller-provided buffers (tests); the limits are the C side's — a refusal raises RuntimeError with its status."""
    dev = _lib.require_device(dy2, x2, out, workspace)
    if dy2.dim() != 2 or x2.dim() != 2 or dy2.shape[0] != x2.shape[0]:
        raise RuntimeError("wgrad_own: dy2 (m, n) and x2 (m, k) with the same m")
    if dy2.stride(1) != 1 or x2.stride(1) != 1:
        raise RuntimeError("wgrad_own: the channel stride of both operands must be 1")
    if out is None:
        out = torch.empty(dy2.shape[1], x2.shape[1], device=dev, dtype=out_dtype or dy2.dtype)
    elif out.shape != (dy2.shape[1], x2.shape[1]) or out.stride(1) != 1 or out.dtype != (out_dtype or out.dtype):
        raise RuntimeError("wgrad_own: out must be (n, k) rows of out_dtype with channel stride 1")
    P = wgrad_block(dy2, x2, out_dtype, slabs, out, workspace)
    if workspace is None:
        ws = _lib.workspace("zigma_linear_wgrad", P, dev)
    _lib.call("zigma_linear_wgrad", P, dev)
    return out


def wgrad_workspace_bytes(m, n, k, dtype=torch.bfloat16, slabs=0):
    """bytes of workspace zigma_linear_wgrad asks for at this shape (0: one slab, the kernel writes the result itself)"""
    P = _lib.LinearWgradParams()
    P.m, P.n, P.k, P.slabs, P.dtype, P.out_dtype = m, n, k, int(slabs), _lib._DT[dtype], _lib._DT[dtype]
    return int(_lib.lib().zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)))


def wgrad(dy2, x2, out_dtype=None):
    """dy2 (m, n), x2 (m, k), same 16-bit dtype -> dy2^T x2 (n, k) in that dtype: the own split-K kernel where plan_wgrad says so, else the fp32
    sum of the library's slab products.  out_dtype=torch.float32 (the gradient of an fp32 weight under autocast): the same sums, delivered without the
    rounding to the operand type."""
    f32 = out_dtype == torch.float32 and dy2.dtype != torch.float32
    if plan_wgrad(dy2, x2) == "own":
        return wgrad_own(dy2, x2, out_dtype=torch.float32 if f32 else None)
    m, n = dy2.shape
    k = x2.shape[1]
    s = _slabs(m, n, k) if (SPLIT_WGRAD and dy2.is_cuda and dy2.dtype in (torch.bfloat16, torch.float16)) else 1
    if s <= 1 and f32:               # one product of the library with an fp32 result
        if _bmm_takes_out_dtype(dy2):
            return torch.bmm(dy2.t().unsqueeze(0), x2.unsqueeze(0), out_dtype=torch.float32)[0]
        return dy2.t().float() @ x2.float()
    if s <= 1:
        return dy2.t() @ x2
    dy3 = dy2.reshape(s, m // s, n)
    x3 = x2.reshape(s, m // s, k)
    # fp32 slab partials (one rounding at the end, like the single GEMM of the reference; a 16-bit partial could also overflow in fp16)
    if _bmm_takes_out_dtype(dy2):
        part = torch.bmm(dy3.transpose(1, 2), x3, out_dtype=torch.float32)
    else:                                  # (a torch without out_dtype on bmm)
        part = torch.bmm(dy3.transpose(1, 2), x3).float()
    return part.sum(0) if f32 else part.sum(0).to(dy2.dtype)


class LinearTrainFn(torch.autograd.Function):
    """F.linear whose weight gradient is formed slab-wise (see the module docstring); dX and dbias as autograd forms them.
    Mixed precision (a 16-bit x beside an fp32 weight under torch.autocast): the forward and dX read the weight's 16-bit shadow (zigma_amd/amp.py) — the
    shadow is what is saved —, dW and dbias are delivered in fp32 from the fp32 sums, and the backward runs with autocast off, as under the reference's
    custom_fwd / custom_bwd."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.amp = amp.mixed(x, weight)
        if ctx.amp:
            weight, bias = amp.operands(x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        r = plan("train", x, weight, bias)            # (autograd is off in here)
        return F.linear(x, weight, bias) if r.kernel == "library" else run(r, x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        if ctx.amp:
            with torch.autocast("cuda", enabled=False):
                return LinearTrainFn._backward(ctx, dy)
        return LinearTrainFn._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dyc = dy2 if dy2.is_contiguous() else dy2.contiguous()
            r = plan("train", dyc, _ContiguousLike(weight))        # dX = dY W = dY (W^T)^T: the same kernels on the transposed weight (a few MB)
            dx = (dy2 @ weight if r.kernel == "library" else run(r, dyc, weight.t().contiguous())).view(x.shape)
        if ctx.needs_input_grad[1]:
            dw = wgrad(dy2, x.reshape(-1, x.shape[-1]), out_dtype=torch.float32 if ctx.amp else None)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.sum(0, dtype=torch.float32) if ctx.amp else dy2.sum(0)
        return dx, dw, db


def linear_train(x, weight, bias=None):
    """differentiable projection of the training path: the slab-wise weight gradient where it pays (many tokens), F.linear otherwise.
    Under torch.autocast a 16-bit x beside an fp32 weight (amp.mixed) runs on the weight's shadow: LinearTrainFn at every token count when autograd records
    (the fp32 parameter receives an fp32 gradient), F.linear on the shadows otherwise."""
    if torch.is_autocast_enabled() and amp.mixed(x, weight) and (bias is None or bias.dtype == weight.dtype):
        if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
            return LinearTrainFn.apply(x, weight, bias)
        return F.linear(x, *amp.operands(x, weight, bias))
    if (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and weight.dtype == x.dtype and (bias is None or bias.dtype == x.dtype)
            and x.numel() // x.shape[-1] >= 4096 and torch.is_grad_enabled() and not torch.is_autocast_enabled()):
        return LinearTrainFn.apply(x, weight, bias)
    return F.linear(x, weight, bias)


_knobs.apply(globals(), "wgrad")
