"""fp32 projections on the bf16 matrix cores by splitting — what PyTorch calls float32_matmul_precision "high" (bfloat16_3x).

The reference's default model is fp32 and its sampler switches autocast off, so every checkpoint it ships samples in fp32.  gfx950 has no
xf32 MFMA and its fp32 matrix rate is 1/16 of the bf16 rate; an fp32 value is the sum of two bf16 values to 16 significant bits.

    split(a), a finite:      hi = bf16_rne(a), clamped to the largest finite bf16 (a finite a never becomes infinite);  lo = bf16_rne(a - float(hi))
    split(a), a non-finite:  hi = bf16(a), lo = 0
    "high":    y = sum_k (x_hi w_hi + x_lo w_hi + x_hi w_lo) + bias      three bf16 MFMA products, fp32 accumulators, lo x lo omitted
    "medium":  y = sum_k x_hi w_hi + bias                                the same kernel with one pass
    "highest": the library's fp32 GEMM, bit for bit what it always was — the default; none of this module's code is entered
At the ends of the range (include/zigma_hip.h): split(FLT_MAX) is hi = 0x7f7f, lo = 2^120, so "high" returns +inf for FLT_MAX under a unit
weight; an fp32 subnormal keeps about 7 bits (the planes' subnormal spacing is 2^-133).

The kernel is csrc/linear_split.hip (zigma_linear_f32_split): the weight planes are split once here (split_weight, cached against the
parameter's version counter — so a warmed-up forward holds no split and a hipGraph capture never captures one), x is split inside the kernel
on its way into LDS.  Which calls take it: linear.plan (the four block projections and the text rows of an fp32 model at inference; x_proj,
dt_proj, the adaLN / embedding / final-layer products and everything under autograd stay where they are).

Knob: PRECISION (ZIGMA_KNOBS="fp32_matmul.PRECISION=high"); public setters: zigma_amd.set_float32_matmul_precision / get_float32_matmul_precision.
torch's own global setting is not read."""
import weakref

import torch

from . import _knobs, _lib, amp

MODES = ("highest", "high", "medium")
PRECISION = "highest"
_PASSES = {"high": 3, "medium": 1}
ROUTE_KERNEL = {"high": "split3", "medium": "split1"}          # routing.KERNELS names of the two modes

_knobs.apply(globals(), "fp32_matmul")
if PRECISION not in MODES:
    raise RuntimeError(f"ZIGMA_KNOBS: fp32_matmul.PRECISION must be one of {MODES}, got {PRECISION!r}")


def set_float32_matmul_precision(mode):
    """ "highest" (default): fp32 projections run on the library's fp32 GEMM;  "high": on the bf16 matrix cores as three split products (about
    16 mantissa bits);  "medium": as one bf16 product.  Inference only; under autograd every mode is "highest"."""
    global PRECISION
    if mode not in MODES:
        raise ValueError(f"set_float32_matmul_precision: {mode!r} is none of {MODES}")
    PRECISION = mode


def get_float32_matmul_precision():
    return PRECISION


_MAX_BF16 = 3.3895313892515355e38          # 0x7f7f: the largest finite bf16


def split(t):
    """(hi, lo) bf16 tensors of an fp32 tensor by the definition above (CPU or GPU; torch's fp32 -> bf16 conversion rounds to nearest even)"""
    a = t.detach().to(torch.float32)
    finite = torch.isfinite(a)
    hi = torch.where(finite, a.clamp(-_MAX_BF16, _MAX_BF16), a).to(torch.bfloat16)
    lo = torch.where(finite, a - hi.float(), torch.zeros_like(a)).to(torch.bfloat16)
    return hi, lo


# ---- the weight planes: one cache entry per live weight ------------------------------------------------------------------------------------
_CACHE = {}                    # (device, data_ptr) -> (key, hi, lo, token)
CACHE_STATS = {"hit": 0, "miss": 0}
MAX_CACHE_ENTRIES = 4096       # backstop (weights that die drop their entry themselves): the oldest entries go first


def _drop(slot, token):
    hit = _CACHE.get(slot)
    if hit is not None and hit[3] is token:
        del _CACHE[slot]


def split_weight(w):
    """split(w) as contiguous (n, k) planes, cached on (data_ptr, _version, shape, stride, device) like Mamba._scan_consts: an in-place update of
    the parameter bumps its version and the next call splits again, replacing the stale entry (one slot per device address); the entry goes
    when the tensor object does."""
    slot = (str(w.device), w.data_ptr())
    key = (w.data_ptr(), w._version, tuple(w.shape), tuple(w.stride()), str(w.device), amp.step_count())      # (fused optimizers do not move _version)
    hit = _CACHE.get(slot)
    if hit is not None and hit[0] == key:
        CACHE_STATS["hit"] += 1
        return hit[1], hit[2]
    CACHE_STATS["miss"] += 1
    hi, lo = split(w)
    hi, lo = hi.contiguous(), lo.contiguous()
    token = object()
    _CACHE.pop(slot, None)                       # (re-inserted at the young end)
    _CACHE[slot] = (key, hi, lo, token)
    weakref.finalize(w, _drop, slot, token)
    while len(_CACHE) > MAX_CACHE_ENTRIES:
        del _CACHE[next(iter(_CACHE))]
    return hi, lo


def clear_cache():
    _CACHE.clear()


# ---- the call ----------------------------------------------------------------------------------------------------------------------------------
def linear_split_block(x, w_hi, w_lo, bias, out, passes):
    """The parameter block of zigma_linear_f32_split: x (m, k) fp32 rows one pitch apart or contiguous (..., k), the weight's bf16 planes (one pass reads
    w_hi only), out (m, n) fp32 rows (None: fresh contiguous rows, a placeholder address — a block to ask about).  Reads shapes, strides and
    addresses only, so descriptors (_lib.Desc) serve as well as tensors."""
    n, k = w_hi.shape[0], x.shape[-1]
    m = x.numel() // k
    if out is None:
        out = _lib.Desc.fresh(x, (m, n), 1)
    P = _lib.LinearSplitParams()
    P.m, P.n, P.k, P.passes, P.flags = m, n, k, passes, 0
    P.x_row_stride, P.w_hi_row_stride, P.w_lo_row_stride, P.out_row_stride = x.stride(-2), w_hi.stride(0), w_lo.stride(0), out.stride(-2)
    P.x, P.w_hi, P.w_lo, P.bias, P.out = _lib.ptr(x), _lib.ptr(w_hi), _lib.ptr(w_lo) if passes == 3 else None, _lib.ptr(bias), _lib.ptr(out)
    return P


def split_eligible(x, weight, bias=None):
    """zigma_linear_f32_split takes x @ weight.T (+ bias) on these tensors: what plan_linear_split() (csrc/linear_plan.h) serves with three passes on fresh
    contiguous planes of the weight (nothing is split or cached for the question), and what the block cannot say — fp32 throughout, on the device, a 2-D
    weight, unit channel strides, a > 2-D x that is one sequence of rows, no autograd"""
    f32 = torch.float32
    if not (x.is_cuda and weight.is_cuda and x.dtype == f32 and weight.dtype == f32 and len(weight.shape) == 2 and x.dim() >= 2):
        return False
    if bias is not None and not (bias.is_cuda and bias.dtype == f32 and bias.stride(0) == 1):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        return False
    if x.shape[-1] != weight.shape[1] or x.stride(-1) != 1 or (x.dim() > 2 and not x.is_contiguous()):
        return False
    w_hi, w_lo = (_lib.Desc.fresh(x, tuple(weight.shape), i, torch.bfloat16) for i in (2, 3))
    status, kernel = _lib.plan("zigma_linear_f32_split", linear_split_block(x, w_hi, w_lo, bias, None, 3))
    return status == 0 and kernel is not None


def linear_split(x, weight, bias=None, mode=None, out=None):
    """out = x @ weight.T (+ bias) in fp32 on the bf16 matrix cores: mode "high" (three split products) or "medium" (one); default: PRECISION.
    x (..., k) fp32 with unit channel stride (a 2-D x may be a view of wider rows), weight (n, k) fp32, out (..., n) fp32 rows (may be a view of
    wider rows).  Shapes and alignments outside the kernel's limits raise (there is no fallback in here — linear.plan decides before it calls)."""
    mode = PRECISION if mode is None else mode
    if mode not in _PASSES:
        raise ValueError(f"linear_split: mode must be 'high' or 'medium', got {mode!r}")
    dev = _lib.require_device(x, weight, bias, out)
    f32 = torch.float32
    if x.dtype != f32 or weight.dtype != f32 or (bias is not None and bias.dtype != f32) or (out is not None and out.dtype != f32):
        raise RuntimeError("linear_split: x, weight, bias and out must be float32")
    if weight.dim() != 2 or x.shape[-1] != weight.shape[1] or x.stride(-1) != 1 or (bias is not None and (bias.shape != (weight.shape[0],) or bias.stride(0) != 1)):
        raise RuntimeError("linear_split: x (..., k) with channel stride 1, weight (n, k), bias (n)")
    n, k = weight.shape
    lead = x.shape[:-1]
    x2 = x if x.dim() == 2 else x.reshape(-1, k)
    if out is None:
        out = torch.empty(x2.shape[0], n, device=x.device, dtype=f32)
    elif out.shape[-1] != n or out.stride(-1) != 1 or out.numel() != x2.shape[0] * n:
        raise RuntimeError("linear_split: out must be (..., n) float32 rows with channel stride 1")
    o2 = out if out.dim() == 2 else out.view(-1, n)
    w_hi, w_lo = split_weight(weight)
    _lib.call("zigma_linear_f32_split", linear_split_block(x2, w_hi, w_lo, bias, o2, _PASSES[mode]), dev)
    return out if out.dim() == len(lead) + 1 and out.shape[:-1] == lead else out.view(*lead, n)


def reference(x, w, bias=None, mode="high"):
    """the same arithmetic in torch, the bf16 products accumulated in float64 (CPU or GPU): what the kernel computes up to its fp32 accumulation"""
    if mode == "highest":
        y = x.double() @ w.double().t()
    else:
        xh, xl = (t.double() for t in split(x))
        wh, wl = (t.double() for t in split(w))
        y = xh @ wh.t()
        if mode == "high":
            y = y + (xl @ wh.t() + xh @ wl.t())
        elif mode != "medium":
            raise ValueError(f"reference: unknown mode {mode!r}")
    return y if bias is None else y + bias.double()
