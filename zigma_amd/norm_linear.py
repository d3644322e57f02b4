"""LayerNorm (no affine weight) + adaLN modulate + projection in one kernel (zigma_norm_linear_fwd, csrc/norm_linear.hip): the pre-attention
`modulate(norm_msa(h), shift, scale)` of the block folded into CrossAttention.to_q (reference model_zigma.py:441-446, :104-128), so the modulated
LayerNorm output never reaches memory.  The library's own refusals are plan_norm_linear() (csrc/norm_linear_plan.h); norm_linear_shape_ok /
norm_linear_eligible build the block the launch would get (norm_linear_block) and ask it (zigma_norm_linear_fwd_plan).  Whether the
block takes the kernel is model_zigma.fuse_norm_to_q (knob FUSE_NORM_TO_Q)."""
import torch

from . import _lib


def norm_linear_block(x, weight, shift, scale, eps=0.0, out=None):
    """The parameter block of zigma_norm_linear_fwd: x (B, L, k) rows of all samples in one pitch, weight (n, k), shift / scale (B, k) rows of one pitch, out
    (B * L, n) rows (None: fresh contiguous rows, a placeholder address — a block to ask about).  Reads shapes, strides, dtypes and addresses only."""
    Bsz, L, k = x.shape
    n = weight.shape[0]
    if out is None:
        out = _lib.Desc.fresh(x, (Bsz * L, n), 1)
    P = _lib.NormLinearParams()
    P.m, P.n, P.k, P.dtype, P.flags, P.rows_per_batch, P.eps = Bsz * L, n, k, _lib.dtype_id(x), 0, L, float(eps)
    P.x_row_stride, P.w_row_stride, P.out_row_stride, P.mod_batch_stride = x.stride(1), weight.stride(0), out.stride(0), shift.stride(0)
    P.x, P.w, P.shift, P.scale, P.out = _lib.ptr(x), _lib.ptr(weight), _lib.ptr(shift), _lib.ptr(scale), _lib.ptr(out)
    return P


def _served(P):
    status, kernel = _lib.plan("zigma_norm_linear_fwd", P)
    return status == 0 and kernel is not None


def norm_linear_shape_ok(m, n, k, rows_per_batch):
    """plan_norm_linear serves this shape on aligned contiguous bf16 operands (shift / scale rows k apart) and a fresh output"""
    if rows_per_batch < 1 or m % rows_per_batch:
        return False            # (not (B, L, k) rows at all)
    x = _lib.Desc.fresh(None, (m // rows_per_batch, rows_per_batch, k), 2, torch.bfloat16)
    w, shift, scale = _lib.Desc.fresh(x, (n, k), 3), _lib.Desc.fresh(x, (m // rows_per_batch, k), 4), _lib.Desc.fresh(x, (m // rows_per_batch, k), 5)
    return _served(norm_linear_block(x, w, shift, scale))


def norm_linear_eligible(x, weight, shift, scale, bias=None):
    """zigma_norm_linear_fwd takes these tensors: what plan_norm_linear() serves, asked through the library, and what the block cannot say — (B, L, k) rows
    of all samples in one pitch, weight (n, k), shift / scale (B, k) rows of ONE pitch (column slices of a wider tensor pass), all of one dtype on the
    device, unit channel strides, no bias, no autograd"""
    if bias is not None or x.dim() != 3 or weight.dim() != 2 or shift.dim() != 2 or scale.dim() != 2:
        return False
    if not (x.is_cuda and x.dtype in _lib._DT and weight.dtype == x.dtype and shift.dtype == x.dtype and scale.dtype == x.dtype):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or shift.requires_grad or scale.requires_grad):
        return False
    Bsz, L, k = x.shape
    if weight.shape[1] != k or tuple(shift.shape) != (Bsz, k) or tuple(scale.shape) != (Bsz, k):
        return False
    if x.stride(2) != 1 or weight.stride(1) != 1 or shift.stride(1) != 1 or scale.stride(1) != 1 or x.stride(0) != L * x.stride(1) or shift.stride(0) != scale.stride(0):
        return False
    return _served(norm_linear_block(x, weight, shift, scale))


def norm_linear(x, weight, shift, scale, eps, out=None):
    """out[b, l, :] = weight @ r16(r16(LN(x[b, l, :])) * (1 + scale[b]) + shift[b])   (r16: rounded to the I/O type; LN without affine weight, fp32 statistics).
    x: (B, L, k); weight: (n, k); shift / scale: (B, k); out: optional (B * L, n) view whose rows may be a column slice of a wider buffer."""
    dev = _lib.require_device(x, weight, shift, scale, out)
    Bsz, L, k = x.shape
    n = weight.shape[0]
    if out is None:
        out = torch.empty(Bsz * L, n, device=x.device, dtype=x.dtype)
    o2 = out if out.dim() == 2 else out.view(-1, n)
    _lib.call("zigma_norm_linear_fwd", norm_linear_block(x, weight, shift, scale, eps, o2), dev)
    return out.view(Bsz, L, n) if out.dim() == 2 and out.is_contiguous() else out
