"""LayerNorm (no affine weight) + adaLN modulate + projection in one kernel (zigma_norm_linear_fwd, csrc/norm_linear.hip): the pre-attention
`modulate(norm_msa(h), shift, scale)` of the block folded into CrossAttention.to_q (reference model_zigma.py:441-446, :104-128), so the modulated
LayerNorm output never reaches memory.  The library's own refusals are plan_norm_linear() (csrc/norm_linear_plan.h); norm_linear_shape_ok /
norm_linear_eligible restate them for shapes and tensors, and tests/test_norm_linear_cpu.py checks them against the compiled header.  Whether the
block takes the kernel is model_zigma.fuse_norm_to_q (knob FUSE_NORM_TO_Q)."""
import torch

from . import _lib

TILE = 128                     # rows per workgroup (kNlTile)
N_OUT = 512                    # output features (kNlN)
K_SERVED = (512, 640, 768)     # the instantiated row lengths
MFMA_DTYPES = (torch.bfloat16, torch.float16)


def norm_linear_shape_ok(m, n, k, rows_per_batch):
    """the shape limits of plan_norm_linear: n = 512, k of the instantiation set, whole 128-row tiles, whole samples"""
    return n == N_OUT and k in K_SERVED and m > 0 and m % TILE == 0 and m // TILE <= 0x7fffffff and rows_per_batch >= 1 and m % rows_per_batch == 0


def norm_linear_eligible(x, weight, shift, scale, bias=None):
    """limits of zigma_norm_linear_fwd on these tensors: (B, L, k) rows of one pitch, weight (512, k), shift / scale (B, k) rows of one pitch (column
    slices of a wider tensor pass), all bf16 or all fp16 on the device, 16-byte aligned rows, no bias, no autograd"""
    if bias is not None or x.dim() != 3 or weight.dim() != 2 or shift.dim() != 2 or scale.dim() != 2:
        return False
    if not (x.is_cuda and x.dtype in MFMA_DTYPES and weight.dtype == x.dtype and shift.dtype == x.dtype and scale.dtype == x.dtype):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or shift.requires_grad or scale.requires_grad):
        return False
    Bsz, L, k = x.shape
    n = weight.shape[0]
    if weight.shape[1] != k or shift.shape != (Bsz, k) or scale.shape != (Bsz, k) or not norm_linear_shape_ok(Bsz * L, n, k, L):
        return False
    if x.stride(2) != 1 or weight.stride(1) != 1 or shift.stride(1) != 1 or scale.stride(1) != 1 or x.stride(0) != L * x.stride(1):
        return False
    if shift.stride(0) != scale.stride(0) or shift.stride(0) < 0 or not (k <= x.stride(1) < 1 << 27) or not (k <= weight.stride(0) < 1 << 27):
        return False
    return all(s % 8 == 0 for s in (x.stride(1), weight.stride(0), shift.stride(0))) and all(t.data_ptr() % 16 == 0 for t in (x, weight, shift, scale))


def norm_linear(x, weight, shift, scale, eps, out=None):
    """out[b, l, :] = weight @ r16(r16(LN(x[b, l, :])) * (1 + scale[b]) + shift[b])   (r16: rounded to the I/O type; LN without affine weight, fp32 statistics).
    x: (B, L, k); weight: (n, k); shift / scale: (B, k); out: optional (B * L, n) view whose rows may be a column slice of a wider buffer."""
    dev = _lib.require_device(x, weight, shift, scale, out)
    Bsz, L, k = x.shape
    n = weight.shape[0]
    if out is None:
        out = torch.empty(Bsz * L, n, device=x.device, dtype=x.dtype)
    o2 = out if out.dim() == 2 else out.view(-1, n)
    P = _lib.NormLinearParams()
    P.m, P.n, P.k, P.dtype, P.flags, P.rows_per_batch, P.eps = Bsz * L, n, k, _lib.dtype_id(x), 0, L, float(eps)
    P.x_row_stride, P.w_row_stride, P.out_row_stride, P.mod_batch_stride = x.stride(1), weight.stride(0), o2.stride(0), shift.stride(0)
    P.x, P.w, P.shift, P.scale, P.out = _lib.ptr(x), _lib.ptr(weight), _lib.ptr(shift), _lib.ptr(scale), _lib.ptr(o2)
    _lib.call("zigma_norm_linear_fwd", P, dev)
    return out.view(Bsz, L, n) if out.dim() == 2 and out.is_contiguous() else out
