"""The small per-forward operators around the blocks on their own HIP kernels (csrc/embed.hip, csrc/skinny_linear.hip): patch
embedding + bias + position table, sinusoidal timestep features, the timestep MLP / adaLN modulation of all blocks (a few rows of
activations against up to 88 MB of weights), final LayerNorm + output projection.

Mirrors timm's PatchEmbed as ZigMa uses it (reference model_zigma.py:608-614,924,939-940), TimestepEmbedder (:232-275), the adaLN
`SiLU + Linear` of every Block (:441,447) and FinalLayer without conditioning (:313-337).  Inference only; anything the kernels do not take goes to the
torch composition in model_zigma.py.  The kernels' limits are the plans of csrc/outer_plan.h: every `*_eligible` builds the parameter block the launch would
get (`*_block`) and asks the library (_lib.served), and keeps only what a block cannot say — the device, one dtype across the operands, unit channel strides,
contiguity of operands the block has no pitch for, shapes that agree, no autograd, the knob.  A predicate that says yes returns its block; handed to the
wrapper (`block=`), the launch only sets the output's address.  No fallback inside the wrappers: a call outside the limits raises.
"""
import torch

from . import _lib

BF16 = torch.bfloat16
USE_EMBED_KERNELS = True      # False: the torch composition everywhere (A/B in tests and tools)
from . import _knobs  # noqa: E402
_knobs.apply(globals(), "embed")      # ZIGMA_KNOBS="embed.USE_EMBED_KERNELS=False" switches EVERY kernel of this module to torch (A/B tools)


def _same(x, *others):
    """the operands (None: absent) share x's dtype"""
    return all(t is None or t.dtype == x.dtype for t in others)


def _no_grad(*tensors):
    return not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors))


def _patch_embed_operands(x, weight, bias, pos):
    if not (x.dim() == 4 and weight.dim() == 4 and _same(x, weight, bias, pos) and x.stride(3) == 1 and weight.is_contiguous()):
        return False
    E, C, p, q = weight.shape
    if p != q or p < 1 or x.shape[1] != C or (bias is not None and not (bias.shape == (E,) and bias.is_contiguous())):
        return False
    return pos is None or (tuple(pos.shape[-2:]) == ((x.shape[2] // p) * (x.shape[3] // p), E) and pos.stride(-1) == 1)


def patch_embed_block(x, weight, bias=None, pos=None, out=None):
    """The parameter block of zigma_patch_embed_fwd: x (B, C, H, W), weight (E, C, p, p), bias (E), pos (1, L, E) or (L, E), out (B, L, E) (None: fresh
    contiguous rows, a placeholder address — a block to ask about).  Reads shapes, strides, dtypes and addresses only."""
    E, C, p, _ = weight.shape
    Bsz, _, H, W = x.shape
    if out is None:
        out = _lib.Desc.fresh(x, (Bsz, (H // p) * (W // p), E), 1)
    P = _lib.PatchEmbedParams()
    P.batch, P.in_chans, P.height, P.width, P.patch, P.embed_dim, P.dtype, P.flags = Bsz, C, H, W, p, E, _lib.dtype_id(x), 0
    P.x_batch_stride, P.x_chan_stride, P.x_row_stride = x.stride(0), x.stride(1), x.stride(2)
    P.out_batch_stride, P.out_row_stride = out.stride(0), out.stride(1)
    P.x, P.weight, P.bias, P.out = _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out)
    if pos is not None:
        P.pos, P.pos_row_stride = _lib.ptr(pos), pos.stride(-2)
    return P


def patch_embed_eligible(x, weight, bias, pos):
    if not (x.is_cuda and USE_EMBED_KERNELS and x.dtype in _lib._DT and _patch_embed_operands(x, weight, bias, pos)):
        return False
    P = patch_embed_block(x, weight, bias, pos)
    return _lib.served("zigma_patch_embed_fwd", P) and P


def patch_embed(x, weight, bias=None, pos=None, block=None):
    """x (B, C, H, W), weight (E, C, p, p), bias (E), pos (1, L, E) or (L, E) -> (B, L, E) = bf16(bf16(conv + bias) + pos).  block: what patch_embed_eligible
    returned for these operands."""
    dev = _lib.require_device(x, weight, bias, pos)
    if block is None:
        if not _patch_embed_operands(x, weight, bias, pos):
            raise RuntimeError("patch_embed: (B, C, H, W) input with unit stride along W, contiguous (E, C, p, p) weight and (E,) bias, (L, E) position rows, one dtype")
        block = patch_embed_block(x, weight, bias, pos)
    out = torch.empty(x.shape[0], (x.shape[2] // block.patch) * (x.shape[3] // block.patch), block.embed_dim, device=x.device, dtype=x.dtype)
    block.out = _lib.ptr(out)
    _lib.call("zigma_patch_embed_fwd", block, dev)
    return out


def _timestep_embed_operands(t, freqs):
    return t.dim() == 1 and t.is_contiguous() and freqs.dim() == 1 and freqs.is_contiguous() and _same(t, freqs) and freqs.device == t.device


def timestep_embed_block(t, freqs, dim, out=None):
    """The parameter block of zigma_timestep_embed_fwd: t (B,), freqs (dim // 2,), out (B, dim) (None: fresh rows, a placeholder address)"""
    if out is None:
        out = _lib.Desc.fresh(t, (t.shape[0], dim), 1)
    P = _lib.TimestepEmbedParams()
    P.batch, P.dim, P.dtype, P.flags, P.out_row_stride = t.shape[0], dim, _lib.dtype_id(t), 0, out.stride(0)
    P.t, P.freqs, P.out = _lib.ptr(t), _lib.ptr(freqs), _lib.ptr(out)
    return P


def timestep_embed_eligible(t, freqs):
    if not (t.is_cuda and USE_EMBED_KERNELS and t.dtype in _lib._DT and _timestep_embed_operands(t, freqs)):
        return False
    P = timestep_embed_block(t, freqs, 2 * freqs.shape[0])
    return _lib.served("zigma_timestep_embed_fwd", P) and P


def timestep_embed(t, freqs, dim, block=None):
    """t (B,) bf16, freqs (dim // 2,) bf16 -> (B, dim) bf16 = [cos(t f), sin(t f)] (products and functions in fp32)"""
    dev = _lib.require_device(t, freqs)
    if not _timestep_embed_operands(t, freqs) or freqs.shape[0] != dim // 2:
        raise RuntimeError("timestep_embed: contiguous t (B,) and freqs (dim // 2,) of one dtype on one device")
    if block is None or block.dim != dim:
        block = timestep_embed_block(t, freqs, dim)
    out = torch.empty(t.shape[0], dim, device=t.device, dtype=t.dtype)
    block.out = _lib.ptr(out)
    _lib.call("zigma_timestep_embed_fwd", block, dev)
    return out


def _skinny_linear_operands(x, weight, bias):
    if not (x.dim() == 2 and weight.dim() == 2 and _same(x, weight, bias) and weight.shape[1] == x.shape[1] and x.stride(1) == 1 and weight.stride(1) == 1):
        return False
    return bias is None or (bias.shape == (weight.shape[0],) and bias.is_contiguous())


def skinny_linear_block(x, weight, bias=None, silu=False, out=None):
    """The parameter block of zigma_skinny_linear_fwd: x (m, k) rows, weight (n, k) rows, bias (n), out (m, n) (None: fresh rows, a placeholder address)"""
    if out is None:
        out = _lib.Desc.fresh(x, (x.shape[0], weight.shape[0]), 1)
    P = _lib.SkinnyParams()
    P.m, P.n, P.k, P.dtype, P.flags = x.shape[0], weight.shape[0], x.shape[1], _lib.dtype_id(x), int(bool(silu))
    P.x_row_stride, P.w_row_stride, P.out_row_stride = x.stride(0), weight.stride(0), out.stride(0)
    P.x, P.w, P.bias, P.out = _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out)
    return P


def skinny_linear_eligible(x, weight, bias=None, silu=False):
    if not (x.is_cuda and USE_EMBED_KERNELS and x.dtype in _lib._DT and _skinny_linear_operands(x, weight, bias) and _no_grad(x, weight, bias)):
        return False
    P = skinny_linear_block(x, weight, bias, silu)
    return _lib.served("zigma_skinny_linear_fwd", P) and P


def skinny_linear(x, weight, bias=None, silu=False, block=None):
    """(m, k) @ (n, k)^T + bias for a few rows, optionally on silu(x) rounded to bf16 (the reference's `SiLU -> Linear` in bf16).  block: what
    skinny_linear_eligible returned for these operands and this `silu`."""
    dev = _lib.require_device(x, weight, bias)
    if block is None:
        if not (_skinny_linear_operands(x, weight, bias) and _no_grad(x, weight, bias)):
            raise RuntimeError("skinny_linear: (m, k) and (n, k) rows and an (n,) bias of one dtype, unit channel strides, no autograd")
        block = skinny_linear_block(x, weight, bias, silu)
    out = torch.empty(x.shape[0], weight.shape[0], device=x.device, dtype=x.dtype)
    block.out = _lib.ptr(out)
    _lib.call("zigma_skinny_linear_fwd", block, dev)
    return out


def _final_layer_operands(x, weight, bias):
    if not (weight.dim() == 2 and _same(x, weight, bias) and x.shape[-1] == weight.shape[1] and x.is_contiguous() and weight.is_contiguous()):
        return False
    return (bias is None or bias.is_contiguous()) and _no_grad(x, weight, bias)


def final_layer_block(x, weight, bias, eps, out=None):
    """The parameter block of zigma_final_layer_fwd: x (..., E) contiguous, weight (n_out, E), bias (n_out), out (rows, n_out) (None: fresh rows, a placeholder
    address)"""
    n_out, E = weight.shape
    rows = x.numel() // E if E else 0
    if out is None:
        out = _lib.Desc.fresh(x, (rows, n_out), 1)
    P = _lib.FinalLayerParams()
    P.rows, P.cols, P.n_out, P.dtype, P.flags, P.eps = rows, E, n_out, _lib.dtype_id(x), 0, float(eps)
    P.x_row_stride, P.out_row_stride = E, out.stride(0)
    P.x, P.weight, P.bias, P.out = _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out)
    return P


def final_layer_eligible(x, weight, bias, eps=0.0):
    if not (x.is_cuda and USE_EMBED_KERNELS and x.dtype in _lib._DT and _final_layer_operands(x, weight, bias)):
        return False
    P = final_layer_block(x, weight, bias, eps)
    return _lib.served("zigma_final_layer_fwd", P) and P


def final_layer(x, weight, bias, eps, block=None):
    """Linear(LayerNorm(x, no affine, eps)) for a projection to a few features: (..., E) -> (..., n_out).  block: what final_layer_eligible returned for these
    operands and this eps."""
    dev = _lib.require_device(x, weight, bias)
    if block is None:
        if not _final_layer_operands(x, weight, bias):
            raise RuntimeError("final_layer: contiguous (..., E) input, (n_out, E) weight and bias of one dtype, no autograd")
        block = final_layer_block(x, weight, bias, eps)
    out = torch.empty(block.rows, block.n_out, device=x.device, dtype=x.dtype)
    block.out = _lib.ptr(out)
    _lib.call("zigma_final_layer_fwd", block, dev)
    return out.view(*x.shape[:-1], block.n_out)


def _final_layer_guided_operands(x_pair, weight, bias, scale, grid, frames):
    """x_pair (2B, L, E): the conditional half first.  What final_layer takes, and: an even batch, L = max(frames, 1) * grid^2 tokens per sample (the output's
    shape), one fp32 scale per sample on the same device."""
    if x_pair.dim() != 3 or x_pair.shape[0] % 2 or not _final_layer_operands(x_pair, weight, bias) or x_pair.shape[1] != max(frames, 1) * grid * grid:
        return False
    return (torch.is_tensor(scale) and scale.is_cuda and scale.device == x_pair.device and scale.dtype == torch.float32
            and scale.shape == (x_pair.shape[0] // 2,) and scale.is_contiguous() and not scale.requires_grad)


def final_layer_cfg_block(x_pair, weight, bias, eps, scale, *, patch, chans, grid, frames=0, out_dtype=torch.float32, out=None):
    """The parameter block of zigma_final_layer_cfg_fwd: x_pair (2B, L, E) contiguous, scale (B,) fp32, out (B, [T,] C, H, W) of out_dtype (None: fresh, a
    placeholder address)"""
    Bsz, L, E = x_pair.shape[0] // 2, x_pair.shape[1], x_pair.shape[2]
    if out is None:
        out = _lib.Desc.fresh(x_pair, (Bsz,) + ((frames,) if frames else ()) + (chans, grid * patch, grid * patch), 1, out_dtype)
    P = _lib.FinalLayerCfgParams()
    P.rows, P.cols, P.n_out, P.dtype, P.out_dtype, P.flags, P.eps = Bsz * L, E, weight.shape[0], _lib.dtype_id(x_pair), _lib._DT.get(out_dtype, -1), 0, float(eps)
    P.rows_per_sample, P.tokens_per_frame, P.grid_w, P.patch, P.chans = L, grid * grid, grid, patch, chans
    P.x_row_stride = x_pair.stride(1)
    P.out_sample_stride, P.out_chan_stride, P.out_row_stride = out.stride(0), out.stride(-3), out.stride(-2)
    P.out_frame_stride = out.stride(1) if frames else 0
    P.x_cond, P.x_uncond = _lib.ptr(x_pair), _lib.ptr(x_pair) + Bsz * x_pair.stride(0) * x_pair.dtype.itemsize
    P.weight, P.bias, P.scale, P.out = _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(scale), _lib.ptr(out)
    return P


def final_layer_guided_eligible(x_pair, weight, bias, scale, *, patch, chans, grid, frames=0, out_dtype=torch.float32, eps=0.0):
    if not (x_pair.is_cuda and USE_EMBED_KERNELS and x_pair.dtype in _lib._DT and _final_layer_guided_operands(x_pair, weight, bias, scale, grid, frames)):
        return False
    P = final_layer_cfg_block(x_pair, weight, bias, eps, scale, patch=patch, chans=chans, grid=grid, frames=frames, out_dtype=out_dtype)
    return _lib.served("zigma_final_layer_cfg_fwd", P) and P


def final_layer_guided(x_pair, weight, bias, eps, scale, *, patch, chans, grid, frames=0, out_dtype=torch.float32, block=None):
    """Classifier-free guidance on the final layer's fp32 accumulators: x_pair (2B, L, E) = [conditional; unconditional] tokens ->
    v_u + scale * (v_c - v_u) with v = Linear(LayerNorm(x)), rounded ONCE to out_dtype and stored unpatchified:
    (B, C, H, W), or (B, T, C, H, W) with frames = T > 0.  scale: (B,) fp32 on the device.  block: what final_layer_guided_eligible returned for these
    operands, this geometry and this eps."""
    dev = _lib.require_device(x_pair, weight, bias, scale)
    if block is None:
        if not _final_layer_guided_operands(x_pair, weight, bias, scale, grid, frames):
            raise RuntimeError("final_layer_guided: contiguous (2B, L = frames * grid^2, E) input, (n_out, E) weight and bias of one dtype, (B,) fp32 scale on "
                               "the device, no autograd")
        block = final_layer_cfg_block(x_pair, weight, bias, eps, scale, patch=patch, chans=chans, grid=grid, frames=frames, out_dtype=out_dtype)
    side = grid * patch
    out = torch.empty((x_pair.shape[0] // 2,) + ((frames,) if frames else ()) + (chans, side, side), device=x_pair.device, dtype=out_dtype)
    block.out = _lib.ptr(out)
    _lib.call("zigma_final_layer_cfg_fwd", block, dev)
    return out
