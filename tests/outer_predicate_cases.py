"""Sweeps of the nine eligibility predicates that ask the library's plans about the operators around the blocks, cross-attention, the glue backward and the
weight gradient (embed.*_eligible, attention.cross_attn*_eligible, layernorm.glue_bwd_eligible, wgrad.own_serves) over the edges of every clause — dtype,
each size at its limit and one step past it, row pitches k / k + 4 / k + 8, addresses 2 and 8 bytes off, and every clause Python keeps for itself — and the
answer each point must get.

RECORDED holds the answers of the parent commit 631768e — the last one whose predicates restated the C limits by hand — on these same descriptors, one
character per point in the order of the sweep (`PYTHONPATH=<checkout> python tests/outer_predicate_cases.py` prints the tables of that checkout); they are
not taken from the code under test.  EXCEPTIONS lists, one by one, the points where the current predicates may answer differently; the only reason is that
the hand-written predicate said yes to a block the library refuses or answers as an empty call.  test_host_cpu.py runs the sweeps through the current code.
"""
import contextlib
import itertools

import torch

from zigma_amd import _lib

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF, F16, F32)
MAX_EXCEPTIONS = 0.02         # of the recorded points


class T(_lib.Desc):
    """a device tensor as the predicates read it (the package's descriptor, with a device); nothing is allocated.  pitch: elements between rows (the last but
    one dimension; outer dimensions stay dense over it); off: bytes the address lies off a 512-byte boundary; last: the channel stride"""

    def __init__(self, dtype, *shape, ptr=1, pitch=None, off=0, last=1, gap=0, cuda=True, grad=False, device=0):
        strides, n = [last], (pitch if pitch is not None else shape[-1] * last) if len(shape) > 1 else 0
        for d in reversed(shape[1:-1]):
            strides.append(n)
            n = n * d + gap
        if len(shape) > 1:
            strides.append(n)
        super().__init__(dtype, tuple(shape), tuple(reversed(strides)), (ptr << 36) + off, cuda, grad)
        self.device = torch.device("cuda", device) if cuda else torch.device("cpu")


def _other(dt):
    return F16 if dt != F16 else BF


def _points(axes, variants):
    """the product of the axes, each with every variant: (values of the axes..., variant)"""
    return itertools.product(*axes, variants)


# Every sweep yields (point, args, kwargs, policy, kernels): the predicate's operands, the clauses Python keeps for itself that fail at this point
# ({name: fails}), and the kernels a yes may be served by.
def sweep_patch_embed():
    variants = ("base", "cpu", "x_stride_2", "w_loose", "w_off2", "w_off8", "chans_mismatch", "height_9", "no_bias", "bias_other_dtype", "bias_loose", "bias_off2",
                "bias_off8", "no_pos", "pos_other_dtype", "pos_rows", "pos_stride_2", "pos_pitch+4", "pos_pitch+8", "pos_off2", "pos_off8")
    for dt, E, B, v in _points((DTYPES, (8, 12, 64, 1024, 1032), (0, 1, 65535, 65536)), variants):
        x = T(dt, B, 4, 9 if v == "height_9" else 8, 8, ptr=1, last=2 if v == "x_stride_2" else 1, cuda=v != "cpu")
        w = T(dt, E, 5 if v == "chans_mismatch" else 4, 2, 2, ptr=2, off={"w_off2": 2, "w_off8": 8}.get(v, 0), gap=4 if v == "w_loose" else 0)
        bias = None if v == "no_bias" else T(_other(dt) if v == "bias_other_dtype" else dt, E, ptr=3, off={"bias_off2": 2, "bias_off8": 8}.get(v, 0),
                                            last=2 if v == "bias_loose" else 1)
        pos = None if v == "no_pos" else T(_other(dt) if v == "pos_other_dtype" else dt, 1, 15 if v == "pos_rows" else 16, E, ptr=4,
                                          pitch={"pos_pitch+4": E + 4, "pos_pitch+8": E + 8, "pos_stride_2": 2 * E}.get(v), last=2 if v == "pos_stride_2" else 1,
                                          off={"pos_off2": 2, "pos_off8": 8}.get(v, 0))
        policy = {"on the device": v == "cpu", "one dtype": v in ("bias_other_dtype", "pos_other_dtype"), "unit channel strides": v in ("x_stride_2", "pos_stride_2"),
                  "contiguous": v in ("w_loose", "bias_loose"), "shapes agree": v in ("chans_mismatch", "pos_rows")}
        yield (str(dt), E, B, v), (x, w, bias, pos), {}, policy, ("patch_embed",)


def sweep_timestep_embed():
    variants = ("base", "cpu", "t_loose", "freqs_loose", "freqs_other_dtype", "t_2d", "other_device")
    for dt, B, half, v in _points((DTYPES, (0, 1, 7), (0, 1, 4)), variants):
        t = T(dt, *((B, 1) if v == "t_2d" else (B,)), ptr=1, last=2 if v == "t_loose" else 1, cuda=v != "cpu")
        f = T(_other(dt) if v == "freqs_other_dtype" else dt, half, ptr=2, last=2 if v == "freqs_loose" else 1, cuda=v != "cpu", device=1 if v == "other_device" else 0)
        policy = {"on the device": v == "cpu", "one dtype": v == "freqs_other_dtype", "contiguous": v in ("t_loose", "freqs_loose"), "shapes agree": v == "t_2d",
                  "one device": v == "other_device"}
        yield (str(dt), B, half, v), (t, f), {}, policy, ("timestep_embed",)


def sweep_skinny_linear():
    variants = ("base", "cpu", "x_pitch+4", "x_pitch+8", "w_pitch+4", "w_pitch+8", "x_off2", "x_off8", "w_off2", "w_off8", "no_bias", "bias_off2", "bias_off4",
                "bias_off8", "bias_other_dtype", "bias_rows", "bias_loose", "x_stride_2", "w_stride_2", "k_mismatch", "grad")
    for dt, m, n, k, v in _points((DTYPES, (0, 1, 64, 65), (16, 24, 32), (128, 192, 1024, 1152)), variants):
        x = T(dt, m, k, ptr=1, pitch={"x_pitch+4": k + 4, "x_pitch+8": k + 8, "x_stride_2": 2 * k}.get(v), off={"x_off2": 2, "x_off8": 8}.get(v, 0),
              last=2 if v == "x_stride_2" else 1, cuda=v != "cpu")
        kw = k + 128 if v == "k_mismatch" else k
        w = T(dt, n, kw, ptr=2, pitch={"w_pitch+4": kw + 4, "w_pitch+8": kw + 8, "w_stride_2": 2 * kw}.get(v), off={"w_off2": 2, "w_off8": 8}.get(v, 0),
              last=2 if v == "w_stride_2" else 1, grad=v == "grad")
        bias = None if v == "no_bias" else T(_other(dt) if v == "bias_other_dtype" else dt, n + 16 if v == "bias_rows" else n, ptr=3,
                                            off={"bias_off2": 2, "bias_off4": 4, "bias_off8": 8}.get(v, 0), last=2 if v == "bias_loose" else 1)
        policy = {"on the device": v == "cpu", "one dtype": v == "bias_other_dtype", "unit channel strides": v in ("x_stride_2", "w_stride_2"),
                  "contiguous": v == "bias_loose", "shapes agree": v in ("k_mismatch", "bias_rows"), "no autograd": v == "grad"}
        yield (str(dt), m, n, k, v), (x, w, bias), {}, policy, ("skinny_linear_mfma",)


def sweep_final_layer():
    variants = ("base", "cpu", "x_loose", "x_off2", "x_off8", "w_loose", "w_off2", "w_off8", "cols_mismatch", "no_bias", "bias_other_dtype", "bias_loose", "grad")
    for dt, E, n_out, rows, v in _points((DTYPES, (8, 12, 2048, 2056), (1, 16, 17), (0, 5)), variants):
        x = T(dt, rows, E, ptr=1, pitch=E + 8 if v == "x_loose" else None, off={"x_off2": 2, "x_off8": 8}.get(v, 0), cuda=v != "cpu")
        Ew = E + 8 if v == "cols_mismatch" else E
        w = T(dt, n_out, Ew, ptr=2, pitch=Ew + 8 if v == "w_loose" else None, off={"w_off2": 2, "w_off8": 8}.get(v, 0), grad=v == "grad")
        bias = None if v == "no_bias" else T(_other(dt) if v == "bias_other_dtype" else dt, n_out, ptr=3, last=2 if v == "bias_loose" else 1)
        policy = {"on the device": v == "cpu", "one dtype": v == "bias_other_dtype", "contiguous": v in ("x_loose", "w_loose", "bias_loose"),
                  "shapes agree": v == "cols_mismatch", "no autograd": v == "grad"}
        yield (str(dt), E, n_out, rows, v), (x, w, bias), {}, policy, ("final_layer",)


def sweep_final_layer_guided():
    variants = ("base", "cpu", "odd_batch", "tokens_mismatch", "n_out_mismatch", "out_bf16", "out_f16", "scale_float", "scale_cpu", "scale_f16", "scale_rows",
                "scale_loose", "scale_grad", "scale_other_device", "x_off8", "bias_other_dtype")
    geometries = ((1, 3, 2, 0), (2, 4, 2, 0), (1, 17, 2, 0), (1, 3, 2, 2), (1, 3, 0, 0))      # patch, chans, grid, frames
    for dt, E, (p, ch, grid, frames), v in _points((DTYPES, (64, 2048, 2056), geometries), variants):
        L = max(frames, 1) * grid * grid * (2 if v == "tokens_mismatch" else 1)         # (twice the frames the output has room for)
        x = T(dt, 3 if v == "odd_batch" else 4, L, E, ptr=1, off=8 if v == "x_off8" else 0, cuda=v != "cpu")
        w = T(dt, p * p * ch + (v == "n_out_mismatch"), E, ptr=2)
        bias = T(_other(dt) if v == "bias_other_dtype" else dt, w.shape[0], ptr=3)
        scale = 4.0 if v == "scale_float" else T(F16 if v == "scale_f16" else F32, 3 if v == "scale_rows" else 2, ptr=4, last=2 if v == "scale_loose" else 1,
                                                 cuda=v not in ("cpu", "scale_cpu"), grad=v == "scale_grad", device=1 if v == "scale_other_device" else 0)
        kwargs = dict(patch=p, chans=ch, grid=grid, frames=frames, **({"out_dtype": {"out_bf16": BF, "out_f16": F16}[v]} if v.startswith("out_") else {}))
        policy = {"on the device": v == "cpu", "one dtype": v == "bias_other_dtype", "an even batch": v == "odd_batch",
                  "the tokens of the output": v == "tokens_mismatch" or grid < 1,
                  "an fp32 scale per sample on the device": v in ("scale_float", "scale_cpu", "scale_f16", "scale_rows", "scale_loose", "scale_grad", "scale_other_device")}
        yield (str(dt), E, p, ch, grid, frames, v), (x, w, bias, scale), kwargs, policy, ("final_layer_cfg",)


def _sweep_cross_attn(kernel):
    variants = ("base", "cpu", "batch_0", "tokens_0", "batch_65535", "batch_65536", "heads_65535", "heads_65536", "head_dim_32", "q_pitch+4", "q_pitch+8", "k_pitch+4",
                "k_pitch+8", "v_pitch+4", "v_pitch+8", "q_off2", "q_off8", "k_off2", "k_off8", "v_off2", "v_off8", "q_batch_gap_4", "q_stride_2", "k_other_dtype",
                "v_rows", "batch_mismatch", "width_mismatch")
    for dt, n, v in _points((DTYPES, (0, 1, 128, 129)), variants):
        B = {"batch_0": 0, "batch_65535": 65535, "batch_65536": 65536}.get(v, 2)
        H = {"heads_65535": 65535, "heads_65536": 65536}.get(v, 2)
        C, L = H * (32 if v == "head_dim_32" else 64), 0 if v == "tokens_0" else 33
        big = B > 2          # (one sample broadcast over the batch: the addresses stay small)

        def rows(name, ptr, r, cols=C, dtype=dt, Bsz=B):
            t = T(dtype, Bsz, r, cols, ptr=ptr, pitch={name + "_pitch+4": cols + 4, name + "_pitch+8": cols + 8, name + "_stride_2": 2 * cols}.get(v),
                  off={name + "_off2": 2, name + "_off8": 8}.get(v, 0), last=2 if v == name + "_stride_2" else 1, gap=4 if v == name + "_batch_gap_4" else 0,
                  cuda=v != "cpu")
            if big:
                t.strides = (0,) + t.strides[1:]
            return t
        q, k = rows("q", 1, L), rows("k", 2, n, dtype=_other(dt) if v == "k_other_dtype" else dt, Bsz=B + (v == "batch_mismatch"))
        vv = rows("v", 3, n + (v == "v_rows"), Bsz=B + (v == "batch_mismatch"))
        if v == "width_mismatch":
            k, vv = rows("k", 2, n, cols=C + 64), rows("v", 3, n, cols=C + 64)
        policy = {"on the device": v == "cpu", "one dtype": v == "k_other_dtype", "unit channel strides": v == "q_stride_2",
                  "shapes agree": v in ("v_rows", "batch_mismatch", "width_mismatch")}
        yield (str(dt), n, v), (q, k, vv, H), {}, policy, (kernel,)


def sweep_cross_attn():
    return _sweep_cross_attn("cross_attn_mfma")


def sweep_cross_attn_bwd():
    return _sweep_cross_attn("cross_attn_bwd_mfma")


def sweep_glue_bwd():
    variants = ("base", "cpu", "dy_pitch+4", "dy_pitch+8", "a_pitch+4", "a_pitch+8", "dy_off2", "dy_off8", "a_off2", "a_off8", "s_off2", "s_off8", "s_pitch+4",
                "s_pitch+8", "dy_stride_2", "a_rows", "a_other_dtype", "s_other_dtype", "s_rows", "s_stride_2", "dy_batch_gap_8")
    for dt, L, B, E, v in _points((DTYPES, (64, 100, 128), (1, 2), (128, 192, 8192, 8320)), variants):
        def rows(name, ptr, r=L, dtype=dt):
            return T(dtype, B, r, E, ptr=ptr, pitch={name + "_pitch+4": E + 4, name + "_pitch+8": E + 8, name + "_stride_2": 2 * E}.get(v),
                     off={name + "_off2": 2, name + "_off8": 8}.get(v, 0), last=2 if v == name + "_stride_2" else 1, gap=8 if v == name + "_batch_gap_8" else 0,
                     cuda=v != "cpu")
        dy, a = rows("dy", 1), rows("a", 2, L + (v == "a_rows"), _other(dt) if v == "a_other_dtype" else dt)
        s = T(_other(dt) if v == "s_other_dtype" else dt, B + (v == "s_rows"), E, ptr=3, pitch={"s_pitch+4": E + 4, "s_pitch+8": E + 8, "s_stride_2": 2 * E}.get(v),
              off={"s_off2": 2, "s_off8": 8}.get(v, 0), last=2 if v == "s_stride_2" else 1)
        policy = {"on the device": v == "cpu", "one dtype": v in ("a_other_dtype", "s_other_dtype"), "unit channel strides": v in ("dy_stride_2", "s_stride_2"),
                  "shapes agree": v in ("a_rows", "s_rows"), "samples in one pitch": v == "dy_batch_gap_8"}
        yield (str(dt), L, B, E, v), (dy, a, s), {}, policy, ("scale_reduce_bwd",)


def sweep_own_serves():
    variants = ("base", "cpu", "dy_pitch+4", "dy_pitch+8", "x_pitch+4", "x_pitch+8", "dy_pitch-8", "dy_off2", "dy_off8", "x_off2", "x_off8", "dy_stride_2", "x_stride_2",
                "rows_mismatch", "x_other_dtype", "x_3d")
    sizes = (4, 8, 12, 8192, 8200)
    for dt, m, n, k, v in _points((DTYPES, (0, 1, 512), sizes, sizes), variants):
        def rows(name, ptr, r, cols, dtype=dt):
            return T(dtype, r, cols, ptr=ptr, pitch={name + "_pitch+4": cols + 4, name + "_pitch+8": cols + 8, name + "_pitch-8": cols - 8, name + "_stride_2": 2 * cols}.get(v),
                     off={name + "_off2": 2, name + "_off8": 8}.get(v, 0), last=2 if v == name + "_stride_2" else 1, cuda=v != "cpu")
        dy, x = rows("dy", 1, m, n), rows("x", 2, m + (v == "rows_mismatch"), k, _other(dt) if v == "x_other_dtype" else dt)
        if v == "x_3d":
            x = T(dt, 1, m, k, ptr=2)
        policy = {"on the device": v == "cpu", "unit channel strides": v in ("dy_stride_2", "x_stride_2"), "shapes agree": v in ("rows_mismatch", "x_3d")}
        kernels = tuple(f"wgrad_128x{bk}{sk}" for bk in (64, 128) for sk in ("", "_splitk"))
        yield (str(dt), m, n, k, v), (dy, x), {}, policy, kernels


# predicate: (module, name of the predicate, name of the block builder, entry point, sweep)
SWEEPS = {
    "patch_embed": ("embed", "patch_embed_eligible", "patch_embed_block", "zigma_patch_embed_fwd", sweep_patch_embed),
    "timestep_embed": ("embed", "timestep_embed_eligible", "timestep_embed_block", "zigma_timestep_embed_fwd", sweep_timestep_embed),
    "skinny_linear": ("embed", "skinny_linear_eligible", "skinny_linear_block", "zigma_skinny_linear_fwd", sweep_skinny_linear),
    "final_layer": ("embed", "final_layer_eligible", "final_layer_block", "zigma_final_layer_fwd", sweep_final_layer),
    "final_layer_guided": ("embed", "final_layer_guided_eligible", "final_layer_cfg_block", "zigma_final_layer_cfg_fwd", sweep_final_layer_guided),
    "cross_attn": ("attention", "cross_attn_eligible", "cross_attn_block", "zigma_cross_attn_fwd", sweep_cross_attn),
    "cross_attn_bwd": ("attention", "cross_attn_bwd_eligible", "cross_attn_bwd_block", "zigma_cross_attn_bwd", sweep_cross_attn_bwd),
    "glue_bwd": ("layernorm", "glue_bwd_eligible", "glue_bwd_block", "zigma_scale_reduce_bwd", sweep_glue_bwd),
    "own_serves": ("wgrad", "own_serves", "wgrad_block", "zigma_linear_wgrad", sweep_own_serves),
}


@contextlib.contextmanager
def descriptors_as_tensors():
    """torch.is_tensor says yes to a descriptor (the guided final layer asks it of its scale), autograd is off"""
    real = torch.is_tensor
    torch.is_tensor = lambda t: isinstance(t, _lib.Desc) or real(t)
    try:
        with torch.no_grad():
            yield
    finally:
        torch.is_tensor = real


def answers(which):
    """the predicate's verdict on every point of its sweep, as booleans in the sweep's order (grad mode on at the points that ask about autograd)"""
    import importlib
    module, predicate, _, _, sweep = SWEEPS[which]
    fn = getattr(importlib.import_module("zigma_amd." + module), predicate)
    out = []
    with descriptors_as_tensors():
        for point, args, kwargs, _, _ in sweep():
            with torch.set_grad_enabled(point[-1] == "grad"):
                out.append(bool(fn(*args, **kwargs)))
    return out


def block_args(which, args, kwargs):
    """the block builder's arguments for a point of the sweep (the predicates that take fewer operands than their builders)"""
    if which == "timestep_embed":
        return (*args, 2 * args[1].shape[0]), kwargs
    if which == "final_layer":
        return (*args, 0.0), kwargs
    if which == "final_layer_guided":          # (a Python float for a scale has no address: the block of the same call with a scale tensor)
        return (*args[:3], 0.0, args[3] if isinstance(args[3], T) else T(F32, 2, ptr=4)), kwargs
    if which == "cross_attn_bwd":
        return (*args[:3], T(args[0].dtype, *args[0].shape, ptr=5), args[3]), kwargs
    return args, kwargs


def pack(bits):
    return "".join("01"[b] for b in bits)


# ---- recorded on the parent commit (see the module docstring) -------------------------------------------------------------------------------
RECORDED = {
    "patch_embed": (
        "1000000010000100001001000000010000100001001000000010000100001000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000010000000100001000010010000000100001000010010000000100001000010000000000000000000000010000000100001000010010000000100001000010010000000100001000010000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "00000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
    ),
    "timestep_embed": (
        "1000000100100010000001010000101100010100001000000100100010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "00000000000000000000000000000"
    ),
    "skinny_linear": (
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000010010100001001000000000000000000000000000010010100001001000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000100101000010010000000000000000000000000000100101000010010000"
        "0000000000000000000000001001010000100100000000000000000000000000001001010000100100000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000010010100001001000000000000000000000000000010010100001001000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
    ),
    "final_layer": (
        "1000010001010100001000101010000000010001000000001000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001000"
        "0100010101000010001010100000000100010000000010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
    ),
    "final_layer_guided": (
        "1000010000000000100001000000000000000000000000001000010000000000000000000000000010000100000000001000010000000000000000000000000010000100000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "00000000000000000000000000000000000000000000000000000000000000000000000000000000"
    ),
    "cross_attn": (
        "0000000000000000000000000001011101000101010000000000001011101000101010000000000000000000000000000000000000000000000000000000000000000001011101000101010000000000"
        "0010111010001010100000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000"
    ),
    "cross_attn_bwd": (
        "0000000000000000000000000001011101000101010000000000001011101000101010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000"
    ),
    "glue_bwd": (
        "1001010000000100000000000000000000000000001001010000000100000000000000000000000000001001010000000100000000000000000000000000001001010000000100000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000100101000000010000000000000000000000000000100101000000010000000000000000000000000000100101000000010000000000000000000000000000100101000000010000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "000000000000000000000000000000000000000000000000000000000000000000000000"
    ),
    "own_serves": (
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000100101000000000000000000000000001001010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000100101000000000000000000000000001001010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001001010000000000000000000000000010010100000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001001010000000000000000000000000010010100000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001001010000000000000000000000000010010100000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001001010000000000000000000000000010010100000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000100101000000000000000000000000001001010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000100101000000000000000000000000001001010000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "00000000000000000000000000000000000000000000000000000000000000000000000000000000"
    ),
}
# (predicate, point): reason — the parent's predicate said yes here; the library does not launch this block
EXCEPTIONS = {
    ("patch_embed", ('torch.bfloat16', 8, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 8, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 8, 0, 'no_pos')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 8, 0, 'pos_pitch+8')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 64, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 64, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 64, 0, 'no_pos')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 64, 0, 'pos_pitch+8')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 1024, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 1024, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 1024, 0, 'no_pos')): "an empty call (status 0, nothing launched)",
    ("patch_embed", ('torch.bfloat16', 1024, 0, 'pos_pitch+8')): "an empty call (status 0, nothing launched)",
    ("timestep_embed", ('torch.bfloat16', 0, 0, 'base')): "refused by the library (status -2)",
    ("timestep_embed", ('torch.bfloat16', 0, 1, 'base')): "an empty call (status 0, nothing launched)",
    ("timestep_embed", ('torch.bfloat16', 0, 1, 'freqs_loose')): "an empty call (status 0, nothing launched)",
    ("timestep_embed", ('torch.bfloat16', 0, 4, 'base')): "an empty call (status 0, nothing launched)",
    ("timestep_embed", ('torch.bfloat16', 1, 0, 'base')): "refused by the library (status -2)",
    ("timestep_embed", ('torch.bfloat16', 1, 0, 't_loose')): "refused by the library (status -2)",
    ("timestep_embed", ('torch.bfloat16', 7, 0, 'base')): "refused by the library (status -2)",
    ("final_layer", ('torch.bfloat16', 8, 1, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 8, 1, 0, 'w_loose')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 8, 1, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 8, 1, 0, 'bias_loose')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 8, 16, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 8, 16, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 2048, 1, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 2048, 1, 0, 'w_loose')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 2048, 1, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 2048, 1, 0, 'bias_loose')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 2048, 16, 0, 'base')): "an empty call (status 0, nothing launched)",
    ("final_layer", ('torch.bfloat16', 2048, 16, 0, 'no_bias')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.bfloat16', 1, 'batch_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.bfloat16', 1, 'tokens_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.bfloat16', 128, 'batch_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.bfloat16', 128, 'tokens_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.float16', 1, 'batch_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.float16', 1, 'tokens_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.float16', 128, 'batch_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn", ('torch.float16', 128, 'tokens_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn_bwd", ('torch.bfloat16', 1, 'batch_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn_bwd", ('torch.bfloat16', 1, 'tokens_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn_bwd", ('torch.bfloat16', 128, 'batch_0')): "an empty call (status 0, nothing launched)",
    ("cross_attn_bwd", ('torch.bfloat16', 128, 'tokens_0')): "an empty call (status 0, nothing launched)",
}

if __name__ == "__main__":
    import textwrap
    print("RECORDED = {")
    for name in SWEEPS:
        print(f'    "{name}": (')
        for ln in textwrap.wrap(pack(answers(name)), 160):
            print(f'        "{ln}"')
        print("    ),")
    print("}")
