"""linear.plan calls on descriptors of the shipped projection shapes and their edges, and the Route each must give; the verdicts of
gated_residual_eligible, norm_linear_eligible and split_eligible on the edges of their rules.

The expected routes and verdicts were RECORDED by running the parent commit 01f10da — the last one whose predicates restated the C limits by hand —
on these same descriptors (`PYTHONPATH=<checkout> python tests/linear_route_cases.py` prints the tables of that checkout); they are not taken from
the code under test.  test_linear_route_cases.py runs the tables through the current code, whose predicates ask the built library.
"""
import contextlib
import math

import torch

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PTR = dict(x=1 << 30, w=1 << 36, bias=1 << 42, residual=1 << 44, gate=1 << 45, shift=1 << 46, scale=(1 << 46) + (1 << 20))


class T:
    """a device tensor as the planning predicates read it (shape, strides, dtype, address); nothing is allocated"""

    def __init__(self, dtype, shape, strides=None, ptr=1 << 30, is_cuda=True, requires_grad=False):
        self.dtype, self.shape, self._ptr, self.is_cuda, self.requires_grad = dtype, tuple(shape), ptr, is_cuda, requires_grad
        self.device = torch.device("cuda", 0) if is_cuda else torch.device("cpu")
        self._strides = tuple(strides) if strides else tuple(math.prod(shape[i + 1:]) for i in range(len(shape)))

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return math.prod(self.shape)

    def is_contiguous(self):
        return self._strides == tuple(math.prod(self.shape[i + 1:]) for i in range(len(self.shape)))


def shapes(E):
    """role -> (n, k, bias, gated residual) of a model of width E"""
    return {"in_proj": (4 * E, E, False, False), "out_proj": (E, 2 * E, False, True), "to_q": (512, E, False, False), "to_out": (E, 512, True, True),
            "text": (2 * 512, E, True, False), "train": (4 * E, E, False, False)}


def _case(role, n, k, tokens, dtype=BF, w_dtype=None, bias=None, x="3d", x_pitch=0, res=None, gate_off=0, gate_pitch=0, grad=False, w_grad=False, x_grad=False,
          autocast=None, precision="highest", policy="auto", disabled="", transposed=False, cuda=True):
    """bias: None or the byte offset of its address from a 16-byte boundary;  x: "3d" (B, 1024, k) contiguous | "2d" rows of pitch k + x_pitch | "3d_nc" (B, 1024,
    k) with rows of pitch k + x_pitch;  res: None | "ok" | "misaligned" (8 bytes off) | "pitch" (rows of n + 8) | "batch_pitch" (samples not in one row sequence)
    | "odd_pitch" (rows of n + 4);  gate_off / gate_pitch: bytes off a 16-byte boundary / extra elements per gate row;  transposed: the weight is wgrad's stand-in of
    weight.t().contiguous() of an (k, n) parameter"""
    return dict(role=role, n=n, k=k, tokens=tokens, dtype=dtype, w_dtype=w_dtype or dtype, bias=bias, x=x, x_pitch=x_pitch, res=res, gate_off=gate_off,
                gate_pitch=gate_pitch, grad=grad, w_grad=w_grad, x_grad=x_grad, autocast=autocast, precision=precision, policy=policy, disabled=disabled,
                transposed=transposed, cuda=cuda)


CASES = {}
TOKENS = (2048, 4096, 8192, 16384, 32768, 65536, 131072)
for _E in (512, 640, 768, 1024):
    for _role, (_n, _k, _b, _r) in shapes(_E).items():
        for _t in TOKENS:
            CASES[f"{_role}_E{_E}_t{_t}"] = _case(_role, _n, _k, _t, bias=0 if _b else None, res="ok" if _r else None, x="2d" if _role in ("text", "train") else "3d")
for _t in (8192, 65536):
    for _off in (None, 0, 8, 4, 2):
        CASES[f"to_out_E640_t{_t}_bias_{_off}"] = _case("to_out", 640, 512, _t, bias=_off, res="ok")
        CASES[f"text_E640_t{_t}_bias_{_off}"] = _case("text", 1024, 640, _t, bias=_off, x="2d")
        CASES[f"in_proj_E640_t{_t}_bias_{_off}"] = _case("in_proj", 2560, 640, _t, bias=_off)
    CASES[f"to_out_n8192_t{_t}_bias"] = _case("to_out", 8192, 512, _t, bias=0, res="ok")        # (a bias vector beyond the 8-wave kernel's 8 KB of LDS)
for _role, _n, _k in (("in_proj", 2560, 640), ("out_proj", 640, 1280), ("to_q", 512, 640), ("train", 2560, 640), ("train", 640, 1280)):
    for _t in (8192, 16384, 65536):
        for _p in (4, 8, 128):
            CASES[f"{_role}_k{_k}_t{_t}_2d_pitch+{_p}"] = _case(_role, _n, _k, _t, x="2d", x_pitch=_p)
        CASES[f"{_role}_k{_k}_t{_t}_2d"] = _case(_role, _n, _k, _t, x="2d")
        CASES[f"{_role}_k{_k}_t{_t}_3d_nc"] = _case(_role, _n, _k, _t, x="3d_nc", x_pitch=128)
for _role, _n, _k, _b in (("out_proj", 640, 1280, None), ("to_out", 640, 512, 0), ("out_proj", 768, 1536, None)):
    for _t in (8192, 16384, 65536):
        for _res in ("misaligned", "pitch", "batch_pitch", "odd_pitch"):
            CASES[f"{_role}_n{_n}_t{_t}_res_{_res}"] = _case(_role, _n, _k, _t, bias=_b, res=_res)
        CASES[f"{_role}_n{_n}_t{_t}_gate_misaligned"] = _case(_role, _n, _k, _t, bias=_b, res="ok", gate_off=8)
        CASES[f"{_role}_n{_n}_t{_t}_gate_pitch+4"] = _case(_role, _n, _k, _t, bias=_b, res="ok", gate_pitch=4)
        CASES[f"{_role}_n{_n}_t{_t}_gate_pitch+8"] = _case(_role, _n, _k, _t, bias=_b, res="ok", gate_pitch=8)
        CASES[f"{_role}_n{_n}_t{_t}_no_residual"] = _case(_role, _n, _k, _t, bias=_b)
        CASES[f"{_role}_n{_n}_t{_t}_2d_residual"] = _case(_role, _n, _k, _t, bias=_b, x="2d", res="ok")
        CASES[f"{_role}_n{_n}_t{_t}_grad_mode"] = _case(_role, _n, _k, _t, bias=_b, res="ok", grad=True)
        CASES[f"{_role}_n{_n}_t{_t}_fp16"] = _case(_role, _n, _k, _t, dtype=F16, bias=_b, res="ok")
for _mode in ("highest", "high", "medium"):
    for _role, (_n, _k, _b, _r) in shapes(640).items():
        CASES[f"fp32_{_mode}_{_role}"] = _case(_role, _n, _k, 8192, dtype=F32, bias=0 if _b else None, res="ok" if _r else None, precision=_mode)
    CASES[f"fp32_{_mode}_bias_8"] = _case("to_out", 640, 512, 8192, dtype=F32, bias=8, precision=_mode)
    CASES[f"fp32_{_mode}_x_pitch+4"] = _case("in_proj", 2560, 640, 8192, dtype=F32, x="2d", x_pitch=4, precision=_mode)
    CASES[f"fp32_{_mode}_x_pitch+2"] = _case("in_proj", 2560, 640, 8192, dtype=F32, x="2d", x_pitch=2, precision=_mode)
    CASES[f"fp32_{_mode}_3d_nc"] = _case("in_proj", 2560, 640, 8192, dtype=F32, x="3d_nc", x_pitch=64, precision=_mode)
    CASES[f"fp32_{_mode}_tokens_100"] = _case("in_proj", 2560, 640, 100, dtype=F32, x="2d", precision=_mode)
    CASES[f"fp32_{_mode}_n_100"] = _case("text", 100, 640, 2048, dtype=F32, x="2d", precision=_mode)
    CASES[f"fp32_{_mode}_grad"] = _case("in_proj", 2560, 640, 8192, dtype=F32, grad=True, w_grad=True, precision=_mode)
    CASES[f"fp32_{_mode}_policy_off"] = _case("in_proj", 2560, 640, 8192, dtype=F32, precision=_mode, policy="off")
    CASES[f"fp32_{_mode}_mixed_bf16_x"] = _case("in_proj", 2560, 640, 8192, dtype=BF, w_dtype=F32, precision=_mode)
for _ac in (BF, F16):
    _tag = "bf16" if _ac == BF else "fp16"
    for _role, (_n, _k, _b, _r) in shapes(640).items():
        for _t in (8192, 65536):
            CASES[f"autocast_{_tag}_{_role}_t{_t}"] = _case(_role, _n, _k, _t, dtype=_ac, w_dtype=F32, bias=0 if _b else None, res="ok" if _r else None, autocast=_ac)
    CASES[f"autocast_{_tag}_param_grad"] = _case("in_proj", 2560, 640, 65536, dtype=_ac, w_dtype=F32, autocast=_ac, grad=True, w_grad=True)
    CASES[f"autocast_{_tag}_param_grad_off"] = _case("in_proj", 2560, 640, 65536, dtype=_ac, w_dtype=F32, autocast=_ac, w_grad=True)
    CASES[f"autocast_{_tag}_grad_mode_frozen"] = _case("out_proj", 640, 1280, 65536, dtype=_ac, w_dtype=F32, autocast=_ac, grad=True, res="ok")
    CASES[f"autocast_{_tag}_fp32_x"] = _case("in_proj", 2560, 640, 65536, dtype=F32, w_dtype=F32, autocast=_ac)
    CASES[f"autocast_{_tag}_other_16bit_x"] = _case("in_proj", 2560, 640, 65536, dtype=F16 if _ac == BF else BF, w_dtype=F32, autocast=_ac)
    CASES[f"autocast_{_tag}_16bit_weight"] = _case("in_proj", 2560, 640, 65536, dtype=_ac, autocast=_ac)
for _t in (8192, 65536):
    CASES[f"grad_x_t{_t}"] = _case("in_proj", 2560, 640, _t, grad=True, x_grad=True)
    CASES[f"grad_w_t{_t}"] = _case("in_proj", 2560, 640, _t, grad=True, w_grad=True)
    CASES[f"no_grad_w_requires_grad_t{_t}"] = _case("in_proj", 2560, 640, _t, w_grad=True)
    CASES[f"grad_mode_nothing_requires_t{_t}"] = _case("in_proj", 2560, 640, _t, grad=True)
    CASES[f"cpu_t{_t}"] = _case("in_proj", 2560, 640, _t, cuda=False)
    CASES[f"mixed_16bit_t{_t}"] = _case("in_proj", 2560, 640, _t, dtype=F16, w_dtype=BF)
    CASES[f"tokens_odd_t{_t}"] = _case("to_q", 512, 640, _t + 4, x="2d")
    CASES[f"tokens_plus_8_t{_t}"] = _case("to_q", 512, 640, _t + 8, x="2d")
    CASES[f"n_100_t{_t}"] = _case("text", 100, 640, _t, x="2d")
    CASES[f"k_100_t{_t}"] = _case("text", 640, 100, _t, x="2d")
    for _policy in ("all", "off"):
        for _role, (_n, _k, _b, _r) in shapes(640).items():
            CASES[f"policy_{_policy}_{_role}_t{_t}"] = _case(_role, _n, _k, _t, bias=0 if _b else None, res="ok" if _r else None, policy=_policy)
        CASES[f"policy_{_policy}_in_proj_n_100_t{_t}"] = _case("in_proj", 100, 640, _t, policy=_policy)
        CASES[f"policy_{_policy}_to_out_res_misaligned_t{_t}"] = _case("to_out", 640, 512, _t, bias=0, res="misaligned", policy=_policy)
    for _row in ("in_proj.ws", "in_proj.ws+in_proj.halves", "out_proj.sm+out_proj.tiled"):
        CASES[f"disabled_{_row}_in_proj_t{_t}"] = _case("in_proj", 2560, 640, _t, disabled=_row)
        CASES[f"disabled_{_row}_out_proj_t{_t}"] = _case("out_proj", 640, 1280, _t, res="ok", disabled=_row)
    for _n, _k in ((2560, 640), (640, 2560), (640, 1280), (1280, 640), (512, 640), (640, 512), (3072, 768), (100, 640)):
        CASES[f"wgrad_dx_n{_n}_k{_k}_t{_t}"] = _case("train", _n, _k, _t, x="2d", transposed=True)
        CASES[f"wgrad_dx_n{_n}_k{_k}_t{_t}_fp16"] = _case("train", _n, _k, _t, dtype=F16, x="2d", transposed=True)


def _operands(c):
    n, k, tokens, dt, cuda = c["n"], c["k"], c["tokens"], c["dtype"], c["cuda"]
    es = 4 if dt == F32 else 2
    L = 1024 if tokens % 1024 == 0 else tokens
    B = tokens // L
    if c["x"] == "2d":
        x = T(dt, (tokens, k), (k + c["x_pitch"], 1), PTR["x"], cuda, c["x_grad"])
    else:
        pitch = k + c["x_pitch"]
        x = T(dt, (B, L, k), (L * pitch, pitch, 1), PTR["x"], cuda, c["x_grad"])
    if c["transposed"]:
        from zigma_amd import wgrad
        w = wgrad._ContiguousLike(T(c["w_dtype"], (k, n), None, PTR["w"], cuda, c["w_grad"]))
    else:
        w = T(c["w_dtype"], (n, k), None, PTR["w"], cuda, c["w_grad"])
    bias = None if c["bias"] is None else T(c["w_dtype"], (n,), None, PTR["bias"] + c["bias"], cuda, c["w_grad"])
    residual = gate = None
    if c["res"]:
        pitch = n + {"pitch": 8, "odd_pitch": 4}.get(c["res"], 0)
        lead = (B, L) if c["x"] != "2d" else (1, tokens)
        batch = lead[1] * pitch + (pitch if c["res"] == "batch_pitch" else 0)
        residual = T(dt, (*lead, n), (batch, pitch, 1), PTR["residual"] + (8 if c["res"] == "misaligned" else 0), cuda)
        gate = T(dt, (lead[0], n), (n + c["gate_pitch"], 1), PTR["gate"] + c["gate_off"], cuda)
    del es
    return x, w, bias, residual, gate


@contextlib.contextmanager
def _setting(c):
    from zigma_amd import fp32_matmul, routing
    saved = (fp32_matmul.PRECISION, routing.POLICY, routing.DISABLED)
    fp32_matmul.PRECISION, routing.POLICY, routing.DISABLED = c["precision"], c["policy"], c["disabled"]
    ac = (torch.is_autocast_enabled(), torch.get_autocast_dtype("cuda"))
    try:
        if c["autocast"]:           # (the thread's autocast state, set directly: torch.autocast("cuda") switches itself off where no device is present)
            torch.set_autocast_enabled(True), torch.set_autocast_dtype("cuda", c["autocast"])
        with torch.set_grad_enabled(c["grad"]):
            yield
    finally:
        torch.set_autocast_enabled(ac[0]), torch.set_autocast_dtype("cuda", ac[1])
        fp32_matmul.PRECISION, routing.POLICY, routing.DISABLED = saved


def call(plan, c):
    """linear.plan on the case's descriptors under the case's knobs, grad mode and autocast state -> (kernel, fuse_add, row)"""
    x, w, bias, residual, gate = _operands(c)
    with _setting(c):
        return tuple(plan(c["role"], x, w, bias, residual, gate))


# ---- the verdicts of the three predicates outside the walk ------------------------------------------------------------------------------------
def _gated(dtype=BF, B=16, L=256, k=192, n=256, res_dtype=None, gate_dtype=None, res_pitch=0, res_batch=0, res_off=0, gate_off=0, gate_pitch=0, x_dim=3,
           gate_dim=2, res_col_stride=1, gate_col_stride=1):
    return dict(dtype=dtype, B=B, L=L, k=k, n=n, res_dtype=res_dtype or dtype, gate_dtype=gate_dtype or dtype, res_pitch=res_pitch, res_batch=res_batch,
                res_off=res_off, gate_off=gate_off, gate_pitch=gate_pitch, x_dim=x_dim, gate_dim=gate_dim, res_col_stride=res_col_stride, gate_col_stride=gate_col_stride)


GATED_CASES = {
    "plain": _gated(), "fp16": _gated(F16), "fp32": _gated(F32), "rows_128": _gated(L=128), "rows_264": _gated(L=264), "rows_512": _gated(L=512), "one_sample": _gated(B=1),
    "res_other_dtype": _gated(res_dtype=F16), "gate_other_dtype": _gated(gate_dtype=F16), "res_pitch+8": _gated(res_pitch=8), "res_pitch+4": _gated(res_pitch=4),
    "res_pitch+128": _gated(res_pitch=128), "res_batch_gap": _gated(res_batch=256), "res_2_bytes_off": _gated(res_off=2), "res_8_bytes_off": _gated(res_off=8),
    "res_16_bytes_off": _gated(res_off=16), "gate_8_bytes_off": _gated(gate_off=8), "gate_16_bytes_off": _gated(gate_off=16), "gate_pitch+4": _gated(gate_pitch=4),
    "gate_pitch+8": _gated(gate_pitch=8), "x_2d": _gated(x_dim=2), "gate_3d": _gated(gate_dim=3), "res_col_stride_2": _gated(res_col_stride=2),
    "gate_col_stride_2": _gated(gate_col_stride=2), "res_pitch_2^22": _gated(B=1, res_pitch=(1 << 22) - 256), "res_pitch_2^22-8": _gated(B=1, res_pitch=(1 << 22) - 264),
}


def call_gated(gated_residual_eligible, c):
    B, L, k, n = c["B"], c["L"], c["k"], c["n"]
    x = T(c["dtype"], (B, L, k), None, PTR["x"]) if c["x_dim"] == 3 else T(c["dtype"], (B * L, k), None, PTR["x"])
    pitch = (n + c["res_pitch"]) * c["res_col_stride"]
    residual = T(c["res_dtype"], (B, L, n), (L * pitch + c["res_batch"], pitch, c["res_col_stride"]), PTR["residual"] + c["res_off"])
    gpitch = (n + c["gate_pitch"]) * c["gate_col_stride"]
    gate = T(c["gate_dtype"], (B, n), (gpitch, c["gate_col_stride"]), PTR["gate"] + c["gate_off"]) if c["gate_dim"] == 2 else \
        T(c["gate_dtype"], (B, 1, n), (gpitch, gpitch, c["gate_col_stride"]), PTR["gate"] + c["gate_off"])
    with torch.no_grad():
        return bool(gated_residual_eligible(x, residual, gate))


def _nl(dtype=BF, B=2, L=1024, k=640, n=512, x_pitch=0, w_pitch=0, mod_pitch=None, x_off=0, w_off=0, shift_off=0, scale_off=0, bias=False, cuda=True, grad=False,
        w_dtype=None, mod_dtype=None, x_batch_gap=0, scale_pitch=None):
    return dict(dtype=dtype, B=B, L=L, k=k, n=n, x_pitch=x_pitch, w_pitch=w_pitch, mod_pitch=6 * k if mod_pitch is None else mod_pitch, x_off=x_off, w_off=w_off,
                shift_off=shift_off, scale_off=scale_off, bias=bias, cuda=cuda, grad=grad, w_dtype=w_dtype or dtype, mod_dtype=mod_dtype or dtype,
                x_batch_gap=x_batch_gap, scale_pitch=scale_pitch)


NORM_LINEAR_CASES = {
    "plain": _nl(), "fp16": _nl(F16), "fp32": _nl(F32), "k512": _nl(k=512), "k768": _nl(k=768), "k576": _nl(k=576), "k1024": _nl(k=1024), "n640": _nl(n=640), "n256": _nl(n=256),
    "L128": _nl(L=128), "L64_B2": _nl(L=64), "L64_B1": _nl(B=1, L=64), "L96_B4": _nl(B=4, L=96), "L1032": _nl(L=1032), "x_pitch+8": _nl(x_pitch=8), "x_pitch+4": _nl(x_pitch=4),
    "w_pitch+8": _nl(w_pitch=8), "w_pitch+4": _nl(w_pitch=4), "mod_pitch_k": _nl(mod_pitch=640), "mod_pitch_0": _nl(mod_pitch=0), "mod_pitch+4": _nl(mod_pitch=6 * 640 + 4),
    "x_2_bytes_off": _nl(x_off=2), "x_16_bytes_off": _nl(x_off=16), "w_8_bytes_off": _nl(w_off=8), "shift_8_bytes_off": _nl(shift_off=8), "scale_8_bytes_off": _nl(scale_off=8),
    "scale_16_bytes_off": _nl(scale_off=16), "bias": _nl(bias=True), "cpu": _nl(cuda=False), "requires_grad": _nl(grad=True), "w_other_dtype": _nl(w_dtype=F16),
    "mod_other_dtype": _nl(mod_dtype=F16), "x_batch_gap": _nl(x_batch_gap=640), "scale_other_pitch": _nl(scale_pitch=3 * 640),
    "x_pitch_2^27": _nl(B=1, L=128, x_pitch=(1 << 27) - 640), "x_pitch_2^27-8": _nl(B=1, L=128, x_pitch=(1 << 27) - 648),
    "w_pitch_2^27": _nl(w_pitch=(1 << 27) - 640), "w_pitch_2^27-8": _nl(w_pitch=(1 << 27) - 648),
}


def call_norm_linear(norm_linear_eligible, c):
    B, L, k, n, dt, cuda = c["B"], c["L"], c["k"], c["n"], c["dtype"], c["cuda"]
    pitch = k + c["x_pitch"]
    x = T(dt, (B, L, k), (L * pitch + c["x_batch_gap"], pitch, 1), PTR["x"] + c["x_off"], cuda, c["grad"])
    w = T(c["w_dtype"], (n, k), (k + c["w_pitch"], 1), PTR["w"] + c["w_off"], cuda)
    shift = T(c["mod_dtype"], (B, k), (c["mod_pitch"], 1), PTR["shift"] + c["shift_off"], cuda)
    scale = T(c["mod_dtype"], (B, k), (c["mod_pitch"] if c["scale_pitch"] is None else c["scale_pitch"], 1), PTR["scale"] + c["scale_off"], cuda)
    bias = T(dt, (n,), None, PTR["bias"], cuda) if c["bias"] else None
    with torch.set_grad_enabled(c["grad"]):
        return bool(norm_linear_eligible(x, w, shift, scale, bias))


def _sp(tokens=2048, n=2560, k=640, dtype=F32, w_dtype=F32, bias=None, bias_dtype=F32, x="2d", x_pitch=0, x_off=0, cuda=True, grad=False, w_grad=False, w_dim=2):
    return dict(tokens=tokens, n=n, k=k, dtype=dtype, w_dtype=w_dtype, bias=bias, bias_dtype=bias_dtype, x=x, x_pitch=x_pitch, x_off=x_off, cuda=cuda, grad=grad,
                w_grad=w_grad, w_dim=w_dim)


SPLIT_CASES = {
    "plain": _sp(), "3d": _sp(x="3d"), "bias": _sp(bias=0), "bias_8_bytes_off": _sp(bias=8), "bias_bf16": _sp(bias=0, bias_dtype=BF), "x_bf16": _sp(dtype=BF), "w_bf16": _sp(w_dtype=BF),
    "cpu": _sp(cuda=False), "grad_w": _sp(grad=True, w_grad=True), "no_grad_w_requires": _sp(w_grad=True), "grad_mode_nothing_requires": _sp(grad=True), "w_3d": _sp(w_dim=3),
    "k_32": _sp(k=32), "k_64": _sp(k=64), "k_96": _sp(k=96), "k_65536": _sp(tokens=8, n=128, k=65536), "k_65600": _sp(tokens=8, n=128, k=65600),
    "n_64": _sp(n=64), "n_128": _sp(n=128), "n_192": _sp(n=192), "n_65536": _sp(tokens=8, n=65536, k=64), "n_65664": _sp(tokens=8, n=65664, k=64),
    "tokens_8": _sp(tokens=8), "tokens_4": _sp(tokens=4), "tokens_100": _sp(tokens=100), "tokens_0": _sp(tokens=0), "tiles_2^31": _sp(tokens=1 << 29, n=512, k=64),
    "tiles_below_2^31": _sp(tokens=(1 << 29) - 128, n=512, k=64), "x_pitch+4": _sp(x_pitch=4), "x_pitch+2": _sp(x_pitch=2), "x_pitch-64": _sp(x_pitch=-64),
    "x_3d_nc": _sp(x="3d", x_pitch=64), "x_8_bytes_off": _sp(x_off=8), "x_16_bytes_off": _sp(x_off=16),
}


def call_split(split_eligible, c):
    tokens, n, k, cuda = c["tokens"], c["n"], c["k"], c["cuda"]
    pitch = k + c["x_pitch"]
    if c["x"] == "2d":
        x = T(c["dtype"], (tokens, k), (pitch, 1), PTR["x"] + c["x_off"], cuda)
    else:
        L = 1024 if tokens % 1024 == 0 else tokens
        x = T(c["dtype"], (tokens // L, L, k), (L * pitch, pitch, 1), PTR["x"] + c["x_off"], cuda)
    w = T(c["w_dtype"], (n, k) if c["w_dim"] == 2 else (1, n, k), None, PTR["w"], cuda, c["w_grad"])
    bias = None if c["bias"] is None else T(c["bias_dtype"], (n,), None, PTR["bias"] + c["bias"], cuda)
    with torch.set_grad_enabled(c["grad"]):
        return bool(split_eligible(x, w, bias))


# case: (kernel, fuse_add, row), recorded on the parent commit
EXPECTED = {
    'in_proj_E512_t2048': ('library', False, 'in_proj.library'),
    'in_proj_E512_t4096': ('library', False, 'in_proj.library'),
    'in_proj_E512_t8192': ('ws', False, 'in_proj.ws'),
    'in_proj_E512_t16384': ('ws', False, 'in_proj.ws'),
    'in_proj_E512_t32768': ('ws', False, 'in_proj.ws'),
    'in_proj_E512_t65536': ('ws', False, 'in_proj.ws'),
    'in_proj_E512_t131072': ('ws', False, 'in_proj.ws'),
    'out_proj_E512_t2048': ('sm', False, 'out_proj.sm'),
    'out_proj_E512_t4096': ('sm', False, 'out_proj.sm'),
    'out_proj_E512_t8192': ('sm', False, 'out_proj.sm'),
    'out_proj_E512_t16384': ('library', False, 'out_proj.library'),
    'out_proj_E512_t32768': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E512_t65536': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E512_t131072': ('tiled', True, 'out_proj.tiled'),
    'to_q_E512_t2048': ('sm', False, 'to_q.sm'),
    'to_q_E512_t4096': ('sm', False, 'to_q.sm'),
    'to_q_E512_t8192': ('sm', False, 'to_q.sm'),
    'to_q_E512_t16384': ('tiled', False, 'to_q.tiled'),
    'to_q_E512_t32768': ('tiled', False, 'to_q.tiled'),
    'to_q_E512_t65536': ('tiled', False, 'to_q.tiled'),
    'to_q_E512_t131072': ('tiled', False, 'to_q.tiled'),
    'to_out_E512_t2048': ('sm', True, 'to_out.sm'),
    'to_out_E512_t4096': ('sm', True, 'to_out.sm'),
    'to_out_E512_t8192': ('sm', True, 'to_out.sm'),
    'to_out_E512_t16384': ('tiled', True, 'to_out.tiled'),
    'to_out_E512_t32768': ('tiled', True, 'to_out.tiled'),
    'to_out_E512_t65536': ('tiled', True, 'to_out.tiled'),
    'to_out_E512_t131072': ('tiled', True, 'to_out.tiled'),
    'text_E512_t2048': ('tiled', False, 'text.tiled'),
    'text_E512_t4096': ('tiled', False, 'text.tiled'),
    'text_E512_t8192': ('tiled', False, 'text.tiled'),
    'text_E512_t16384': ('tiled', False, 'text.tiled'),
    'text_E512_t32768': ('tiled', False, 'text.tiled'),
    'text_E512_t65536': ('tiled', False, 'text.tiled'),
    'text_E512_t131072': ('tiled', False, 'text.tiled'),
    'train_E512_t2048': ('ws', False, 'train.ws'),
    'train_E512_t4096': ('ws', False, 'train.ws'),
    'train_E512_t8192': ('ws', False, 'train.ws'),
    'train_E512_t16384': ('ws', False, 'train.ws'),
    'train_E512_t32768': ('ws', False, 'train.ws'),
    'train_E512_t65536': ('ws', False, 'train.ws'),
    'train_E512_t131072': ('ws', False, 'train.ws'),
    'in_proj_E640_t2048': ('library', False, 'in_proj.library'),
    'in_proj_E640_t4096': ('library', False, 'in_proj.library'),
    'in_proj_E640_t8192': ('ws', False, 'in_proj.ws'),
    'in_proj_E640_t16384': ('ws', False, 'in_proj.ws'),
    'in_proj_E640_t32768': ('ws', False, 'in_proj.ws'),
    'in_proj_E640_t65536': ('ws', False, 'in_proj.ws'),
    'in_proj_E640_t131072': ('ws', False, 'in_proj.ws'),
    'out_proj_E640_t2048': ('sm', False, 'out_proj.sm'),
    'out_proj_E640_t4096': ('sm', False, 'out_proj.sm'),
    'out_proj_E640_t8192': ('sm', False, 'out_proj.sm'),
    'out_proj_E640_t16384': ('ws128', False, 'out_proj.ws128'),
    'out_proj_E640_t32768': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E640_t65536': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E640_t131072': ('tiled', True, 'out_proj.tiled'),
    'to_q_E640_t2048': ('sm', False, 'to_q.sm'),
    'to_q_E640_t4096': ('sm', False, 'to_q.sm'),
    'to_q_E640_t8192': ('sm', False, 'to_q.sm'),
    'to_q_E640_t16384': ('tiled', False, 'to_q.tiled'),
    'to_q_E640_t32768': ('tiled', False, 'to_q.tiled'),
    'to_q_E640_t65536': ('tiled', False, 'to_q.tiled'),
    'to_q_E640_t131072': ('tiled', False, 'to_q.tiled'),
    'to_out_E640_t2048': ('sm', True, 'to_out.sm'),
    'to_out_E640_t4096': ('sm', True, 'to_out.sm'),
    'to_out_E640_t8192': ('sm', True, 'to_out.sm'),
    'to_out_E640_t16384': ('tiled', True, 'to_out.tiled'),
    'to_out_E640_t32768': ('tiled', True, 'to_out.tiled'),
    'to_out_E640_t65536': ('tiled', True, 'to_out.tiled'),
    'to_out_E640_t131072': ('tiled', True, 'to_out.tiled'),
    'text_E640_t2048': ('tiled', False, 'text.tiled'),
    'text_E640_t4096': ('tiled', False, 'text.tiled'),
    'text_E640_t8192': ('tiled', False, 'text.tiled'),
    'text_E640_t16384': ('tiled', False, 'text.tiled'),
    'text_E640_t32768': ('tiled', False, 'text.tiled'),
    'text_E640_t65536': ('tiled', False, 'text.tiled'),
    'text_E640_t131072': ('tiled', False, 'text.tiled'),
    'train_E640_t2048': ('ws', False, 'train.ws'),
    'train_E640_t4096': ('ws', False, 'train.ws'),
    'train_E640_t8192': ('ws', False, 'train.ws'),
    'train_E640_t16384': ('ws', False, 'train.ws'),
    'train_E640_t32768': ('ws', False, 'train.ws'),
    'train_E640_t65536': ('ws', False, 'train.ws'),
    'train_E640_t131072': ('ws', False, 'train.ws'),
    'in_proj_E768_t2048': ('library', False, 'in_proj.library'),
    'in_proj_E768_t4096': ('library', False, 'in_proj.library'),
    'in_proj_E768_t8192': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E768_t16384': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E768_t32768': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E768_t65536': ('library', False, 'in_proj.library_k768'),
    'in_proj_E768_t131072': ('library', False, 'in_proj.library_k768'),
    'out_proj_E768_t2048': ('sm', False, 'out_proj.sm'),
    'out_proj_E768_t4096': ('sm', False, 'out_proj.sm'),
    'out_proj_E768_t8192': ('sm', False, 'out_proj.sm'),
    'out_proj_E768_t16384': ('ws128', False, 'out_proj.ws128'),
    'out_proj_E768_t32768': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E768_t65536': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E768_t131072': ('tiled', True, 'out_proj.tiled'),
    'to_q_E768_t2048': ('sm', False, 'to_q.sm'),
    'to_q_E768_t4096': ('sm', False, 'to_q.sm'),
    'to_q_E768_t8192': ('sm', False, 'to_q.sm'),
    'to_q_E768_t16384': ('tiled', False, 'to_q.tiled'),
    'to_q_E768_t32768': ('tiled', False, 'to_q.tiled'),
    'to_q_E768_t65536': ('tiled', False, 'to_q.tiled'),
    'to_q_E768_t131072': ('tiled', False, 'to_q.tiled'),
    'to_out_E768_t2048': ('sm', True, 'to_out.sm'),
    'to_out_E768_t4096': ('sm', True, 'to_out.sm'),
    'to_out_E768_t8192': ('sm', True, 'to_out.sm'),
    'to_out_E768_t16384': ('tiled', True, 'to_out.tiled'),
    'to_out_E768_t32768': ('tiled', True, 'to_out.tiled'),
    'to_out_E768_t65536': ('tiled', True, 'to_out.tiled'),
    'to_out_E768_t131072': ('tiled', True, 'to_out.tiled'),
    'text_E768_t2048': ('tiled', False, 'text.tiled'),
    'text_E768_t4096': ('tiled', False, 'text.tiled'),
    'text_E768_t8192': ('tiled', False, 'text.tiled'),
    'text_E768_t16384': ('tiled', False, 'text.tiled'),
    'text_E768_t32768': ('tiled', False, 'text.tiled'),
    'text_E768_t65536': ('tiled', False, 'text.tiled'),
    'text_E768_t131072': ('tiled', False, 'text.tiled'),
    'train_E768_t2048': ('tiled', False, 'train.tiled'),
    'train_E768_t4096': ('tiled', False, 'train.tiled'),
    'train_E768_t8192': ('tiled', False, 'train.tiled'),
    'train_E768_t16384': ('tiled', False, 'train.tiled'),
    'train_E768_t32768': ('tiled', False, 'train.tiled'),
    'train_E768_t65536': ('tiled', False, 'train.tiled'),
    'train_E768_t131072': ('tiled', False, 'train.tiled'),
    'in_proj_E1024_t2048': ('library', False, 'in_proj.library'),
    'in_proj_E1024_t4096': ('library', False, 'in_proj.library'),
    'in_proj_E1024_t8192': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E1024_t16384': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E1024_t32768': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E1024_t65536': ('tiled', False, 'in_proj.tiled_wide_k'),
    'in_proj_E1024_t131072': ('tiled', False, 'in_proj.tiled_wide_k'),
    'out_proj_E1024_t2048': ('sm', False, 'out_proj.sm'),
    'out_proj_E1024_t4096': ('sm', False, 'out_proj.sm'),
    'out_proj_E1024_t8192': ('sm', False, 'out_proj.sm'),
    'out_proj_E1024_t16384': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E1024_t32768': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E1024_t65536': ('tiled', True, 'out_proj.tiled'),
    'out_proj_E1024_t131072': ('tiled', True, 'out_proj.tiled'),
    'to_q_E1024_t2048': ('sm', False, 'to_q.sm'),
    'to_q_E1024_t4096': ('sm', False, 'to_q.sm'),
    'to_q_E1024_t8192': ('sm', False, 'to_q.sm'),
    'to_q_E1024_t16384': ('tiled', False, 'to_q.tiled'),
    'to_q_E1024_t32768': ('tiled', False, 'to_q.tiled'),
    'to_q_E1024_t65536': ('tiled', False, 'to_q.tiled'),
    'to_q_E1024_t131072': ('tiled', False, 'to_q.tiled'),
    'to_out_E1024_t2048': ('sm', True, 'to_out.sm'),
    'to_out_E1024_t4096': ('sm', True, 'to_out.sm'),
    'to_out_E1024_t8192': ('sm', True, 'to_out.sm'),
    'to_out_E1024_t16384': ('tiled', True, 'to_out.tiled'),
    'to_out_E1024_t32768': ('tiled', True, 'to_out.tiled'),
    'to_out_E1024_t65536': ('tiled', True, 'to_out.tiled'),
    'to_out_E1024_t131072': ('tiled', True, 'to_out.tiled'),
    'text_E1024_t2048': ('tiled', False, 'text.tiled'),
    'text_E1024_t4096': ('tiled', False, 'text.tiled'),
    'text_E1024_t8192': ('tiled', False, 'text.tiled'),
    'text_E1024_t16384': ('tiled', False, 'text.tiled'),
    'text_E1024_t32768': ('tiled', False, 'text.tiled'),
    'text_E1024_t65536': ('tiled', False, 'text.tiled'),
    'text_E1024_t131072': ('tiled', False, 'text.tiled'),
    'train_E1024_t2048': ('tiled', False, 'train.tiled'),
    'train_E1024_t4096': ('tiled', False, 'train.tiled'),
    'train_E1024_t8192': ('tiled', False, 'train.tiled'),
    'train_E1024_t16384': ('tiled', False, 'train.tiled'),
    'train_E1024_t32768': ('tiled', False, 'train.tiled'),
    'train_E1024_t65536': ('tiled', False, 'train.tiled'),
    'train_E1024_t131072': ('tiled', False, 'train.tiled'),
    'to_out_E640_t8192_bias_None': ('sm', True, 'to_out.sm'),
    'text_E640_t8192_bias_None': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t8192_bias_None': ('ws', False, 'in_proj.ws'),
    'to_out_E640_t8192_bias_0': ('sm', True, 'to_out.sm'),
    'text_E640_t8192_bias_0': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t8192_bias_0': ('library', False, 'in_proj.library'),
    'to_out_E640_t8192_bias_8': ('sm', True, 'to_out.sm'),
    'text_E640_t8192_bias_8': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t8192_bias_8': ('library', False, 'in_proj.library'),
    'to_out_E640_t8192_bias_4': ('tiled', True, 'to_out.tiled'),
    'text_E640_t8192_bias_4': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t8192_bias_4': ('library', False, 'in_proj.library'),
    'to_out_E640_t8192_bias_2': ('library', False, 'not-16bit-inference'),
    'text_E640_t8192_bias_2': ('library', False, 'not-16bit-inference'),
    'in_proj_E640_t8192_bias_2': ('library', False, 'not-16bit-inference'),
    'to_out_n8192_t8192_bias': ('library', False, 'not-16bit-inference'),
    'to_out_E640_t65536_bias_None': ('tiled', True, 'to_out.tiled'),
    'text_E640_t65536_bias_None': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t65536_bias_None': ('ws', False, 'in_proj.ws'),
    'to_out_E640_t65536_bias_0': ('tiled', True, 'to_out.tiled'),
    'text_E640_t65536_bias_0': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t65536_bias_0': ('library', False, 'in_proj.library'),
    'to_out_E640_t65536_bias_8': ('tiled', True, 'to_out.tiled'),
    'text_E640_t65536_bias_8': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t65536_bias_8': ('library', False, 'in_proj.library'),
    'to_out_E640_t65536_bias_4': ('tiled', True, 'to_out.tiled'),
    'text_E640_t65536_bias_4': ('tiled', False, 'text.tiled'),
    'in_proj_E640_t65536_bias_4': ('library', False, 'in_proj.library'),
    'to_out_E640_t65536_bias_2': ('library', False, 'not-16bit-inference'),
    'text_E640_t65536_bias_2': ('library', False, 'not-16bit-inference'),
    'in_proj_E640_t65536_bias_2': ('library', False, 'not-16bit-inference'),
    'to_out_n8192_t65536_bias': ('library', False, 'not-16bit-inference'),
    'in_proj_k640_t8192_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'in_proj_k640_t8192_2d_pitch+8': ('library', False, 'in_proj.library'),
    'in_proj_k640_t8192_2d_pitch+128': ('ws', False, 'in_proj.ws'),
    'in_proj_k640_t8192_2d': ('ws', False, 'in_proj.ws'),
    'in_proj_k640_t8192_3d_nc': ('library', False, 'not-16bit-inference'),
    'in_proj_k640_t16384_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'in_proj_k640_t16384_2d_pitch+8': ('library', False, 'in_proj.library'),
    'in_proj_k640_t16384_2d_pitch+128': ('ws', False, 'in_proj.ws'),
    'in_proj_k640_t16384_2d': ('ws', False, 'in_proj.ws'),
    'in_proj_k640_t16384_3d_nc': ('library', False, 'not-16bit-inference'),
    'in_proj_k640_t65536_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'in_proj_k640_t65536_2d_pitch+8': ('library', False, 'in_proj.library'),
    'in_proj_k640_t65536_2d_pitch+128': ('ws', False, 'in_proj.ws'),
    'in_proj_k640_t65536_2d': ('ws', False, 'in_proj.ws'),
    'in_proj_k640_t65536_3d_nc': ('library', False, 'not-16bit-inference'),
    'out_proj_k1280_t8192_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'out_proj_k1280_t8192_2d_pitch+8': ('sm', False, 'out_proj.sm'),
    'out_proj_k1280_t8192_2d_pitch+128': ('sm', False, 'out_proj.sm'),
    'out_proj_k1280_t8192_2d': ('sm', False, 'out_proj.sm'),
    'out_proj_k1280_t8192_3d_nc': ('library', False, 'not-16bit-inference'),
    'out_proj_k1280_t16384_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'out_proj_k1280_t16384_2d_pitch+8': ('library', False, 'out_proj.library'),
    'out_proj_k1280_t16384_2d_pitch+128': ('ws128', False, 'out_proj.ws128'),
    'out_proj_k1280_t16384_2d': ('ws128', False, 'out_proj.ws128'),
    'out_proj_k1280_t16384_3d_nc': ('library', False, 'not-16bit-inference'),
    'out_proj_k1280_t65536_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'out_proj_k1280_t65536_2d_pitch+8': ('tiled', False, 'out_proj.tiled'),
    'out_proj_k1280_t65536_2d_pitch+128': ('tiled', False, 'out_proj.tiled'),
    'out_proj_k1280_t65536_2d': ('tiled', False, 'out_proj.tiled'),
    'out_proj_k1280_t65536_3d_nc': ('library', False, 'not-16bit-inference'),
    'to_q_k640_t8192_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'to_q_k640_t8192_2d_pitch+8': ('sm', False, 'to_q.sm'),
    'to_q_k640_t8192_2d_pitch+128': ('sm', False, 'to_q.sm'),
    'to_q_k640_t8192_2d': ('sm', False, 'to_q.sm'),
    'to_q_k640_t8192_3d_nc': ('library', False, 'not-16bit-inference'),
    'to_q_k640_t16384_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'to_q_k640_t16384_2d_pitch+8': ('tiled', False, 'to_q.tiled'),
    'to_q_k640_t16384_2d_pitch+128': ('tiled', False, 'to_q.tiled'),
    'to_q_k640_t16384_2d': ('tiled', False, 'to_q.tiled'),
    'to_q_k640_t16384_3d_nc': ('library', False, 'not-16bit-inference'),
    'to_q_k640_t65536_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'to_q_k640_t65536_2d_pitch+8': ('tiled', False, 'to_q.tiled'),
    'to_q_k640_t65536_2d_pitch+128': ('tiled', False, 'to_q.tiled'),
    'to_q_k640_t65536_2d': ('tiled', False, 'to_q.tiled'),
    'to_q_k640_t65536_3d_nc': ('library', False, 'not-16bit-inference'),
    'train_k640_t8192_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'train_k640_t8192_2d_pitch+8': ('tiled', False, 'train.tiled'),
    'train_k640_t8192_2d_pitch+128': ('ws', False, 'train.ws'),
    'train_k640_t8192_2d': ('ws', False, 'train.ws'),
    'train_k640_t8192_3d_nc': ('library', False, 'not-16bit-inference'),
    'train_k640_t16384_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'train_k640_t16384_2d_pitch+8': ('tiled', False, 'train.tiled'),
    'train_k640_t16384_2d_pitch+128': ('ws', False, 'train.ws'),
    'train_k640_t16384_2d': ('ws', False, 'train.ws'),
    'train_k640_t16384_3d_nc': ('library', False, 'not-16bit-inference'),
    'train_k640_t65536_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'train_k640_t65536_2d_pitch+8': ('tiled', False, 'train.tiled'),
    'train_k640_t65536_2d_pitch+128': ('ws', False, 'train.ws'),
    'train_k640_t65536_2d': ('ws', False, 'train.ws'),
    'train_k640_t65536_3d_nc': ('library', False, 'not-16bit-inference'),
    'train_k1280_t8192_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'train_k1280_t8192_2d_pitch+8': ('tiled', False, 'train.tiled'),
    'train_k1280_t8192_2d_pitch+128': ('ws128', False, 'train.ws128'),
    'train_k1280_t8192_2d': ('ws128', False, 'train.ws128'),
    'train_k1280_t8192_3d_nc': ('library', False, 'not-16bit-inference'),
    'train_k1280_t16384_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'train_k1280_t16384_2d_pitch+8': ('tiled', False, 'train.tiled'),
    'train_k1280_t16384_2d_pitch+128': ('ws128', False, 'train.ws128'),
    'train_k1280_t16384_2d': ('ws128', False, 'train.ws128'),
    'train_k1280_t16384_3d_nc': ('library', False, 'not-16bit-inference'),
    'train_k1280_t65536_2d_pitch+4': ('library', False, 'not-16bit-inference'),
    'train_k1280_t65536_2d_pitch+8': ('tiled', False, 'train.tiled'),
    'train_k1280_t65536_2d_pitch+128': ('ws128', False, 'train.ws128'),
    'train_k1280_t65536_2d': ('ws128', False, 'train.ws128'),
    'train_k1280_t65536_3d_nc': ('library', False, 'not-16bit-inference'),
    'out_proj_n640_t8192_res_misaligned': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_res_pitch': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_res_batch_pitch': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_res_odd_pitch': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_gate_misaligned': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_gate_pitch+4': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_gate_pitch+8': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_no_residual': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_2d_residual': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_grad_mode': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t8192_fp16': ('sm', False, 'out_proj.sm'),
    'out_proj_n640_t16384_res_misaligned': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_res_pitch': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_res_batch_pitch': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_res_odd_pitch': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_gate_misaligned': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_gate_pitch+4': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_gate_pitch+8': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_no_residual': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_2d_residual': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_grad_mode': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t16384_fp16': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n640_t65536_res_misaligned': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_res_pitch': ('tiled', True, 'out_proj.tiled'),
    'out_proj_n640_t65536_res_batch_pitch': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_res_odd_pitch': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_gate_misaligned': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_gate_pitch+4': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_gate_pitch+8': ('tiled', True, 'out_proj.tiled'),
    'out_proj_n640_t65536_no_residual': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_2d_residual': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_grad_mode': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n640_t65536_fp16': ('tiled', True, 'out_proj.tiled'),
    'to_out_n640_t8192_res_misaligned': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_res_pitch': ('sm', True, 'to_out.sm'),
    'to_out_n640_t8192_res_batch_pitch': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_res_odd_pitch': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_gate_misaligned': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_gate_pitch+4': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_gate_pitch+8': ('sm', True, 'to_out.sm'),
    'to_out_n640_t8192_no_residual': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_2d_residual': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_grad_mode': ('sm', False, 'to_out.sm'),
    'to_out_n640_t8192_fp16': ('sm', True, 'to_out.sm'),
    'to_out_n640_t16384_res_misaligned': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_res_pitch': ('tiled', True, 'to_out.tiled'),
    'to_out_n640_t16384_res_batch_pitch': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_res_odd_pitch': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_gate_misaligned': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_gate_pitch+4': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_gate_pitch+8': ('tiled', True, 'to_out.tiled'),
    'to_out_n640_t16384_no_residual': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_2d_residual': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_grad_mode': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t16384_fp16': ('tiled', True, 'to_out.tiled'),
    'to_out_n640_t65536_res_misaligned': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_res_pitch': ('tiled', True, 'to_out.tiled'),
    'to_out_n640_t65536_res_batch_pitch': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_res_odd_pitch': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_gate_misaligned': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_gate_pitch+4': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_gate_pitch+8': ('tiled', True, 'to_out.tiled'),
    'to_out_n640_t65536_no_residual': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_2d_residual': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_grad_mode': ('tiled', False, 'to_out.tiled'),
    'to_out_n640_t65536_fp16': ('tiled', True, 'to_out.tiled'),
    'out_proj_n768_t8192_res_misaligned': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_res_pitch': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_res_batch_pitch': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_res_odd_pitch': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_gate_misaligned': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_gate_pitch+4': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_gate_pitch+8': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_no_residual': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_2d_residual': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_grad_mode': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t8192_fp16': ('sm', False, 'out_proj.sm'),
    'out_proj_n768_t16384_res_misaligned': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_res_pitch': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_res_batch_pitch': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_res_odd_pitch': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_gate_misaligned': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_gate_pitch+4': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_gate_pitch+8': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_no_residual': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_2d_residual': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_grad_mode': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t16384_fp16': ('ws128', False, 'out_proj.ws128'),
    'out_proj_n768_t65536_res_misaligned': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_res_pitch': ('tiled', True, 'out_proj.tiled'),
    'out_proj_n768_t65536_res_batch_pitch': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_res_odd_pitch': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_gate_misaligned': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_gate_pitch+4': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_gate_pitch+8': ('tiled', True, 'out_proj.tiled'),
    'out_proj_n768_t65536_no_residual': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_2d_residual': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_grad_mode': ('tiled', False, 'out_proj.tiled'),
    'out_proj_n768_t65536_fp16': ('tiled', True, 'out_proj.tiled'),
    'fp32_highest_in_proj': ('library', False, 'not-16bit-inference'),
    'fp32_highest_out_proj': ('library', False, 'not-16bit-inference'),
    'fp32_highest_to_q': ('library', False, 'not-16bit-inference'),
    'fp32_highest_to_out': ('library', False, 'not-16bit-inference'),
    'fp32_highest_text': ('library', False, 'not-16bit-inference'),
    'fp32_highest_train': ('library', False, 'not-16bit-inference'),
    'fp32_highest_bias_8': ('library', False, 'not-16bit-inference'),
    'fp32_highest_x_pitch+4': ('library', False, 'not-16bit-inference'),
    'fp32_highest_x_pitch+2': ('library', False, 'not-16bit-inference'),
    'fp32_highest_3d_nc': ('library', False, 'not-16bit-inference'),
    'fp32_highest_tokens_100': ('library', False, 'not-16bit-inference'),
    'fp32_highest_n_100': ('library', False, 'not-16bit-inference'),
    'fp32_highest_grad': ('library', False, 'not-16bit-inference'),
    'fp32_highest_policy_off': ('library', False, 'not-16bit-inference'),
    'fp32_highest_mixed_bf16_x': ('library', False, 'not-16bit-inference'),
    'fp32_high_in_proj': ('split3', False, 'fp32.high'),
    'fp32_high_out_proj': ('split3', False, 'fp32.high'),
    'fp32_high_to_q': ('split3', False, 'fp32.high'),
    'fp32_high_to_out': ('split3', False, 'fp32.high'),
    'fp32_high_text': ('split3', False, 'fp32.high'),
    'fp32_high_train': ('split3', False, 'fp32.high'),
    'fp32_high_bias_8': ('library', False, 'not-16bit-inference'),
    'fp32_high_x_pitch+4': ('split3', False, 'fp32.high'),
    'fp32_high_x_pitch+2': ('library', False, 'not-16bit-inference'),
    'fp32_high_3d_nc': ('library', False, 'not-16bit-inference'),
    'fp32_high_tokens_100': ('library', False, 'not-16bit-inference'),
    'fp32_high_n_100': ('library', False, 'not-16bit-inference'),
    'fp32_high_grad': ('library', False, 'not-16bit-inference'),
    'fp32_high_policy_off': ('library', False, 'not-16bit-inference'),
    'fp32_high_mixed_bf16_x': ('library', False, 'not-16bit-inference'),
    'fp32_medium_in_proj': ('split1', False, 'fp32.medium'),
    'fp32_medium_out_proj': ('split1', False, 'fp32.medium'),
    'fp32_medium_to_q': ('split1', False, 'fp32.medium'),
    'fp32_medium_to_out': ('split1', False, 'fp32.medium'),
    'fp32_medium_text': ('split1', False, 'fp32.medium'),
    'fp32_medium_train': ('split1', False, 'fp32.medium'),
    'fp32_medium_bias_8': ('library', False, 'not-16bit-inference'),
    'fp32_medium_x_pitch+4': ('split1', False, 'fp32.medium'),
    'fp32_medium_x_pitch+2': ('library', False, 'not-16bit-inference'),
    'fp32_medium_3d_nc': ('library', False, 'not-16bit-inference'),
    'fp32_medium_tokens_100': ('library', False, 'not-16bit-inference'),
    'fp32_medium_n_100': ('library', False, 'not-16bit-inference'),
    'fp32_medium_grad': ('library', False, 'not-16bit-inference'),
    'fp32_medium_policy_off': ('library', False, 'not-16bit-inference'),
    'fp32_medium_mixed_bf16_x': ('library', False, 'not-16bit-inference'),
    'autocast_bf16_in_proj_t8192': ('ws', False, 'in_proj.ws'),
    'autocast_bf16_in_proj_t65536': ('ws', False, 'in_proj.ws'),
    'autocast_bf16_out_proj_t8192': ('sm', False, 'out_proj.sm'),
    'autocast_bf16_out_proj_t65536': ('tiled', True, 'out_proj.tiled'),
    'autocast_bf16_to_q_t8192': ('sm', False, 'to_q.sm'),
    'autocast_bf16_to_q_t65536': ('tiled', False, 'to_q.tiled'),
    'autocast_bf16_to_out_t8192': ('sm', True, 'to_out.sm'),
    'autocast_bf16_to_out_t65536': ('tiled', True, 'to_out.tiled'),
    'autocast_bf16_text_t8192': ('tiled', False, 'text.tiled'),
    'autocast_bf16_text_t65536': ('tiled', False, 'text.tiled'),
    'autocast_bf16_train_t8192': ('ws', False, 'train.ws'),
    'autocast_bf16_train_t65536': ('ws', False, 'train.ws'),
    'autocast_bf16_param_grad': ('library', False, 'autograd'),
    'autocast_bf16_param_grad_off': ('ws', False, 'in_proj.ws'),
    'autocast_bf16_grad_mode_frozen': ('tiled', False, 'out_proj.tiled'),
    'autocast_bf16_fp32_x': ('library', False, 'not-16bit-inference'),
    'autocast_bf16_other_16bit_x': ('library', False, 'not-16bit-inference'),
    'autocast_bf16_16bit_weight': ('ws', False, 'in_proj.ws'),
    'autocast_fp16_in_proj_t8192': ('ws', False, 'in_proj.ws'),
    'autocast_fp16_in_proj_t65536': ('ws', False, 'in_proj.ws'),
    'autocast_fp16_out_proj_t8192': ('sm', False, 'out_proj.sm'),
    'autocast_fp16_out_proj_t65536': ('tiled', True, 'out_proj.tiled'),
    'autocast_fp16_to_q_t8192': ('sm', False, 'to_q.sm'),
    'autocast_fp16_to_q_t65536': ('tiled', False, 'to_q.tiled'),
    'autocast_fp16_to_out_t8192': ('sm', True, 'to_out.sm'),
    'autocast_fp16_to_out_t65536': ('tiled', True, 'to_out.tiled'),
    'autocast_fp16_text_t8192': ('tiled', False, 'text.tiled'),
    'autocast_fp16_text_t65536': ('tiled', False, 'text.tiled'),
    'autocast_fp16_train_t8192': ('ws', False, 'train.ws'),
    'autocast_fp16_train_t65536': ('ws', False, 'train.ws'),
    'autocast_fp16_param_grad': ('library', False, 'autograd'),
    'autocast_fp16_param_grad_off': ('ws', False, 'in_proj.ws'),
    'autocast_fp16_grad_mode_frozen': ('tiled', False, 'out_proj.tiled'),
    'autocast_fp16_fp32_x': ('library', False, 'not-16bit-inference'),
    'autocast_fp16_other_16bit_x': ('library', False, 'not-16bit-inference'),
    'autocast_fp16_16bit_weight': ('ws', False, 'in_proj.ws'),
    'grad_x_t8192': ('library', False, 'not-16bit-inference'),
    'grad_w_t8192': ('library', False, 'not-16bit-inference'),
    'no_grad_w_requires_grad_t8192': ('ws', False, 'in_proj.ws'),
    'grad_mode_nothing_requires_t8192': ('ws', False, 'in_proj.ws'),
    'cpu_t8192': ('library', False, 'not-16bit-inference'),
    'mixed_16bit_t8192': ('library', False, 'not-16bit-inference'),
    'tokens_odd_t8192': ('library', False, 'not-16bit-inference'),
    'tokens_plus_8_t8192': ('tiled', False, 'to_q.tiled'),
    'n_100_t8192': ('library', False, 'not-16bit-inference'),
    'k_100_t8192': ('library', False, 'not-16bit-inference'),
    'policy_all_in_proj_t8192': ('tiled', False, 'policy.all'),
    'policy_all_out_proj_t8192': ('tiled', True, 'policy.all'),
    'policy_all_to_q_t8192': ('tiled', False, 'policy.all'),
    'policy_all_to_out_t8192': ('tiled', True, 'policy.all'),
    'policy_all_text_t8192': ('tiled', False, 'text.tiled'),
    'policy_all_train_t8192': ('ws', False, 'train.ws'),
    'policy_all_in_proj_n_100_t8192': ('library', False, 'not-16bit-inference'),
    'policy_all_to_out_res_misaligned_t8192': ('tiled', False, 'policy.all'),
    'policy_off_in_proj_t8192': ('library', False, 'policy.off'),
    'policy_off_out_proj_t8192': ('library', False, 'policy.off'),
    'policy_off_to_q_t8192': ('library', False, 'policy.off'),
    'policy_off_to_out_t8192': ('library', False, 'policy.off'),
    'policy_off_text_t8192': ('library', False, 'policy.off'),
    'policy_off_train_t8192': ('library', False, 'policy.off'),
    'policy_off_in_proj_n_100_t8192': ('library', False, 'not-16bit-inference'),
    'policy_off_to_out_res_misaligned_t8192': ('library', False, 'policy.off'),
    'disabled_in_proj.ws_in_proj_t8192': ('library', False, 'in_proj.library'),
    'disabled_in_proj.ws_out_proj_t8192': ('sm', False, 'out_proj.sm'),
    'disabled_in_proj.ws+in_proj.halves_in_proj_t8192': ('library', False, 'in_proj.library'),
    'disabled_in_proj.ws+in_proj.halves_out_proj_t8192': ('sm', False, 'out_proj.sm'),
    'disabled_out_proj.sm+out_proj.tiled_in_proj_t8192': ('ws', False, 'in_proj.ws'),
    'disabled_out_proj.sm+out_proj.tiled_out_proj_t8192': ('library', False, 'out_proj.library'),
    'wgrad_dx_n2560_k640_t8192': ('ws', False, 'train.ws'),
    'wgrad_dx_n2560_k640_t8192_fp16': ('ws', False, 'train.ws'),
    'wgrad_dx_n640_k2560_t8192': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n640_k2560_t8192_fp16': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n640_k1280_t8192': ('ws128', False, 'train.ws128'),
    'wgrad_dx_n640_k1280_t8192_fp16': ('ws128', False, 'train.ws128'),
    'wgrad_dx_n1280_k640_t8192': ('ws', False, 'train.ws'),
    'wgrad_dx_n1280_k640_t8192_fp16': ('ws', False, 'train.ws'),
    'wgrad_dx_n512_k640_t8192': ('ws', False, 'train.ws'),
    'wgrad_dx_n512_k640_t8192_fp16': ('ws', False, 'train.ws'),
    'wgrad_dx_n640_k512_t8192': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n640_k512_t8192_fp16': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n3072_k768_t8192': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n3072_k768_t8192_fp16': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n100_k640_t8192': ('library', False, 'not-16bit-inference'),
    'wgrad_dx_n100_k640_t8192_fp16': ('library', False, 'not-16bit-inference'),
    'grad_x_t65536': ('library', False, 'not-16bit-inference'),
    'grad_w_t65536': ('library', False, 'not-16bit-inference'),
    'no_grad_w_requires_grad_t65536': ('ws', False, 'in_proj.ws'),
    'grad_mode_nothing_requires_t65536': ('ws', False, 'in_proj.ws'),
    'cpu_t65536': ('library', False, 'not-16bit-inference'),
    'mixed_16bit_t65536': ('library', False, 'not-16bit-inference'),
    'tokens_odd_t65536': ('library', False, 'not-16bit-inference'),
    'tokens_plus_8_t65536': ('tiled', False, 'to_q.tiled'),
    'n_100_t65536': ('library', False, 'not-16bit-inference'),
    'k_100_t65536': ('library', False, 'not-16bit-inference'),
    'policy_all_in_proj_t65536': ('tiled', False, 'policy.all'),
    'policy_all_out_proj_t65536': ('tiled', True, 'policy.all'),
    'policy_all_to_q_t65536': ('tiled', False, 'policy.all'),
    'policy_all_to_out_t65536': ('tiled', True, 'policy.all'),
    'policy_all_text_t65536': ('tiled', False, 'text.tiled'),
    'policy_all_train_t65536': ('ws', False, 'train.ws'),
    'policy_all_in_proj_n_100_t65536': ('library', False, 'not-16bit-inference'),
    'policy_all_to_out_res_misaligned_t65536': ('tiled', False, 'policy.all'),
    'policy_off_in_proj_t65536': ('library', False, 'policy.off'),
    'policy_off_out_proj_t65536': ('library', False, 'policy.off'),
    'policy_off_to_q_t65536': ('library', False, 'policy.off'),
    'policy_off_to_out_t65536': ('library', False, 'policy.off'),
    'policy_off_text_t65536': ('library', False, 'policy.off'),
    'policy_off_train_t65536': ('library', False, 'policy.off'),
    'policy_off_in_proj_n_100_t65536': ('library', False, 'not-16bit-inference'),
    'policy_off_to_out_res_misaligned_t65536': ('library', False, 'policy.off'),
    'disabled_in_proj.ws_in_proj_t65536': ('tiled_halves', False, 'in_proj.halves'),
    'disabled_in_proj.ws_out_proj_t65536': ('tiled', True, 'out_proj.tiled'),
    'disabled_in_proj.ws+in_proj.halves_in_proj_t65536': ('library', False, 'in_proj.library'),
    'disabled_in_proj.ws+in_proj.halves_out_proj_t65536': ('tiled', True, 'out_proj.tiled'),
    'disabled_out_proj.sm+out_proj.tiled_in_proj_t65536': ('ws', False, 'in_proj.ws'),
    'disabled_out_proj.sm+out_proj.tiled_out_proj_t65536': ('library', False, 'out_proj.library'),
    'wgrad_dx_n2560_k640_t65536': ('ws', False, 'train.ws'),
    'wgrad_dx_n2560_k640_t65536_fp16': ('ws', False, 'train.ws'),
    'wgrad_dx_n640_k2560_t65536': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n640_k2560_t65536_fp16': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n640_k1280_t65536': ('ws128', False, 'train.ws128'),
    'wgrad_dx_n640_k1280_t65536_fp16': ('ws128', False, 'train.ws128'),
    'wgrad_dx_n1280_k640_t65536': ('ws', False, 'train.ws'),
    'wgrad_dx_n1280_k640_t65536_fp16': ('ws', False, 'train.ws'),
    'wgrad_dx_n512_k640_t65536': ('ws', False, 'train.ws'),
    'wgrad_dx_n512_k640_t65536_fp16': ('ws', False, 'train.ws'),
    'wgrad_dx_n640_k512_t65536': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n640_k512_t65536_fp16': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n3072_k768_t65536': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n3072_k768_t65536_fp16': ('tiled', False, 'train.tiled'),
    'wgrad_dx_n100_k640_t65536': ('library', False, 'not-16bit-inference'),
    'wgrad_dx_n100_k640_t65536_fp16': ('library', False, 'not-16bit-inference'),
}

# the cases of GATED_CASES the predicate accepts, recorded on the parent commit
GATED_ACCEPTED = {
    'plain', 'fp16', 'rows_512', 'one_sample', 'res_pitch+8', 'res_pitch+128', 'res_16_bytes_off', 'gate_16_bytes_off', 'gate_pitch+8', 'res_pitch_2^22-8'
}

# the cases of NORM_LINEAR_CASES the predicate accepts, recorded on the parent commit
NORM_LINEAR_ACCEPTED = {
    'plain', 'fp16', 'k512', 'k768', 'L128', 'L64_B2', 'L96_B4', 'x_pitch+8', 'w_pitch+8', 'mod_pitch_k', 'mod_pitch_0', 'x_16_bytes_off', 'scale_16_bytes_off', 'x_pitch_2^27-8', 'w_pitch_2^27-8'
}

# the cases of SPLIT_CASES the predicate accepts, recorded on the parent commit
SPLIT_ACCEPTED = {
    'plain', '3d', 'bias', 'no_grad_w_requires', 'grad_mode_nothing_requires', 'k_64', 'k_65536', 'n_128', 'n_65536', 'tokens_8', 'tiles_2^31', 'tiles_below_2^31', 'x_pitch+4', 'x_16_bytes_off'
}


if __name__ == "__main__":
    from zigma_amd.fp32_matmul import split_eligible
    from zigma_amd.linear import gated_residual_eligible, plan
    from zigma_amd.norm_linear import norm_linear_eligible
    print("# case: (kernel, fuse_add, row), recorded on the parent commit\nEXPECTED = {")
    for name, case in CASES.items():
        print(f"    {name!r}: {call(plan, case)!r},")
    print("}")
    for title, cases, fn, pred in (("GATED", GATED_CASES, call_gated, gated_residual_eligible), ("NORM_LINEAR", NORM_LINEAR_CASES, call_norm_linear, norm_linear_eligible),
                                   ("SPLIT", SPLIT_CASES, call_split, split_eligible)):
        print(f"\n# the cases of {title}_CASES the predicate accepts, recorded on the parent commit\n{title}_ACCEPTED = {{")
        print("    " + ", ".join(repr(name) for name, case in cases.items() if fn(pred, case)))
        print("}")
