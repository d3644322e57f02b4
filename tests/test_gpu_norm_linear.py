"""zigma_norm_linear_fwd (csrc/norm_linear.hip) on the GPU: LayerNorm + adaLN modulate + to_q in one kernel, at the smallest shapes where it can go wrong,
against float64 on the same 16-bit operands and against the two-kernel pair it replaces; the plan's refusals; the block's engagement at 65 536 tokens."""
import ast
import ctypes

import pytest
import torch

from conftest import load_golden
from norm_linear_cases import CASES, OK, make_params
from oracle.param_fill import fill_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from zigma_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()


def _inputs(m, k, rpb, dtype, seed):
    """rows with a per-row offset and scale — mean up to +-8 standard deviations, standard deviations over two decades (an E[x^2] - mean^2 shortcut
    or a dropped lane-pair exchange fails visibly) — and shift / scale rows as strided column slices of a (B, 6k) tensor, as the block passes them"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    std = 10.0 ** (torch.rand(m, 1, generator=g) * 2 - 1)
    mean = (torch.rand(m, 1, generator=g) * 16 - 8) * std
    x = (mean + std * torch.randn(m, k, generator=g)).to(DEV, dtype).view(m // rpb, rpb, k)
    w = (torch.randn(512, k, generator=g) * k ** -0.5).to(DEV, dtype)
    mod = (torch.randn(m // rpb, 6 * k, generator=g) * 0.5).to(DEV, dtype)
    return x, w, mod[:, 3 * k:4 * k], mod[:, 4 * k:5 * k]


def _float64(x, w, shift, scale, dtype):
    """LayerNorm -> round -> modulate -> round -> product, in float64 on the same 16-bit operands"""
    r16 = lambda t: t.to(torch.float32).to(dtype).double()
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    y = r16((xd - mean) / torch.sqrt(var + EPS))
    xa = r16(y * (1 + scale.double().unsqueeze(1)) + shift.double().unsqueeze(1))
    return xa.reshape(-1, x.shape[-1]) @ w.double().T


@pytest.mark.parametrize("m,k,rpb,dtype,sliced", [
    (128, 640, 128, torch.bfloat16, False),       # one tile, one sample
    (384, 640, 128, torch.bfloat16, False),       # odd tile count, three samples with different shift / scale rows
    (384, 640, 96, torch.bfloat16, False),        # tiles straddling sample boundaries (per-row batch index)
    (1152, 512, 384, torch.bfloat16, False),      # the other two k instantiations, several tiles
    (1152, 768, 384, torch.bfloat16, False),
    (256, 640, 256, torch.float16, True),         # fp16; output into a column slice of a wider buffer
])
def test_norm_linear_kernel_vs_float64(m, k, rpb, dtype, sliced):
    """every output against float64 under the bars of a 16-bit projection (test_linear_kernel_vs_float64: norm-wise < 2.5e-3, allclose(1.6e-2, 1e-2) — an
    xa element whose 16-bit rounding falls the other way moves an output by about 2^-8 |xa w| ~ 1e-4, far inside one output ulp); against the pair
    zigma_add_norm_fwd + zigma_linear_fwd under the same norm-wise bar (share of bit-equal elements printed); two launches bit-identical; kernel name."""
    from zigma_amd import _lib
    from zigma_amd.layernorm import block_norm
    from zigma_amd.linear import linear
    from zigma_amd.norm_linear import norm_linear, norm_linear_eligible
    x, w, shift, scale = _inputs(m, k, rpb, dtype, seed=m + k + rpb)
    assert shift.stride(0) == 6 * k and norm_linear_eligible(x, w, shift, scale)
    if sliced:
        wide = torch.full((m, 512 + 128), 3.0, device=DEV, dtype=dtype)
        norm_linear(x, w, shift, scale, EPS, out=wide[:, 64:64 + 512])
        got = wide[:, 64:64 + 512].clone()
        assert float((wide[:, :64] - 3).abs().max()) == 0 and float((wide[:, 64 + 512:] - 3).abs().max()) == 0      # bytes beside the slice untouched
    else:
        got = norm_linear(x, w, shift, scale, EPS).view(m, 512)
    assert _lib.last_kernel() == f"norm_linear_k{k}"
    ref = _float64(x, w, shift, scale, dtype)
    e = float((got.double() - ref).norm() / ref.norm())
    _, _, _, xa = block_norm(x, None, None, None, EPS, False, residual_in_fp32=False, shift=shift, scale=scale, want_x=True, want_y=False, want_res_out=False)
    pair = linear(xa, w).view(m, 512)
    e_pair = float((got.double() - pair.double()).norm() / pair.double().norm())
    print(f"norm_linear {m}x{k} rpb {rpb} {dtype}: vs float64 {e:.3e}, vs pair {e_pair:.3e}, bit-equal with the pair {float((got == pair).float().mean()):.4f}")
    assert e < 2.5e-3
    assert torch.allclose(got.double(), ref, rtol=1.6e-2, atol=1e-2)
    assert e_pair < 2.5e-3
    again = norm_linear(x, w, shift, scale, EPS).view(m, 512)
    assert torch.equal(again, got)                  # a synchronisation slip in the weight ring shows as flicker


def test_norm_linear_refusals_launch_nothing():
    """the refusals of the case table: the library returns the plan's status and leaves the output alone"""
    from zigma_amd import _lib
    L = _lib.lib()
    x, w, shift, scale = _inputs(384, 640, 128, torch.bfloat16, seed=1)
    mod = torch.zeros(8, 6 * 640 + 64, device=DEV, dtype=torch.bfloat16)
    out = torch.full((384 * 1024 + 64,), 5.0, device=DEV, dtype=torch.bfloat16)
    ptrs = dict(x=x.data_ptr(), w=w.data_ptr(), shift=mod.data_ptr(), scale=mod[:, 640:].data_ptr(), out=out.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    n = 0
    for name, ov, status, kernel in CASES:
        if kernel is not None:
            continue
        P = make_params(_lib.NormLinearParams, ov, ptrs)
        assert L.zigma_norm_linear_fwd(ctypes.byref(P), ctypes.c_void_p(stream)) == status, name
        n += status != OK
    torch.cuda.synchronize()
    assert n >= 30 and float((out - 5).abs().max()) == 0
    assert L.zigma_norm_linear_fwd(None, ctypes.c_void_p(stream)) == -1


def readme_model(depth):
    from zigma_amd.model_zigma import ZigMa
    g = load_golden("r2_readme_b2.npz")
    cfg = dict(ast.literal_eval(str(g["cfg"])), depth=depth)
    m = ZigMa(device="cpu", dtype=torch.bfloat16, **cfg)
    fill_state(m, int(g["seed"]))
    gen = torch.Generator().manual_seed(7)
    Bsz = 64
    x = torch.randn(Bsz, *g["x"].shape[1:], generator=gen)
    t = torch.rand(Bsz, generator=gen)
    y = torch.rand(Bsz, *g["y"].shape[1:], generator=gen)
    return m.to(DEV).eval(), cfg, (x.to(DEV).bfloat16(), t.to(DEV).bfloat16(), y.to(DEV).bfloat16())


def run_traced(m, args, monkeypatch, **knobs):
    import zigma_amd.model_zigma as mz
    from zigma_amd import _lib
    for k, v in knobs.items():
        monkeypatch.setattr(mz, k, v)
    trace = []
    monkeypatch.setattr(_lib, "TRACE", trace)
    with torch.no_grad():
        out = m(*args)
    monkeypatch.setattr(_lib, "TRACE", None)
    counts = {}
    for fn, _, _ in trace:
        counts[fn] = counts.get(fn, 0) + 1
    return out.double(), counts


MODEL_DISTANCE = 2.53e-3             # FUSE_OUT_PROJ_ADD on vs off with FUSE_NORM_TO_Q = False, this model and input (measured 2026-10-19 on an MI355X: 2.527e-3)
MODEL_BAR = 1.5 * MODEL_DISTANCE     # 3.79e-3; FUSE_NORM_TO_Q on vs off measured 7.7e-4 the same day


def test_block_takes_the_fused_kernel_at_65536_tokens(monkeypatch):
    """README configuration with depth 2 at B = 64 (65 536 tokens, the smallest batch at which the engagement gate opens): from the call trace one
    zigma_norm_linear_fwd per block, one zigma_add_norm_fwd fewer per block than with FUSE_NORM_TO_Q = False, zigma_linear_fwd == 3 depth + 2; the output
    norm-wise against the same model with the knob off.
    The bar is 1.5 x the mutual distance of the knob-off model's two existing compositions (FUSE_OUT_PROJ_ADD on / off), the project's own measure of
    "same result, rounded at other points".  Measured 2026-10-19 on an MI355X: distance 2.53e-3, so the bar is 3.79e-3; the fused path sits at 7.7e-4
    from the knob-off model."""
    m, cfg, args = readme_model(depth=2)
    depth = cfg["depth"]
    on, c_on = run_traced(m, args, monkeypatch, FUSE_NORM_TO_Q=True)
    off, c_off = run_traced(m, args, monkeypatch, FUSE_NORM_TO_Q=False)
    assert c_on.get("zigma_norm_linear_fwd", 0) == depth and c_off.get("zigma_norm_linear_fwd", 0) == 0, (c_on, c_off)
    assert c_on["zigma_add_norm_fwd"] == c_off["zigma_add_norm_fwd"] - depth, (c_on, c_off)
    assert c_on["zigma_linear_fwd"] == 3 * depth + 2 and c_off["zigma_linear_fwd"] == 4 * depth + 2, (c_on, c_off)
    e = float((on - off).norm() / off.norm())
    print(f"README depth {depth}, B = 64: FUSE_NORM_TO_Q on vs off {e:.3e} (bar {MODEL_BAR:.3e})")
    assert e < MODEL_BAR
