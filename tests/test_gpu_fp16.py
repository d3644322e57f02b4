"""GPU tests of the fp16 forms of the matrix-core kernels: an fp16 model's block loop runs the kernels, routes and fusions of the bf16 model's.

Every case runs on fp16 operands.  The kernel-level cases mirror the bf16 originals of tests/test_gpu_parity.py (same parameter lists, same
structure) with fp16 rounding (numpy float16, round to nearest even) in the oracles.  Bounds are the bf16 bounds of the same check divided by 8:
fp16 carries three more mantissa bits than bf16 (11 against 8 significant bits).  With the tests' input distributions (x ~ N(0, 1), w ~ N(0, 1/k),
fp32 accumulation, one rounding) the rounding floor alone is 2.08e-4 norm-wise for a plain product, 2.54e-4 with the fused gated add and 3.03e-4
with the unfused add (bf16: 1.66e-3 / 2.03e-3 / 2.42e-3), so each bound keeps the >= 1.2 x room over the floor its bf16 original has."""
import ast

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import zigma_oracle as zo
from oracle.param_fill import fill_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = torch.float16
ERR_DTYPE = -3                      # ZIGMA_ERR_DTYPE (include/zigma_hip.h)


def r16(a):
    """fp16 rounding of the oracles (round to nearest even), as float32"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def T(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def N(t):
    return t.detach().float().cpu().numpy()


def nerr(got, ref):
    return float((got - ref).norm() / ref.norm())


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from zigma_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()


# ---------------------------------------------------------------------------------------------------
# 1. kernels vs float64 (+ 2. the families bit-identical with the 8-wave tiled kernel)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N_,bias,act", [(4096, 640, 2560, False, 1280), (2048, 1280, 640, False, None), (1040, 640, 512, False, None),
                                            (4096, 512, 640, True, None), (16, 64, 128, True, 64), (272, 128, 384, True, None),
                                            (65536, 640, 2560, False, 1280), (4096, 768, 3072, False, None), (65536, 768, 3072, False, 1536),
                                            (2048, 1536, 768, False, None)])
def test_linear_kernel_vs_float64(M, K, N_, bias, act, monkeypatch):
    """zigma_linear_fwd's 8-wave tiled kernel on fp16: every output against float64 on the same operands (bias before the single rounding;
    SiLU on columns >= act), ragged token counts, a strided output."""
    from zigma_amd import _lib
    import zigma_amd.routing as zr
    from zigma_amd.linear import linear, linear_eligible
    monkeypatch.setattr(zr, "POLICY", "all")
    g = torch.Generator(device="cpu").manual_seed(M + N_)
    x = torch.randn(M, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H)
    b = (torch.randn(N_, generator=g) * 0.5).to(DEV, H) if bias else None
    assert linear_eligible(x, w, b)
    y = linear(x, w, b, act)
    assert _lib.last_kernel().startswith("linear_tn_") and y.shape == (M, N_) and y.dtype == H
    rows = torch.arange(M, device=DEV) if M <= 4096 else torch.randint(0, M, (2048,), generator=g).to(DEV)
    ref = x[rows].double() @ w.double().T + (b.double() if bias else 0)
    if act is not None:
        ref[:, act:] = torch.nn.functional.silu(ref[:, act:])
    got = y[rows].double()
    e = nerr(got, ref)
    print(f"linear_tn f16 {M}x{K}x{N_}: {e:.3e}")
    assert e < 3.1e-4
    assert torch.allclose(got, ref, rtol=2e-3, atol=1.25e-3)
    if M <= 4096:
        wide = torch.zeros(M, N_ + 128, device=DEV, dtype=H)
        linear(x, w, b, act, out=wide[:, 64:64 + N_])
        assert torch.equal(wide[:, 64:64 + N_], y) and float(wide[:, :64].abs().max()) == 0 and float(wide[:, 64 + N_:].abs().max()) == 0


@pytest.mark.parametrize("M,K,N_", [(65536, 640, 2560), (65536, 640, 512), (16384, 192, 4096), (65536, 1280, 256), (32768, 512, 1024),
                                    (65536, 768, 3072), (8192, 768, 3072), (16384, 768, 3072), (65536, 1536, 768), (65536, 768, 512)])
def test_linear4w_kernel(M, K, N_, monkeypatch):
    """The generated 4-wave loop in its f16 form: sampled rows against float64, torch.equal with the 8-wave kernel (same MFMA, same accumulation
    order; this pins v_cvt_pk_f16_f32 of the generated text against from_float<F16> = round to nearest even), run-to-run identity, strided output."""
    from zigma_amd import _lib
    import zigma_amd.routing as zr
    from zigma_amd.linear import linear, linear_eligible
    from zigma_amd.routing import serves_4w
    g = torch.Generator(device="cpu").manual_seed(M + N_ + K)
    x = torch.randn(M, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H)
    assert serves_4w(M, N_, K)
    monkeypatch.setattr(zr, "POLICY", "all")
    assert linear_eligible(x, w, None)
    y = linear(x, w)
    assert _lib.last_kernel() == "linear4w_256x256" and y.shape == (M, N_)
    rows = torch.randint(0, M, (1024,), generator=g).to(DEV)
    rows[:4] = torch.tensor([0, 255, 256, M - 1], device=DEV)
    ref = x[rows].double() @ w.double().T
    got = y[rows].double()
    e = nerr(got, ref)
    print(f"linear4w f16 {M}x{K}x{N_}: {e:.3e}")
    assert e < 3.1e-4
    assert torch.allclose(got, ref, rtol=2e-3, atol=1.25e-3)
    y8 = linear(x, w, _probe_flags=0x2000)
    assert _lib.last_kernel().startswith("linear_tn_")
    assert torch.equal(y, y8)
    for _ in range(4):
        assert torch.equal(linear(x, w), y)
    if N_ <= 1024:
        wide = torch.zeros(M, N_ + 256, device=DEV, dtype=H)
        linear(x, w, out=wide[:, 128:128 + N_])
        assert _lib.last_kernel() == "linear4w_256x256"
        assert torch.equal(wide[:, 128:128 + N_], y) and float(wide[:, :128].abs().max()) == 0 and float(wide[:, 128 + N_:].abs().max()) == 0


@pytest.mark.parametrize("M,K,N_", [(65536, 640, 2560), (65536, 640, 512), (32768, 640, 2560), (4096, 640, 8192), (5632, 512, 1024), (512 * 43, 512, 256),
                                    (16384, 640, 1280), (8192, 1280, 640), (16384, 1536, 768), (65536, 1280, 640), (512 * 33, 1536, 128), (8192, 1536, 768)])
def test_linear_ws_kernel(M, K, N_):
    """The weight-stationary kernel on fp16: sampled rows against float64; the WHOLE result torch.equal with the tiled kernel; run-to-run
    identity; strided output and input."""
    from zigma_amd import _lib
    from zigma_amd.linear import linear, linear_ws_eligible
    g = torch.Generator(device="cpu").manual_seed(M + N_ + K)
    x = torch.randn(M, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H)
    assert linear_ws_eligible(x, w)
    y = linear(x, w, weight_stationary=True)
    kname = "linear_ws" if K <= 640 else "linear_ws_128"
    assert _lib.last_kernel() == kname and y.shape == (M, N_)
    rows = torch.randint(0, M, (1024,), generator=g).to(DEV)
    rows[:6] = torch.tensor([0, 63, 64, 511, 512, M - 1], device=DEV)
    ref = x[rows].double() @ w.double().T
    got = y[rows].double()
    e = nerr(got, ref)
    print(f"linear_ws f16 {M}x{K}x{N_}: {e:.3e}")
    assert e < 3.1e-4
    assert torch.allclose(got, ref, rtol=2e-3, atol=1.25e-3)
    y8 = linear(x, w, _probe_flags=0x2000)
    assert _lib.last_kernel().startswith("linear_tn_")
    assert torch.equal(y, y8)
    for _ in range(4):
        assert torch.equal(linear(x, w, weight_stationary=True), y)
    wide = torch.zeros(M, N_ + 256, device=DEV, dtype=H)
    linear(x, w, out=wide[:, 128:128 + N_], weight_stationary=True)
    assert _lib.last_kernel() == kname
    assert torch.equal(wide[:, 128:128 + N_], y) and float(wide[:, :128].abs().max()) == 0 and float(wide[:, 128 + N_:].abs().max()) == 0
    xs = torch.zeros(M, K + 128, device=DEV, dtype=H)
    xs[:, :K] = x
    assert torch.equal(linear(xs[:, :K], w, weight_stationary=True), y)


@pytest.mark.parametrize("M,K,N_,col", [(65536, 640, 2560, 1280), (16384, 640, 1280, 640), (5632, 512, 1024, 256), (8192, 640, 512, 0)])
def test_linear_ws_silu_epilogue(M, K, N_, col):
    """linear_ws_kernel<.., SL> on fp16: columns >= silu_from_col leave as silu(.) of the fp32 accumulator, the columns below are bit-identical
    with the plain kernel; float64 reference; run-to-run identity.  (4e-3 / 8 against silu of the ROUNDED product: one fp16 rounding apart.)"""
    from zigma_amd import _lib
    from zigma_amd.linear import linear
    g = torch.Generator(device="cpu").manual_seed(M + N_ + K + 1)
    x = torch.randn(M, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * 2.0 * K ** -0.5).to(DEV, H)
    y0 = linear(x, w, weight_stationary=True)
    y = linear(x, w, weight_stationary=True, silu_from_col=col)
    assert _lib.last_kernel() == "linear_ws_silu"
    assert torch.equal(y[:, :col], y0[:, :col])
    rows = torch.randint(0, M, (1024,), generator=g).to(DEV)
    rows[:6] = torch.tensor([0, 63, 64, 511, 512, M - 1], device=DEV)
    acc = x[rows].double() @ w.double().T
    ref = torch.nn.functional.silu(acc[:, col:])
    got = y[rows][:, col:].double()
    e = nerr(got, ref)
    print(f"linear_ws_silu f16 {M}x{K}x{N_}: {e:.3e}")
    assert e < 3.1e-4
    assert torch.allclose(got, ref, rtol=2e-3, atol=1.25e-3)
    ref2 = torch.nn.functional.silu(y0[:, col:].float())
    assert nerr(y[:, col:].float(), ref2) < 4e-3 / 8
    assert torch.equal(linear(x, w, weight_stationary=True, silu_from_col=col), y)
    with pytest.raises(RuntimeError):
        linear(x, w, weight_stationary=True, silu_from_col=col + 64)


@pytest.mark.parametrize("M,K,N_", [(8192, 1280, 640), (16384, 1536, 768), (128, 128, 640), (384, 192, 768), (8192, 512, 640), (2048, 1280, 1920),
                                    (4096 + 128, 640, 1280), (8192, 640, 512), (16384, 640, 2560)])
def test_linear_sm_kernel(M, K, N_):
    """The few-token tiled kernel on fp16: sampled rows against float64; the WHOLE result torch.equal with the 8-wave tiled kernel; run-to-run
    identity; strided output; the limits."""
    from zigma_amd import _lib
    from zigma_amd.linear import linear, linear_sm_eligible
    g = torch.Generator(device="cpu").manual_seed(M + N_ + K + 7)
    x = torch.randn(M, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H)
    assert linear_sm_eligible(x, w)
    y = linear(x, w, few_tokens=True)
    assert _lib.last_kernel() == ("linear_sm_128x160" if N_ % 160 == 0 else "linear_sm_128x192" if N_ % 192 == 0 else "linear_sm_128x128") and y.shape == (M, N_)
    rows = torch.randint(0, M, (min(M, 1024),), generator=g).to(DEV)
    rows[:4] = torch.tensor([0, 31, 127, M - 1], device=DEV)
    ref = x[rows].double() @ w.double().T
    got = y[rows].double()
    e = nerr(got, ref)
    print(f"linear_sm f16 {M}x{K}x{N_}: {e:.3e}")
    assert e < 3.1e-4
    assert torch.allclose(got, ref, rtol=2e-3, atol=1.25e-3)
    y8 = linear(x, w, _probe_flags=0x2000)
    assert _lib.last_kernel().startswith("linear_tn_")
    assert torch.equal(y, y8)
    for _ in range(3):
        assert torch.equal(linear(x, w, few_tokens=True), y)
    wide = torch.zeros(M, N_ + 256, device=DEV, dtype=H)
    linear(x, w, out=wide[:, 128:128 + N_], few_tokens=True)
    assert torch.equal(wide[:, 128:128 + N_], y) and float(wide[:, :128].abs().max()) == 0 and float(wide[:, 128 + N_:].abs().max()) == 0
    assert not linear_sm_eligible(x[:104], w) and not linear_sm_eligible(x, w[:96])
    with pytest.raises(RuntimeError):
        linear(x[:104], w, few_tokens=True)


@pytest.mark.parametrize("Bsz,L,K,N_,bias,res", [(8, 1024, 1280, 640, False, True), (16, 1024, 512, 640, True, True), (8, 1024, 1536, 768, False, True),
                                                  (4, 512, 512, 640, True, False), (2, 256, 256, 1280, True, True)])
def test_linear_sm_bias_and_gated_residual(Bsz, L, K, N_, bias, res):
    """The few-token kernel's epilogue on fp16 (bias in fp32 before the single rounding; out = residual + gate[b] * f16(x W^T + bias)): torch.equal
    with the 8-wave tiled kernel's (same arithmetic and rounding points) and against float64."""
    from zigma_amd import _lib
    from zigma_amd.linear import linear, linear_sm_eligible
    g = torch.Generator(device="cpu").manual_seed(Bsz + K + N_ + 3)
    x = torch.randn(Bsz, L, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H)
    b = (torch.randn(N_, generator=g) * 0.2).to(DEV, H) if bias else None
    r = torch.randn(Bsz, L, N_, generator=g).to(DEV, H) if res else None
    gt = torch.randn(Bsz, N_, generator=g).to(DEV, H) if res else None
    assert linear_sm_eligible(x, w, b)
    y = linear(x, w, b, residual=r, gate=gt, few_tokens=True)
    assert _lib.last_kernel().startswith("linear_sm_128x")
    y8 = linear(x, w, b, residual=r, gate=gt, _probe_flags=0x2000)
    assert _lib.last_kernel().startswith("linear_tn_")
    assert torch.equal(y, y8)
    v = x.double() @ w.double().T + (b.double() if bias else 0)
    ref = (r.double() + gt.double().unsqueeze(1) * v.half().double()) if res else v
    e = nerr(y.double(), ref)
    print(f"linear_sm epilogue f16 {Bsz}x{L}x{K}x{N_}: {e:.3e}")
    assert e < 3.75e-4
    assert torch.equal(linear(x, w, b, residual=r, gate=gt, few_tokens=True), y)


@pytest.mark.parametrize("Bsz,L,K,N_,bias,res", [(64, 1024, 1280, 640, False, False), (64, 1024, 1280, 640, False, True), (64, 1024, 512, 640, True, True),
                                                  (32, 2048, 192, 384, False, True), (128, 256, 256, 1152, True, True)])
def test_linear4w_narrow_tiles_and_gated_residual(Bsz, L, K, N_, bias, res, monkeypatch):
    """The f16 4-wave loop on n % 256 == 128 and with the gated branch add in its epilogue (+ bias as a rank-1 MFMA against 1.0 = 0x3c00):
    out = residual + gate[b] * (x W^T + bias) against float64 on sampled rows; against the 8-wave kernel, which rounds x W^T + b to fp16 before
    the gate (as in bf16 the two gated forms differ by that rounding only — bound 4e-3 / 8 — and the plain form is torch.equal); run-to-run identity."""
    from zigma_amd import _lib
    import zigma_amd.routing as zr
    from zigma_amd.linear import linear
    monkeypatch.setattr(zr, "POLICY", "all")
    g = torch.Generator(device="cpu").manual_seed(Bsz + K + N_)
    M = Bsz * L
    x = torch.randn(Bsz, L, K, generator=g).to(DEV, H)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H)
    b = (torch.randn(N_, generator=g) * 0.5).to(DEV, H) if bias else None
    r = torch.randn(Bsz, L, N_, generator=g).to(DEV, H) if res else None
    gt = torch.randn(Bsz, N_, generator=g).to(DEV, H) if res else None
    y = linear(x, w, b, residual=r, gate=gt)
    assert _lib.last_kernel() == ("linear4w_256x256+128" if N_ % 256 else "linear4w_256x256"), _lib.last_kernel()
    rows = torch.randint(0, M, (768,), generator=g).to(DEV)
    rows[:6] = torch.tensor([0, 127, 128, L - 1, L % M, M - 1], device=DEV)
    val = x.view(M, K)[rows].double() @ w.double().T + (b.double() if bias else 0)
    ref = val if not res else r.view(M, N_)[rows].double() + gt[rows // L].double() * val
    got = y.view(M, N_)[rows].double()
    e = nerr(got, ref)
    print(f"linear4w epilogue f16 {Bsz}x{L}x{K}x{N_}: {e:.3e}")
    assert e < 3.75e-4
    assert torch.allclose(got, ref, rtol=2e-3, atol=2.5e-3)
    y8 = linear(x, w, b, residual=r, gate=gt, _probe_flags=0x2000)
    assert _lib.last_kernel().startswith("linear_tn_")
    assert nerr(y.float(), y8.float()) < 4e-3 / 8
    if not res:
        assert torch.equal(y, y8)
    for _ in range(3):
        assert torch.equal(linear(x, w, b, residual=r, gate=gt), y)


@pytest.mark.parametrize("Bsz,L,K,Nn,bias", [(2, 256, 512, 640, True), (3, 512, 128, 128, False), (16, 1024, 512, 640, True)])
def test_linear_gated_residual_epilogue(Bsz, L, K, Nn, bias, monkeypatch):
    """out = residual + gate[b] * f16(x @ W^T + bias) in the 8-wave kernel's epilogue vs the same spelled out in float64 with the projection rounded
    to fp16 first; and against the fp32 fma of the kernel's own fp16 projection: mul + add instead of the fma moves a result across an fp16 rounding
    boundary with probability ~ ulp32(product) / ulp16(sum) = 2^-13 per element (2^-16 for bf16, whose test allows 1e-3): 8e-3."""
    import zigma_amd.routing as zr
    from zigma_amd import _lib
    from zigma_amd.linear import gated_residual_eligible, linear
    monkeypatch.setattr(zr, "POLICY", "all")
    g = torch.Generator(device="cpu").manual_seed(L + Nn)
    x = torch.randn(Bsz, L, K, generator=g).to(DEV, H)
    w = (torch.randn(Nn, K, generator=g) * K ** -0.5).to(DEV, H)
    b = (torch.randn(Nn, generator=g) * 0.5).to(DEV, H) if bias else None
    wide = torch.randn(Bsz, L, Nn + 64, generator=g).to(DEV, H)
    res = wide[:, :, 64:]
    gate = torch.randn(Bsz, 3 * Nn, generator=g).to(DEV, H)[:, Nn:2 * Nn]
    assert gated_residual_eligible(x, res, gate)
    out = linear(x, w, b, residual=res, gate=gate)
    assert _lib.last_kernel() == "linear_tn_256x128" and out.shape == (Bsz, L, Nn)
    proj = (x.double() @ w.double().T + (b.double() if bias else 0)).to(H).double()
    ref = res.double() + gate.double().unsqueeze(1) * proj
    e = nerr(out.double(), ref)
    print(f"gated residual epilogue f16 {Bsz}x{L}x{K}x{Nn}: {e:.3e}")
    assert e < 3.75e-4 and torch.allclose(out.double(), ref, rtol=2e-3, atol=2e-3)
    plain = linear(x, w, b)
    exact = torch.addcmul(res.float(), gate.float().unsqueeze(1), plain.float()).to(H)
    assert (out != exact).float().mean().item() < 8e-3


@pytest.mark.parametrize("M,K,Nn", [(1, 256, 72), (300, 1280, 72), (4096, 1536, 80), (257, 512, 96), (64, 256, 40), (16384, 1280, 72), (8192, 1536, 80),
                                    (8192, 1280, 72), (1000, 1024, 96), (16352, 1536, 33), (32768, 1536, 80), (512, 2048, 72)])
def test_x_proj_kernel_vs_oracle(M, K, Nn):
    """x_dbl = u @ W_x^T (streaming kernel / split-K form) on fp16 vs float64 numpy on the same operands, output rounded to fp16; run-to-run identity."""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import x_proj, x_proj_eligible
    rng = np.random.default_rng(M + K)
    u = r16(rng.standard_normal((M, K)))
    w = r16(rng.standard_normal((Nn, K)) * K ** -0.5)
    ut, wt = T(u, H), T(w, H)
    assert x_proj_eligible(ut, wt) == (M >= 16384 or (M >= 256 and K <= 1536))
    out = x_proj(ut, wt)
    assert _lib.last_kernel() == ("x_proj_splitk" if M < 16384 and K <= 1536 else "x_proj_mfma") and out.shape == (M, Nn) and out.dtype == H
    assert torch.equal(x_proj(ut, wt), out)
    ref = r16(u.astype(np.float64) @ w.astype(np.float64).T)
    e = rel_err(N(out), ref)
    print(f"x_proj f16 {M}x{K}x{Nn}: {e:.3e}")
    assert e < 3.75e-4 and np.allclose(N(out), ref, rtol=2.5e-3, atol=2.5e-3)


@pytest.mark.parametrize("Bsz,L,Di,Nn,order,flags", [(2, 128, 64, 72, "id", 0), (1, 256, 192, 40, "rand", 0), (1, 256, 192, 40, "rand", 3),
                                                   (16, 1024, 1280, 72, "rand", 0), (64, 256, 128, 96, "none", 1),
                                                   (4, 4096, 640, 72, "rev", 2), (8, 32, 64, 72, "rand", 0)])
def test_conv_x_proj_kernel_vs_oracle(Bsz, L, Di, Nn, order, flags):
    """The one-pass conv + SiLU + x_proj kernel on fp16 vs float64 numpy on the same operands: u (fp16-rounded conv output in scan order) and
    x_dbl = u @ W_x^T on the kernel's OWN u; and against the separate conv kernel's f16 instantiation."""
    from zigma_amd import _lib
    from zigma_amd.causal_conv1d_interface import causal_conv1d_raw
    from zigma_amd.selective_scan_interface import conv_x_proj, conv_x_proj_eligible
    rng = np.random.default_rng(L + Di)
    xz = r16(rng.standard_normal((Bsz, L, 2 * Di)))
    cw = r16(rng.standard_normal((Di, 4)) * 0.5)
    cb = r16(rng.standard_normal(Di) * 0.5)
    w = r16(rng.standard_normal((Nn, Di)) * Di ** -0.5)
    perm = {"id": np.arange(L), "rand": rng.permutation(L), "rev": np.arange(L)[::-1].copy(), "none": None}[order]
    xzt = T(xz, H)
    x_half = xzt[:, :, :Di]
    pt = None if perm is None else torch.tensor(perm, device="cuda", dtype=torch.int32)
    cwt, cbt, wt = T(cw, H), T(cb, H), T(w, H)
    assert conv_x_proj_eligible(x_half, cwt, cbt, wt, pt) == (Bsz * L >= 16384)
    u, x_dbl = conv_x_proj(x_half, cwt, cbt, wt, pt, _flags=flags)
    assert _lib.last_kernel() == "conv_x_proj_mfma" and u.shape == (Bsz, L, Di) and x_dbl.shape == (Bsz, L, Nn) and u.dtype == H
    xg = xz[:, :, :Di].astype(np.float64)
    if perm is not None:
        xg = xg[:, perm]
    xp = np.concatenate([np.zeros((Bsz, 3, Di)), xg], axis=1)
    pre = cb.astype(np.float64) + sum(cw[:, t].astype(np.float64) * xp[:, t:t + L] for t in range(4))
    u_ref = r16(pre / (1.0 + np.exp(-pre)))
    e_u = rel_err(N(u), u_ref)
    xd_ref = r16(N(u).astype(np.float64) @ w.astype(np.float64).T)
    e_x = rel_err(N(x_dbl), xd_ref)
    print(f"conv_x_proj f16 {Bsz}x{L}x{Di}x{Nn} flags {flags}: u {e_u:.3e}, x_dbl {e_x:.3e}")
    assert e_u < 3.75e-4 and np.allclose(N(u), u_ref, rtol=2.5e-3, atol=2.5e-3)
    assert e_x < 3.75e-4 and np.allclose(N(x_dbl), xd_ref, rtol=2.5e-3, atol=2.5e-3)
    u_sep = torch.empty_like(u)
    causal_conv1d_raw(x_half.transpose(1, 2), cwt, cbt, True, out=u_sep.transpose(1, 2), x_row_index=pt)
    assert (u_sep != u).float().mean().item() < 0.02
    assert torch.allclose(u_sep.float(), u.float(), rtol=1e-2 / 8, atol=1e-3 / 8)


@pytest.mark.parametrize("M,Di,R,S", [(1, 64, 40, 72), (100, 128, 40, 72), (4096, 1280, 40, 72), (333, 192, 8, 40), (64, 64, 48, 48)])
def test_dt_proj_softplus_mfma_vs_oracle(M, Di, R, S):
    """out = softplus(x[:, :R] @ W.T + b) on fp16: fp32 oracle on the same operands, result rounded to fp16 (bounds of the bf16 original / 8)."""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import dt_proj_eligible, dt_proj_softplus
    rng = np.random.default_rng(M + R)
    x = r16(rng.standard_normal((2, M, S)))
    w = r16(rng.standard_normal((Di, R)) * 0.3)
    b = (rng.standard_normal(Di) * 2).astype(np.float32)
    b[0] = 25.0
    wt = torch.zeros(Di, 48, device=DEV, dtype=H)[:, :R]
    wt.copy_(T(w, H))
    xt = T(x, H)
    assert dt_proj_eligible(xt, R, wt)
    out = dt_proj_softplus(xt, R, wt, T(b), True)
    assert _lib.last_kernel() == "dt_proj_softplus_mfma" and out.shape == (2, M, Di) and out.dtype == H
    ref = r16(zo.softplus(x[:, :, :R] @ w.T + b))
    e = rel_err(N(out), ref)
    lin = dt_proj_softplus(xt, R, wt, None, False)
    e_lin = rel_err(N(lin), r16(x[:, :, :R] @ w.T))
    print(f"dt_proj f16 {M}x{Di}x{R}: softplus {e:.3e}, linear {e_lin:.3e}")
    assert np.allclose(N(out), ref, rtol=1e-2 / 8, atol=1e-2 / 8) and e < 1e-3 / 8
    assert e_lin < 1e-3 / 8


@pytest.mark.parametrize("Bsz,L,Hh,NC", [(2, 100, 8, 77), (1, 64, 3, 128), (3, 17, 8, 5), (2, 256, 8, 81)])
def test_cross_attn_kernel_vs_oracle(Bsz, L, Hh, NC):
    """softmax(scale Q K^T) V per head on fp16 (both MFMAs in their f16 form, P rounded to fp16) vs float64 numpy on the same operands;
    K / V are row-strided slices of one buffer."""
    from zigma_amd import _lib
    from zigma_amd.attention import cross_attn, cross_attn_eligible
    rng = np.random.default_rng(L + NC)
    C = Hh * 64
    q = r16(rng.standard_normal((Bsz, L, C)))
    kv = r16(rng.standard_normal((Bsz, NC, 2, C)))
    kvt = T(kv, H)
    k, v = kvt[:, :, 0], kvt[:, :, 1]
    assert cross_attn_eligible(T(q, H), k, v, Hh)
    out = cross_attn(T(q, H), k, v, Hh)
    assert _lib.last_kernel() == "cross_attn_mfma" and out.shape == (Bsz, L, C) and out.dtype == H
    assert torch.equal(cross_attn(T(q, H), k, v, Hh), out)
    qh = q.reshape(Bsz, L, Hh, 64).transpose(0, 2, 1, 3).astype(np.float64)
    kh = kv[:, :, 0].reshape(Bsz, NC, Hh, 64).transpose(0, 2, 1, 3).astype(np.float64)
    vh = kv[:, :, 1].reshape(Bsz, NC, Hh, 64).transpose(0, 2, 1, 3).astype(np.float64)
    sc = qh @ kh.transpose(0, 1, 3, 2) * 64 ** -0.5
    pr = np.exp(sc - sc.max(-1, keepdims=True))
    ref = ((pr / pr.sum(-1, keepdims=True)) @ vh).transpose(0, 2, 1, 3).reshape(Bsz, L, C)
    e = rel_err(N(out), ref)
    print(f"cross_attn f16 {Bsz}x{L}x{Hh}x{NC}: {e:.3e}")
    assert e < 7.5e-4
    assert np.allclose(N(out), ref, rtol=3.75e-3, atol=3.75e-3)


# ---------------------------------------------------------------------------------------------------
# 3. every routing cell
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [512, 640, 768, 1024])
@pytest.mark.parametrize("Bsz", [4, 8, 16, 64])
def test_every_routing_cell_vs_float64(E, Bsz):
    """zigma_amd/routing.py is dtype-blind: every cell of the table through linear.project on fp16 operands — the kernel that served the call is the one
    the table names, the fused flag is the row's, no tensor-level refusal, each result against float64 (4e-3 / 8)."""
    import zigma_amd.routing as zr
    from zigma_amd import _lib
    from zigma_amd.linear import project
    L = 1024
    tokens = Bsz * L
    g = torch.Generator(device="cpu").manual_seed(E + Bsz)
    zr.REFUSED.clear()
    for role, (n, k) in {"in_proj": (4 * E, E), "out_proj": (E, 2 * E), "to_q": (512, E), "to_out": (E, 512)}.items():
        x = torch.randn(Bsz, L, k, generator=g).to(DEV, H)
        w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, H)
        b = (torch.randn(n, generator=g) * 0.3).to(DEV, H) if role == "to_out" else None
        res = torch.randn(Bsz, L, n, generator=g).to(DEV, H) if role in ("out_proj", "to_out") else None
        gate = torch.randn(Bsz, n, generator=g).to(DEV, H) if res is not None else None
        r = zr.route(role, tokens, n, k)
        trace = []
        _lib.TRACE = trace
        try:
            with torch.no_grad():
                y = project(role, x, w, b, residual=res, gate=gate)
        finally:
            _lib.TRACE = None
        served = [kern for fn, kern, _ in trace if fn == "zigma_linear_fwd"]
        if r.kernel == "library":
            assert served == [], (role, E, tokens, r, served)
        else:
            want = zr.kernel_name(r, tokens, n, k)
            assert len(served) == (2 if r.kernel == "tiled_halves" else 1) and all(sv.startswith(want) for sv in served), (role, E, tokens, r, served)
            assert all(P.dtype == _lib.F16 for fn, _, P in trace if fn == "zigma_linear_fwd")
            fused = [bool(P.residual) for fn, _, P in trace if fn == "zigma_linear_fwd"]
            assert fused == [bool(res is not None and r.fuse_add)] * len(served), (role, E, tokens, r, fused)
        rows = torch.randint(0, tokens, (512,), generator=g).to(DEV)
        rows[:3] = torch.tensor([0, L - 1, tokens - 1], device=DEV)
        x2, y2 = x.view(tokens, k), y.view(tokens, n)
        ref = x2[rows].double() @ w.double().T + (b.double() if b is not None else 0)
        if res is not None:
            ref = res.view(tokens, n)[rows].double() + gate.double()[rows // L] * ref
        err = nerr(y2[rows].double(), ref)
        print(f"routing cell f16 {role} E={E} tokens={tokens} -> {r.row}: {err:.3e}")
        assert err < 5e-4, (role, E, tokens, r, err)
    assert zr.REFUSED == [], zr.REFUSED


# ---------------------------------------------------------------------------------------------------
# 4. Mamba inner at B = 16
# ---------------------------------------------------------------------------------------------------
def _inner_weights(Di, R, Nst, seed):
    rng = np.random.default_rng(seed)
    n = lambda *s, sc=1.0: r16(rng.standard_normal(s) * sc)
    w = dict(conv_w=n(Di, 4, sc=0.4), conv_b=n(Di, sc=0.1), x_proj_w=n(R + 2 * Nst, Di, sc=Di ** -0.5), dt_proj_w=n(Di, R, sc=R ** -0.5))
    w["A"] = -np.exp(np.log(np.arange(1, Nst + 1, dtype=np.float32))[None].repeat(Di, 0) + 0.2 * rng.standard_normal((Di, Nst))).astype(np.float32)
    w["D"] = (1 + 0.2 * rng.standard_normal(Di)).astype(np.float32)
    dt = np.exp(rng.random(Di) * (np.log(0.1) - np.log(1e-3)) + np.log(1e-3))
    w["dt_bias"] = (dt + np.log(-np.expm1(-dt))).astype(np.float32)
    return w


def test_mamba_inner_b16_fp16():
    """mamba_inner_tok at B = 16, L = 1024, Di = 1280, N = 16, R = 40, the column-zigzag table and its inverse, fp16: four sampled (sample, slab) pairs
    against the staged oracle of test_config2_mamba_inner_full_size_bf16 with fp16 rounding where that one rounds to bf16 (u, x_dbl, the output; the
    step size stays in fp32: dt_proj inside the scan).  Bound 3e-4: the scan's existing fp16 bound (tests/test_gpu_parity.py), above 1e-3 / 8.
    The front is the one-pass conv + x_proj kernel, the scan the whole-sequence kernel with its in-kernel dt_proj — both from the call trace."""
    from zigma_amd import _lib
    from zigma_amd.scan_paths import zigzag_path
    from zigma_amd.selective_scan_interface import mamba_inner_tok
    Bsz, L, Di, R, Nst = 16, 1024, 1280, 40, 16
    w = _inner_weights(Di, R, Nst, seed=2)
    g = torch.Generator().manual_seed(7)
    xz = torch.randn(Bsz, L, 2 * Di, generator=g).half()
    perm = np.asarray(zigzag_path(32)[1]).astype(np.int64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt)
    cw, cb, xw, dw = t(w["conv_w"][:, None, :], H), t(w["conv_b"], H), t(w["x_proj_w"], H), t(w["dt_proj_w"], H)
    A, D, db = t(w["A"], torch.float32), t(w["D"], torch.float32), t(w["dt_bias"], torch.float32)
    p32 = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    trace = []
    _lib.TRACE = trace
    try:
        with torch.no_grad():
            y = mamba_inner_tok(xz.to(DEV), cw, cb, xw, dw, A, D, db, perm=p32, out_rows=p32)
    finally:
        _lib.TRACE = None
    served = [(fn, kern) for fn, kern, _ in trace]
    assert ("zigma_conv_x_proj_fwd", "conv_x_proj_mfma") in served and ("zigma_selective_scan_fwd", "scan_tok2_n16_dtproj") in served, served
    assert y.dtype == H
    worst = 0.0
    for b, slab in ((0, 0), (5, 7), (10, 13), (15, 19)):
        xz_b = xz[b].float().numpy()
        xs = xz_b[perm, :Di]
        u = r16(zo.causal_conv1d(xs.T[None], w["conv_w"], w["conv_b"], "silu")[0].T)
        x_dbl = r16(u.astype(np.float64) @ w["x_proj_w"].astype(np.float64).T)
        delta = zo.softplus((x_dbl[:, :R].astype(np.float64) @ w["dt_proj_w"].astype(np.float64).T).astype(np.float32) + w["dt_bias"])
        sl = slice(slab * 64, slab * 64 + 64)
        z = xz_b[perm][:, Di + sl.start:Di + sl.stop]
        ys = zo.selective_scan(u[:, sl].T[None], delta[:, sl].T[None], w["A"][sl], x_dbl[:, R:R + Nst].T[None],
                               x_dbl[:, R + Nst:R + 2 * Nst].T[None], w["D"][sl], z.T[None], None, False)[0].T
        ref = np.empty_like(ys)
        ref[perm] = ys
        worst = max(worst, rel_err(N(y[b, :, sl]), r16(ref)))
    print(f"fp16 mamba inner B=16 vs oracle, worst of 4 (sample, slab) pairs: {worst:.3e}")
    assert worst < 3e-4, worst


# ---------------------------------------------------------------------------------------------------
# 5. the block path of the README model
# ---------------------------------------------------------------------------------------------------
def _r2_model(name, dtype):
    from zigma_amd.model_zigma import ZigMa
    g = load_golden(name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = ZigMa(device="cpu", dtype=dtype, **cfg)
    fill_state(m, int(g["seed"]))
    return m.to(DEV).eval(), g, cfg


@pytest.mark.parametrize("Bsz", [16, 32])
def test_block_path_fp16_vs_reference(Bsz, monkeypatch):
    """README model (r2_readme_b2 weights) in fp16, B = 16 / 32, the two reference samples at batch positions 0 and B - 1 inside noise (built as
    test_bench_block_path_vs_reference builds them).  From the call trace: the counts that test asserts for its `default` / `default_b32` variants
    (conv_x_proj, scan_tok2 with the in-kernel dt_proj, cross_attn_mfma = depth each; 4 * depth + 2 projection calls; the gated counts), all of them
    on fp16 operands, and (a spy on F.linear) no library product of >= 2048 rows in the block loop: the only such calls are the two operators around
    the blocks that stay bf16-only by design and run as torch ops in an fp16 model — the patch embed (k = in_channels * p^2) and the final layer's
    projection (n = p^2 * out_channels), both of zigma_amd/embed.py.  Accuracy: the same inputs once more with every fp16 gate of the matrix-core kernels
    closed (routing.POLICY = "off", the five predicates False: the library-served fp16 forward of before); with e_own / e_lib the distances of the
    two runs to the reference's fp32 output, e_own < 1.1 * e_lib — the project's margin for "as close to the fp32 result as another 16-bit run"."""
    import torch.nn.functional as F
    import zigma_amd.linear as zl
    import zigma_amd.model_zigma as mz
    import zigma_amd.routing as zr
    import zigma_amd.selective_scan_interface as ssi
    from zigma_amd import _lib
    m, g, cfg = _r2_model("r2_readme_b2", H)
    depth, E = cfg["depth"], cfg["embed_dim"]
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(Bsz, *g["x"].shape[1:], generator=gen)
    t = torch.rand(Bsz, generator=gen)
    y = torch.rand(Bsz, *g["y"].shape[1:], generator=gen)
    for pos, src in ((0, 0), (Bsz - 1, 1)):
        x[pos], t[pos], y[pos] = torch.from_numpy(g["x"][src]), float(g["t"][src]), torch.from_numpy(g["y"][src])
    xd, td, yd = x.to(DEV).half(), t.to(DEV).half(), y.to(DEV).half()
    lib_rows = []
    real_linear = F.linear
    monkeypatch.setattr(F, "linear", lambda inp, wt, bias=None: (lib_rows.append((inp.numel() // inp.shape[-1], wt.shape[0], wt.shape[1])),
                                                                 real_linear(inp, wt, bias))[1])
    trace = []
    monkeypatch.setattr(_lib, "TRACE", trace)
    with torch.no_grad():
        out = m(xd, td, yd)
    monkeypatch.setattr(_lib, "TRACE", None)
    own_lib_rows = list(lib_rows)
    counts, gated = {}, 0
    for fn, kern, P in trace:
        counts[(fn, kern)] = counts.get((fn, kern), 0) + 1
        gated += fn == "zigma_linear_fwd" and bool(P.residual)
    lin = [(kern, P) for fn, kern, P in trace if fn == "zigma_linear_fwd"]
    assert counts.get(("zigma_conv_x_proj_fwd", "conv_x_proj_mfma"), 0) == depth, counts
    assert counts.get(("zigma_selective_scan_fwd", "scan_tok2_n16_dtproj"), 0) == depth, counts
    assert counts.get(("zigma_dt_proj_softplus_fwd", "dt_proj_softplus_mfma"), 0) == 0, counts
    assert counts.get(("zigma_cross_attn_fwd", "cross_attn_mfma"), 0) == depth, counts
    assert len(lin) == 4 * depth + 2, (len(lin), counts)
    assert all(P.dtype == _lib.F16 for fn, _, P in trace if fn in ("zigma_linear_fwd", "zigma_conv_x_proj_fwd", "zigma_cross_attn_fwd"))
    assert sum(1 for _, P in lin if P.m % 256 == 0 and P.m < Bsz * 1024) == 2, counts           # y_embedder, batched K / V
    assert counts.get(("zigma_linear_fwd", "linear_ws"), 0) == depth, counts                     # in_proj, weight-stationary
    assert sum(1 for _, P in lin if P.k == E and P.n == 2 * E and P.m == Bsz * 1024) == 0
    if Bsz == 16:       # out_proj (unfused) on the 128-feature-panel form, its add in the next norm kernel; to_out + bias + add fused
        assert gated == depth and counts.get(("zigma_linear_fwd", "linear_ws_128"), 0) == depth, (gated, counts)
    else:               # out_proj and to_out both carry their gated adds
        assert gated == 2 * depth, (gated, counts)
    assert not any(k.startswith("Cijk") for (_, k), _ in counts.items())
    w_pe, w_fl = m.x_embedder.proj.weight, m.final_layer.linear.weight
    around = {(Bsz * 1024, w_pe.shape[0], w_pe[0].numel()), (Bsz * 1024, w_fl.shape[0], w_fl.shape[1])}      # patch embed, final layer
    big = [c for c in own_lib_rows if c[0] >= 2048]
    assert set(big) <= around and len(big) <= 2, big
    # the library-served fp16 forward: every gate this change opens for fp16, closed
    monkeypatch.setattr(zr, "POLICY", "off")
    monkeypatch.setattr(zl, "linear_eligible", lambda *a, **k: False)
    for name in ("x_proj_eligible", "conv_x_proj_eligible", "dt_proj_eligible"):
        monkeypatch.setattr(ssi, name, lambda *a, **k: False)
    monkeypatch.setattr(mz, "cross_attn_eligible", lambda *a, **k: False)
    trace2 = []
    monkeypatch.setattr(_lib, "TRACE", trace2)
    with torch.no_grad():
        out_lib = m(xd, td, yd)
    monkeypatch.setattr(_lib, "TRACE", None)
    assert not [fn for fn, _, _ in trace2 if fn in ("zigma_linear_fwd", "zigma_conv_x_proj_fwd", "zigma_x_proj_fwd", "zigma_cross_attn_fwd",
                                                    "zigma_dt_proj_softplus_fwd")]
    got, got_lib = N(out)[[0, Bsz - 1]], N(out_lib)[[0, Bsz - 1]]
    e_own, e_lib = rel_err(got, g["out"]), rel_err(got_lib, g["out"])
    print(f"fp16 block path B={Bsz}: own kernels vs reference fp32 {e_own:.3e}, library-served {e_lib:.3e}; own vs library {rel_err(got, got_lib):.3e}; "
          f"linear calls {len(lin)}, gated {gated}")
    assert np.isfinite(N(out_lib)).all(), "the library-served fp16 forward is not finite on this fixture"
    assert np.isfinite(N(out)).all()
    assert e_own < 1.1 * e_lib, (e_own, e_lib)


# ---------------------------------------------------------------------------------------------------
# 6. the training products
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N_", [(16384, 1280, 640), (16384, 640, 2560)])
def test_linear_train_fn_fp16(M, K, N_, monkeypatch):
    """wgrad.LinearTrainFn on fp16: forward product and dX on zigma_linear_fwd (from the call trace), against the library path within 5e-4 and
    against float64; dW (slab-wise, library) does not depend on the policy."""
    import zigma_amd.routing as zr
    import zigma_amd.wgrad as wg
    from zigma_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(DEV, H).requires_grad_(True)
    w = (torch.randn(N_, K, generator=g) * K ** -0.5).to(DEV, H).requires_grad_(True)
    dy = torch.randn(M, N_, generator=g).to(DEV, H)
    monkeypatch.setattr(zr, "POLICY", "auto")
    trace = []
    monkeypatch.setattr(_lib, "TRACE", trace)
    y = wg.linear_train(x, w)
    y.backward(dy)
    monkeypatch.setattr(_lib, "TRACE", None)
    own = [(kern, P.dtype) for fn, kern, P in trace if fn == "zigma_linear_fwd"]
    assert len(own) == 2 and all(d == _lib.F16 for _, d in own), [t[:2] for t in trace]
    got = (y.detach(), x.grad.clone(), w.grad.clone())
    x.grad = w.grad = None
    monkeypatch.setattr(zr, "POLICY", "off")
    y2 = wg.linear_train(x, w)
    y2.backward(dy)
    rows = torch.randint(0, M, (512,), generator=g).to(DEV)
    xd, wd, dyd = x.detach().double(), w.detach().double(), dy.double()
    e_y, e_dx = nerr(got[0][rows].double(), xd[rows] @ wd.T), nerr(got[1][rows].double(), dyd[rows] @ wd)
    l_y, l_dx = nerr(got[0].float(), y2.detach().float()), nerr(got[1].float(), x.grad.float())
    print(f"linear_train f16 {M}x{K}x{N_} {own}: vs float64 y {e_y:.3e} dx {e_dx:.3e}; vs library y {l_y:.3e} dx {l_dx:.3e}")
    assert e_y < 3.1e-4 and e_dx < 3.1e-4
    assert l_y < 5e-4 and l_dx < 5e-4
    assert torch.equal(got[2], w.grad)


def test_model_gradients_fp16_close_to_fp32_reference():
    """The fp16 twin of tests/test_gpu_backward.py::test_model_gradients_bf16_close_to_fp32_reference (same fixture, same limits: fp16 carries
    three more mantissa bits than bf16): fp16 parameters / activations under autograd reach the three backward kernels in their F16 instantiations
    — asserted from the call trace — and the gradients stay within the bf16 limits of the reference's fp32 autograd gradients."""
    from zigma_amd import _lib
    from zigma_amd.model_zigma import ZigMa
    name = "zigma_uncond_zigzag8"
    g, gg = load_golden(name + ".npz"), load_golden("bwd_model_" + name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = ZigMa(device=DEV, dtype=H, **cfg).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    x = T(g["x"]).requires_grad_(True)
    _lib.TRACE = []
    try:
        out = m(x, T(g["t"]), None)
        (out * T(gg["wgt"])).sum().backward()
    finally:
        trace, _lib.TRACE = _lib.TRACE, None
    for fn, field in (("zigma_selective_scan_bwd", "io_dtype"), ("zigma_causal_conv1d_bwd", "io_dtype"), ("zigma_add_norm_bwd", "x_dtype")):
        seen = [getattr(P, field) for f, _, P in trace if f == fn]
        assert seen and all(d == _lib.F16 for d in seen), (fn, seen)
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    e = rel_err(N(x.grad), gg["gx"])
    worst = 1.0
    for k, p in m.named_parameters():
        if "g." + k not in gg or p.grad is None:
            continue
        assert torch.isfinite(p.grad).all(), k
        a, b = N(p.grad).ravel().astype(np.float64), gg["g." + k].ravel().astype(np.float64)
        if np.linalg.norm(b) < 1e-6:
            continue
        worst = min(worst, float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30)))
    print(f"fp16 model gradients vs fp32 reference: input gradient {e:.3e}, worst cosine {worst:.4f}")
    assert e < 8e-2, e
    assert worst > 0.95, worst


# ---------------------------------------------------------------------------------------------------
# 7. refusals stay refusals
# ---------------------------------------------------------------------------------------------------
def test_mixed_dtypes_and_fp32_are_refused():
    """all operands of a call share ONE 16-bit dtype: fp16 x with bf16 w is not eligible anywhere and plans to the library; fp32 is
    ZIGMA_ERR_DTYPE on the C side of every matrix-core entry point and the library route on the host, as before."""
    import zigma_amd.routing as zr
    from zigma_amd.attention import cross_attn_bwd_eligible, cross_attn_eligible
    from zigma_amd.linear import gated_residual_eligible, linear, linear_eligible, plan
    from zigma_amd.selective_scan_interface import (conv_x_proj_eligible, dt_proj_eligible, dt_proj_softplus, x_proj, x_proj_eligible)
    bf = torch.bfloat16
    x = torch.randn(16, 1024, 640, device=DEV)
    w = torch.randn(2560, 640, device=DEV) * 640 ** -0.5
    assert linear_eligible(x.half(), w.half()) and linear_eligible(x.to(bf), w.to(bf))
    assert not linear_eligible(x.half(), w.to(bf)) and not linear_eligible(x.to(bf), w.half())
    assert not linear_eligible(x.half()[..., :512].contiguous(), w.half()[:640, :512].contiguous(), torch.zeros(640, device=DEV, dtype=bf))
    assert plan("in_proj", x.half(), w.to(bf)) == zr.Route("library", False, "not-16bit-inference")
    assert plan("in_proj", x, w).kernel == "library" and not linear_eligible(x, w)
    assert plan("in_proj", x.half(), w.half()).kernel != "library"
    with pytest.raises(RuntimeError, match=rf"status {ERR_DTYPE}\)"):
        linear(x, w)
    res, gate = torch.randn(16, 1024, 2560, device=DEV), torch.randn(16, 2560, device=DEV)
    assert gated_residual_eligible(x.half(), res.half(), gate.half())
    assert not gated_residual_eligible(x.half(), res.to(bf), gate.half()) and not gated_residual_eligible(x.half(), res.half(), gate.to(bf))
    assert not gated_residual_eligible(x, res, gate)
    u, xw = torch.randn(16384, 1280, device=DEV), torch.randn(72, 1280, device=DEV)
    assert x_proj_eligible(u.half(), xw.half()) and not x_proj_eligible(u.half(), xw.to(bf)) and not x_proj_eligible(u, xw)
    with pytest.raises(RuntimeError, match=rf"status {ERR_DTYPE}\)"):
        x_proj(u, xw)
    xz, cw, cb = torch.randn(16, 1024, 2560, device=DEV), torch.randn(1280, 4, device=DEV), torch.randn(1280, device=DEV)
    assert conv_x_proj_eligible(xz.half()[:, :, :1280], cw.half(), cb.half(), xw.half(), None)
    assert not conv_x_proj_eligible(xz.half()[:, :, :1280], cw.to(bf), cb.half(), xw.half(), None)
    assert not conv_x_proj_eligible(xz.half()[:, :, :1280], cw.half(), cb.half(), xw.to(bf), None)
    assert not conv_x_proj_eligible(xz[:, :, :1280], cw, cb, xw, None)
    xd, dw = torch.randn(4096, 72, device=DEV), torch.randn(1280, 40, device=DEV)
    dwp = lambda dt: torch.zeros(1280, 48, device=DEV, dtype=dt)[:, :40].copy_(dw)
    assert dt_proj_eligible(xd.half(), 40, dwp(H)) and not dt_proj_eligible(xd.half(), 40, dwp(bf)) and not dt_proj_eligible(xd, 40, dwp(torch.float32))
    with pytest.raises(RuntimeError, match=rf"status {ERR_DTYPE}\)"):
        dt_proj_softplus(xd, 40, dwp(torch.float32))
    q, kv = torch.randn(2, 256, 512, device=DEV), torch.randn(2, 77, 512, device=DEV)
    assert cross_attn_eligible(q.half(), kv.half(), kv.half(), 8) and not cross_attn_eligible(q.half(), kv.to(bf), kv.half(), 8)
    assert not cross_attn_eligible(q, kv, kv, 8)
    assert cross_attn_bwd_eligible(q.to(bf), kv.to(bf), kv.to(bf), 8) and not cross_attn_bwd_eligible(q.half(), kv.half(), kv.half(), 8)
