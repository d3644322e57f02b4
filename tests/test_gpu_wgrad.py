"""GPU tests of zigma_linear_wgrad (csrc/wgrad.hip): dW = dY^T X on the own split-K MFMA kernel, through zigma_amd.wgrad.

Reference everywhere: float64 `dy.double().T @ x.double()` on the same 16-bit operands, compared with conftest.rel_err.  Bounds: 16-bit outputs the
project's projection bounds (2.5e-3 bf16, 3.1e-4 fp16 — the float64 result rounded to the type is 1.6-1.7e-3 / 2.0-2.1e-4 away at these
shapes), fp32 outputs 2e-5 (the fp32 kernel bound; fp32 accumulation in 64-token steps measures 5.8e-7 at 65 536 tokens, one dropped token row of
65 536 is 3.9e-3).

Measured worst errors on the MI355X (one full-suite run, all 61 cases green; every case prints its figure): the seeded sweep 1.71e-3 bf16 / 2.18e-4
fp16 with 16-bit outputs and 4.0e-7 / 4.4e-7 with fp32 outputs; views 1.68e-3 / 2.05e-4 and 2.2e-7 / 2.4e-7; the six production shapes at 65 536
tokens 1.66e-3 / 2.09e-4 against float64 and 6.5e-5 / 1.8e-5 against the slab-bmm path; through autograd linear_train 1.66e-3 / 2.08e-4 and the
Mamba inner's two products 1.68e-3 / 2.13e-4, the same with the own kernel and with the library path.  The row-by-row and element-by-element sweep of the
same entry point, with NaN surroundings and known answers, is tests/test_gpu_matmul_sweep.py.
"""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
BOUND16 = {torch.bfloat16: 2.5e-3, torch.float16: 3.1e-4}
BOUND32 = 2e-5


def N(t):
    return t.detach().double().cpu().numpy()


def ref64(dy, x):
    return dy.double().T @ x.double()


def bound(dtype, out_dtype):
    return BOUND32 if out_dtype == torch.float32 else BOUND16[dtype]


# ---- 1. layout, exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("m,n,k", [(16, 32, 32), (64, 32, 32), (64, 72, 40), (200, 136, 264)])
def test_wgrad_layout_exact_integers(m, n, k, slabs, dtype):
    """asymmetric small-integer operands (exact in both 16-bit types, all sums small integers): the fp32 result equals the int64 product exactly —
    catches a swapped row / column map and A and B disagreeing on the token permutation of the transposed reads"""
    from zigma_amd import _lib, wgrad as wg
    mi = torch.arange(m).view(m, 1)
    dyi = (3 * mi + 5 * torch.arange(n).view(1, n)) % 7 - 3
    xi = (mi + 2 * torch.arange(k).view(1, k)) % 5 - 2
    want = dyi.T @ xi                                                   # int64
    got = wg.wgrad_own(dyi.to(DEV, dtype), xi.to(DEV, dtype), out_dtype=torch.float32, slabs=slabs)
    assert _lib.last_kernel().startswith("wgrad_")
    assert got.dtype == torch.float32 and got.shape == (n, k)
    assert torch.equal(got.cpu().to(torch.int64), want) and torch.equal(got.cpu(), want.float())


# ---- 2. seeded sweep vs float64 ---------------------------------------------------------------------------------------------------------
SWEEP_M = (1, 8, 24, 64, 72, 264, 1000, 4104)
SWEEP_SLABS = (0, 1, 2, 3, 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,k", [(32, 32), (72, 128), (128, 40), (136, 264), (512, 640)])
def test_wgrad_sweep_vs_float64(n, k, dtype):
    """unit-normal operands, every m x slabs (a forced S above the number of 64-token steps included) x output type; S = 0 twice, bit-equal"""
    from zigma_amd import wgrad as wg
    g = torch.Generator(device="cpu").manual_seed(1000 * n + k)
    m_max = max(SWEEP_M)
    dy_all = torch.randn(m_max, n, generator=g).to(DEV, dtype)
    x_all = torch.randn(m_max, k, generator=g).to(DEV, dtype)
    worst = {}
    for m in SWEEP_M:
        dy, x = dy_all[:m], x_all[:m]
        want = N(ref64(dy, x))
        for out_dtype in (dtype, torch.float32):
            for slabs in SWEEP_SLABS:
                got = wg.wgrad_own(dy, x, out_dtype=out_dtype, slabs=slabs)
                assert got.dtype == out_dtype and got.shape == (n, k)
                err = rel_err(N(got), want)
                key = "f32" if out_dtype == torch.float32 else "io"
                worst[key] = max(worst.get(key, 0.0), err)
                print(f"wgrad sweep {dtype} n={n} k={k} m={m} out={out_dtype} slabs={slabs}: {err:.3e}")
                assert err < bound(dtype, out_dtype), (m, n, k, slabs, out_dtype, err)
                if slabs == 0:
                    assert torch.equal(got, wg.wgrad_own(dy, x, out_dtype=out_dtype, slabs=0))
    print(f"wgrad sweep worst {dtype} n={n} k={k}: {worst}")


# ---- 3. views and bounds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("m,slabs", [(264, 0), (264, 3), (4104, 0), (4104, 3)])
def test_wgrad_views_and_bounds(m, slabs, out_f32, dtype):
    """column views of wider rows whose other columns are NaN, `out` a view inside a sentinel-filled buffer, the workspace NaN before the call:
    finite result within the bounds, every sentinel untouched (nothing outside out[:n, :k] is written, every partial that is read was written)"""
    from zigma_amd import wgrad as wg
    n, k = 72, 40
    g = torch.Generator(device="cpu").manual_seed(m + slabs)
    x_wide = torch.full((m, 72), float("nan"), dtype=dtype)
    x_wide[:, :k] = torch.randn(m, k, generator=g).to(dtype)
    dy_wide = torch.full((m, 96), float("nan"), dtype=dtype)
    dy_wide[:, 8:80] = torch.randn(m, n, generator=g).to(dtype)
    x, dy = x_wide.to(DEV)[:, :k], dy_wide.to(DEV)[:, 8:80]
    out_dtype = torch.float32 if out_f32 else dtype
    sentinel = 12345.0
    big = torch.full((n + 12, k + 24), sentinel, device=DEV, dtype=out_dtype)
    out = big[4:4 + n, 8:8 + k]
    nbytes = wg.wgrad_workspace_bytes(m, n, k, dtype, slabs)
    assert (nbytes > 0) == (slabs == 3 or m == 4104)                    # (the library's own choice is one slab below 1024 tokens)
    ws = torch.full((max(nbytes // 4, 4) + 64,), float("nan"), device=DEV, dtype=torch.float32)
    got = wg.wgrad_own(dy, x, out_dtype=out_dtype, slabs=slabs, out=out, workspace=ws[:max(nbytes // 4, 4)])
    assert got.data_ptr() == out.data_ptr()
    assert torch.isfinite(out).all()
    err = rel_err(N(out), N(ref64(dy, x)))
    print(f"wgrad views {dtype} m={m} slabs={slabs} out={out_dtype}: {err:.3e}")
    assert err < bound(dtype, out_dtype)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[4:4 + n, 8:8 + k] = False
    assert (big[mask] == sentinel).all()
    assert torch.isnan(ws[max(nbytes // 4, 4):]).all()                  # nothing past the workspace that was asked for


# ---- 4. production shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,n,k,pitch", [("in_proj", 2560, 640, 0), ("out_proj", 640, 1280, 0), ("to_q", 512, 640, 0), ("to_out", 640, 512, 0),
                                            ("x_proj", 72, 1280, 0), ("dt_proj", 1280, 40, 72)])
def test_wgrad_production_shapes(name, n, k, pitch, dtype, monkeypatch):
    """the six products of a block at 65 536 tokens, one launch each (dt_proj with x as the 72-pitch column view of x_dbl), against float64 and
    against the slab-bmm path"""
    from zigma_amd import _lib, wgrad as wg
    m = 65536
    g = torch.Generator(device=DEV).manual_seed(n + k)
    dy = torch.randn(m, n, device=DEV, generator=g).to(dtype)
    x = torch.randn(m, pitch or k, device=DEV, generator=g).to(dtype)[:, :k]
    got = wg.wgrad_own(dy, x)
    assert got.dtype == dtype and _lib.last_kernel().startswith("wgrad_")
    want = N(ref64(dy, x))
    err = rel_err(N(got), want)
    monkeypatch.setattr(wg, "OWN_WGRAD", False)
    trace = []
    monkeypatch.setattr(_lib, "TRACE", trace)
    lib_path = wg.wgrad(dy, x.contiguous())
    monkeypatch.setattr(_lib, "TRACE", None)
    assert not trace
    err_bmm = rel_err(N(got), N(lib_path))
    print(f"wgrad production {name} {dtype}: vs float64 {err:.3e}, vs slab-bmm {err_bmm:.3e}")
    assert err < BOUND16[dtype], err
    assert err_bmm < 2 * BOUND16[dtype], err_bmm


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def _raises_status(status, fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert f"(status {status})" in str(e.value), str(e.value)


def test_wgrad_refusals(monkeypatch):
    """every status of the entry point arrives as RuntimeError with its number, nothing is launched (the call trace stays empty, `out` keeps its
    sentinel), and plan_wgrad answers "bmm" for the same tensors"""
    from zigma_amd import _lib, wgrad as wg
    bf = torch.bfloat16
    trace = []
    monkeypatch.setattr(_lib, "TRACE", trace)
    monkeypatch.setattr(wg, "OWN_WGRAD", "all")                       # (the tensor-level layer alone must refuse)
    m = 512
    dy, x = torch.ones(m, 32, device=DEV, dtype=bf), torch.ones(m, 40, device=DEV, dtype=bf)
    out = torch.full((32, 40), 7.0, device=DEV, dtype=torch.float32)
    assert wg.plan_wgrad(dy, x) == "own"

    def block(**kw):
        P = _lib.LinearWgradParams()
        P.m, P.n, P.k, P.dtype, P.out_dtype, P.slabs = m, 32, 40, _lib.BF16, _lib.F32, 1
        P.dy_row_stride, P.x_row_stride, P.out_row_stride = 32, 40, 40
        P.dy, P.x, P.out = dy.data_ptr(), x.data_ptr(), out.data_ptr()
        for key, v in kw.items():
            setattr(P, key, v)
        return P

    # ZIGMA_ERR_NULL (-1)
    for field in ("dy", "x", "out"):
        _raises_status(-1, lambda: _lib.call("zigma_linear_wgrad", block(**{field: None}), dy.device))
    _raises_status(-1, lambda: _lib.call("zigma_linear_wgrad", block(slabs=2, workspace=None, workspace_bytes=1 << 20), dy.device))
    # ZIGMA_ERR_DTYPE (-3): fp32 operands, a mixed pair, an unknown type, an out type that is neither the operands' nor fp32
    _raises_status(-3, lambda: wg.wgrad_own(dy.float(), x.float(), out=out))
    _raises_status(-3, lambda: wg.wgrad_own(dy, x.to(torch.float16), out=out))
    _raises_status(-3, lambda: _lib.call("zigma_linear_wgrad", block(dtype=7), dy.device))
    _raises_status(-3, lambda: wg.wgrad_own(dy, x, out_dtype=torch.float16))
    assert wg.plan_wgrad(dy.float(), x.float()) == "bmm" and wg.plan_wgrad(dy, x.to(torch.float16)) == "bmm"
    # ZIGMA_ERR_SHAPE (-2): m < 1, n / k not a positive multiple of 8 or above 8192, slabs < 0, the workspace smaller than asked
    _raises_status(-2, lambda: _lib.call("zigma_linear_wgrad", block(m=0), dy.device))
    dy100 = torch.ones(m, 100, device=DEV, dtype=bf)
    _raises_status(-2, lambda: wg.wgrad_own(dy100, x))
    _raises_status(-2, lambda: _lib.call("zigma_linear_wgrad", block(k=0), dy.device))
    dy_wide = torch.ones(8, 8200, device=DEV, dtype=bf)
    _raises_status(-2, lambda: wg.wgrad_own(dy_wide, x[:8]))
    _raises_status(-2, lambda: wg.wgrad_own(dy, x, slabs=-1, out=out))
    small = torch.empty(16, device=DEV, dtype=torch.uint8)
    _raises_status(-2, lambda: wg.wgrad_own(dy, x, slabs=2, out=out, workspace=small))
    assert wg.plan_wgrad(dy100, x) == "bmm" and wg.plan_wgrad(dy_wide, x[:8]) == "bmm"
    # ZIGMA_ERR_STRIDE (-4): a row stride below the width or no multiple of 8, misaligned operands, misaligned out / out rows
    dy36 = torch.ones(m, 36, device=DEV, dtype=bf)[:, :32]
    _raises_status(-4, lambda: wg.wgrad_own(dy36, x, out=out))
    _raises_status(-4, lambda: _lib.call("zigma_linear_wgrad", block(x_row_stride=32), dy.device))
    x_off = torch.ones(m * 40 + 8, device=DEV, dtype=bf)[1:1 + m * 40].view(m, 40)
    _raises_status(-4, lambda: wg.wgrad_own(dy, x_off, out=out))
    out_off = torch.full((32 * 40 + 4,), 7.0, device=DEV, dtype=torch.float32)[1:1 + 32 * 40].view(32, 40)
    _raises_status(-4, lambda: wg.wgrad_own(dy, x, out=out_off))
    out_pitch = torch.full((32, 42), 7.0, device=DEV, dtype=torch.float32)[:, :40]
    _raises_status(-4, lambda: wg.wgrad_own(dy, x, out=out_pitch))
    assert wg.plan_wgrad(dy36, x) == "bmm" and wg.plan_wgrad(dy, x_off) == "bmm"
    torch.cuda.synchronize()
    assert not trace
    assert (out == 7.0).all() and (out_off == 7.0).all() and (out_pitch == 7.0).all()
    # ... and the same block, unchanged, is served
    _lib.call("zigma_linear_wgrad", block(), dy.device)
    assert [t[0] for t in trace] == ["zigma_linear_wgrad"] and trace[0][1].startswith("wgrad_") and (out == m).all()


# ---- 6. through autograd ----------------------------------------------------------------------------------------------------------------
LINEAR_TRAIN_KNOB = "all"       # no row of wgrad.PLAN_TABLE says "own" yet (the A/B is not measured), so the own kernel is asked for with the probe setting
MAMBA_KNOB = "all"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,K,Nf,bias", [(8192, 512, 640, True), (16384, 640, 2560, False)])
def test_linear_train_weight_gradient_on_the_own_kernel(M, K, Nf, bias, dtype, monkeypatch):
    from zigma_amd import _lib, wgrad as wg
    g = torch.Generator(device="cpu").manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(DEV, dtype).requires_grad_(True)
    w = (torch.randn(Nf, K, generator=g) * K ** -0.5).to(DEV, dtype).requires_grad_(True)
    b = (torch.randn(Nf, generator=g) * 0.1).to(DEV, dtype).requires_grad_(True) if bias else None
    dy = torch.randn(M, Nf, generator=g).to(DEV, dtype)
    want = N(ref64(dy, x.detach()))
    counts = {}
    for knob in (LINEAR_TRAIN_KNOB, False):
        monkeypatch.setattr(wg, "OWN_WGRAD", knob)
        x.grad = w.grad = None
        y = wg.linear_train(x, w, b)
        trace = []
        monkeypatch.setattr(_lib, "TRACE", trace)
        y.backward(dy)
        monkeypatch.setattr(_lib, "TRACE", None)
        counts[knob] = sum(1 for fn, _, _ in trace if fn == "zigma_linear_wgrad")
        err = rel_err(N(w.grad), want)
        print(f"linear_train {dtype} ({M}, {K}, {Nf}) OWN_WGRAD={knob}: dW vs float64 {err:.3e}")
        assert w.grad.dtype == dtype and err < (BOUND16[dtype] if knob else 2 * BOUND16[dtype]), (knob, err)     # (the library path: as in the production test)
        assert b is None or b.grad is not None
    assert counts == {LINEAR_TRAIN_KNOB: 1, False: 0}, counts


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_mamba_inner_weight_gradients_on_the_own_kernel(dtype, monkeypatch):
    """mamba_inner_tok under autograd with a zigzag table: d_dt_w and d_x_w come from zigma_linear_wgrad (twice in the backward's trace, the dt
    operand as the strided column view of x_dbl), each within the type's bound of the float64 product of the very operands the backward formed;
    with OWN_WGRAD = False the trace holds none and the parameter gradients agree within twice the bound"""
    import zigma_amd.selective_scan_interface as ssi
    from oracle import zigma_oracle as zo
    from zigma_amd import _lib, wgrad as wg
    g = torch.Generator(device="cpu").manual_seed(5)
    Bsz, L, Di, R, Nst = 2, 256, 256, 16, 16
    mk = lambda *s, sc=1.0, dt=dtype: (torch.randn(*s, generator=g) * sc).to(DEV, dt).requires_grad_(True)
    xz, cw, cb = mk(Bsz, L, 2 * Di), mk(Di, 1, 4, sc=0.5), mk(Di, sc=0.1)
    xw, dw = mk(R + 2 * Nst, Di, sc=Di ** -0.5), mk(Di, R, sc=R ** -0.5)
    A = (-torch.exp(torch.randn(Di, Nst, generator=g) * 0.5)).to(DEV).requires_grad_(True)
    D, db = mk(Di, dt=torch.float32), (torch.rand(Di, generator=g) * 0.5).to(DEV).requires_grad_(True)
    perm = torch.as_tensor(zo.zigzag_paths(16)[1].copy()).to(DEV, torch.int32)
    assert perm.shape == (L,)
    wgt = torch.randn(Bsz, L, Di, generator=g).to(DEV, dtype)
    leaves = (xz, cw, cb, xw, dw, A, D, db)
    seen = []
    real = ssi.wgrad

    def spy(dy2, x2):
        out = real(dy2, x2)
        seen.append((dy2.clone(), x2.clone(), x2.is_contiguous(), out))
        return out

    monkeypatch.setattr(ssi, "wgrad", spy)
    grads = {}
    for knob in (MAMBA_KNOB, False):
        monkeypatch.setattr(wg, "OWN_WGRAD", knob)
        for t in leaves:
            t.grad = None
        del seen[:]
        y = ssi.mamba_inner_tok(xz, cw, cb, xw, dw, A, D, db, perm=perm)
        trace = []
        monkeypatch.setattr(_lib, "TRACE", trace)
        (y.float() * wgt.float()).sum().backward()
        monkeypatch.setattr(_lib, "TRACE", None)
        n_own = sum(1 for fn, _, _ in trace if fn == "zigma_linear_wgrad")
        assert n_own == (2 if knob else 0), [t[:2] for t in trace]
        assert len(seen) == 2
        assert [c for _, _, c, _ in seen] == ([False, True] if knob else [True, True])     # the dt operand arrives uncopied only for the own kernel
        for dy2, x2, _, out in seen:
            err = rel_err(N(out), N(ref64(dy2, x2)))
            print(f"mamba_inner {dtype} OWN_WGRAD={knob} dW {tuple(out.shape)}: {err:.3e}")
            assert err < (BOUND16[dtype] if knob else 2 * BOUND16[dtype]), (knob, out.shape, err)
        grads[knob] = (xw.grad.clone(), dw.grad.clone())
    for a, b in zip(grads[MAMBA_KNOB], grads[False]):
        assert rel_err(N(a), N(b)) < 2 * BOUND16[dtype]
