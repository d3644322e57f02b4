"""The dense projections after their predicates ask the library's plans: at the smallest shape that reaches each kernel family, the parameter block that
was launched — plan()'s accepted block, where the call went through linear.project — is byte for byte the block the plain builder makes for those tensors,
the kernel that served it is the one the plan query named, and the result holds the float64 bound of that kernel's own test."""
import pytest
import torch

from test_gpu_norm_linear import EPS, _float64, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture
def trace():
    from zigma_amd import _lib
    _lib.lib()
    _lib.TRACE = []
    yield _lib.TRACE
    _lib.TRACE = None


def _operands(lead, n, k, bias, gated, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*lead, k, generator=g).to(DEV, BF)
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, BF)
    b = None
    if bias is not None:                # bias: bytes off a 16-byte boundary
        b = (torch.randn(n + 8, generator=g) * 0.3).to(DEV, BF)[bias // 2:bias // 2 + n]
        assert b.data_ptr() % 16 == bias
    res = torch.randn(*lead, n, generator=g).to(DEV, BF) if gated else None
    gate = torch.randn(lead[0], n, generator=g).to(DEV, BF) if gated else None
    return x, w, b, res, gate


# (id, how, role / selector, lead dims of x, n, k, bias, gated residual, POLICY, the kernel the family must report)
LINEAR = [
    ("8-wave", "project", "to_out", (8,), 128, 64, 0, False, "auto", "linear_tn_256x128"),
    ("4-wave", "project", "text", (4096,), 4096, 192, None, False, "auto", "linear4w_256x256"),
    ("4-wave gated", "project", "out_proj", (16, 256), 4096, 192, None, True, "all", "linear4w_256x256"),
    ("few-token", "linear", "sm", (128,), 128, 128, 8, False, "auto", "linear_sm_128x128"),
    ("weight-stationary", "project", "train", (512,), 8192, 512, None, False, "auto", "linear_ws"),
    ("weight-stationary 128", "project", "train", (512,), 4096, 1280, None, False, "auto", "linear_ws_128"),
]


@pytest.mark.parametrize("name,how,role,lead,n,k,bias,gated,policy,kernel", LINEAR, ids=[c[0] for c in LINEAR])
def test_linear_block_kernel_and_result(name, how, role, lead, n, k, bias, gated, policy, kernel, trace, monkeypatch):
    from zigma_amd import _lib, linear as zl, routing as zr
    monkeypatch.setattr(zr, "POLICY", policy)
    x, w, b, res, gate = _operands(lead, n, k, bias, gated, seed=n + k)
    with torch.no_grad():
        if how == "project":
            r = zl.plan(role, x, w, b, res, gate)
            assert r.kernel in zl.FAMILY_FLAG and r.fuse_add == gated and r.block is not None, r
            flags = zl.FAMILY_FLAG[r.kernel]
            y = zl.project(role, x, w, b, residual=res, gate=gate)
        else:
            flags = zl.FAMILY_FLAG[role]
            y = zl.linear(x, w, b, few_tokens=True)
    torch.cuda.synchronize()
    assert [fn for fn, _, _ in trace] == ["zigma_linear_fwd"], [t[:2] for t in trace]
    _, served, P = trace[0]
    tokens = x.numel() // k
    built = zl.linear_block(x.view(tokens, k), w, b, y.view(tokens, n), res, gate, flags=flags)
    assert bytes(P) == bytes(built)
    assert _lib.plan("zigma_linear_fwd", built) == (0, served) and served == kernel
    ref = x.view(tokens, k).double() @ w.double().T + (b.double() if b is not None else 0)
    if gated:
        ref = res.view(tokens, n).double() + gate.double().repeat_interleave(lead[1], 0) * ref
    err = float((y.view(tokens, n).double() - ref).norm() / ref.norm())
    print(f"linear plan query {name} ({tokens}, {n}, {k}) -> {served}: {err:.3e}")
    assert err < 4e-3


def test_norm_linear_block_kernel_and_result(trace):
    from zigma_amd import _lib
    from zigma_amd.norm_linear import norm_linear, norm_linear_block, norm_linear_eligible
    x, w, shift, scale = _inputs(128, 512, 128, BF, seed=7)
    assert x.shape == (1, 128, 512) and norm_linear_eligible(x, w, shift, scale)
    got = norm_linear(x, w, shift, scale, EPS).view(128, 512)
    torch.cuda.synchronize()
    assert [fn for fn, _, _ in trace] == ["zigma_norm_linear_fwd"]
    _, served, P = trace[0]
    built = norm_linear_block(x, w, shift, scale, EPS, got)
    assert bytes(P) == bytes(built)
    assert _lib.plan("zigma_norm_linear_fwd", built) == (0, served) and served == "norm_linear_k512"
    ref = _float64(x, w, shift, scale, BF)
    err = float((got.double() - ref).norm() / ref.norm())
    print(f"norm_linear plan query (1, 128, 512) -> {served}: {err:.3e}")
    assert err < 2.5e-3 and torch.allclose(got.double(), ref, rtol=1.6e-2, atol=1e-2)


def test_linear_split_block_kernel_and_result(trace):
    from zigma_amd import _lib
    from zigma_amd.fp32_matmul import linear_split, linear_split_block, split_eligible, split_weight
    g = torch.Generator(device="cpu").manual_seed(11)
    x, w = torch.randn(8, 64, generator=g).to(DEV), (torch.randn(128, 64, generator=g) * 0.125).to(DEV)
    assert split_eligible(x, w)
    ref = x.double() @ w.double().T
    bound = x.double().abs() @ w.double().abs().T
    err = {}
    for mode, passes, tol in (("high", 3, 2.0 ** -14), ("medium", 1, 2.0 ** -6)):
        del trace[:]
        y = linear_split(x, w, mode=mode)
        torch.cuda.synchronize()
        assert [fn for fn, _, _ in trace] == ["zigma_linear_f32_split"]
        _, served, P = trace[0]
        built = linear_split_block(x, *split_weight(w), None, y, passes)
        assert bytes(P) == bytes(built)
        assert _lib.plan("zigma_linear_f32_split", built) == (0, served) and served == f"linear_split{passes}_128x128"
        err[mode] = float((y.double() - ref).norm() / ref.norm())
        print(f"linear_split plan query {mode} (8, 128, 64) -> {served}: {err[mode]:.3e}")
        assert bool(((y.double() - ref).abs() <= tol * bound).all())
    assert err["high"] <= err["medium"] / 64 and err["medium"] <= 4e-3, err
