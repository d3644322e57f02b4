"""GPU tests of zigma_linear_f32_split (csrc/linear_split.hip) and its dispatch: fp32 projections as split bf16 products on the matrix cores.

Measured on an MI355X (printed by the tests): see DESIGN.md §3.4."""
import pytest
import torch
import torch.nn.functional as F

from fp32_matmul_cases import EXACT, RANDOM, RANDOM_VIEWS, exact_case, random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def mode():
    """sets fp32_matmul.PRECISION for one test and puts "highest" back"""
    import zigma_amd
    yield zigma_amd.set_float32_matmul_precision
    zigma_amd.set_float32_matmul_precision("highest")


@pytest.fixture
def trace():
    from zigma_amd import _lib
    _lib.TRACE = []
    yield _lib.TRACE
    _lib.TRACE = None


def split_calls(tr):
    return [(name, kern, P) for name, kern, P in tr if name == "zigma_linear_f32_split"]


# ---- 1. exact, bit for bit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(EXACT)))
def test_exact_integer_products(i):
    """every product and partial sum is an integer below 2^24: the kernel must return the int64 expectation exactly — the operand maps, the plane
    addressing, the tile edges (m = 8, 136, 264: a partly filled last token tile; n = 128 ... 384) and the k loop, with no tolerance"""
    from zigma_amd.fp32_matmul import linear_split
    c = exact_case(i)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    for m in ("high", "medium"):
        y = linear_split(x, w, mode=m)
        torch.cuda.synchronize()
        bad = int((y.cpu().double() != c[m].double()).sum())
        assert bad == 0, (EXACT[i], m, bad)
    assert not torch.equal(c["high"], c["medium"])


# ---- 2. random operands against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(RANDOM)))
def test_random_operands_vs_float64(i):
    """element-wise |y - ref| <= 2^-14 sum|x||w| ("high": 3 x 2^-16 is the split's worst case, 2^-16 is left for the fp32 accumulation) and
    2^-6 sum|x||w| ("medium"); norm-wise err_high <= err_medium / 64 and err_medium <= 4e-3 — on 512 sampled rows plus the first and the last"""
    from zigma_amd.fp32_matmul import linear_split
    m, n, k = RANDOM[i]
    x, w, b = random_case(i, DEV)
    out = None
    if i in RANDOM_VIEWS:                                    # x and out as views of wider rows; what lies beside them must stay untouched
        xw = torch.full((m, k + 64), 7.0, device=DEV)
        xw[:, 32:32 + k] = x
        x = xw[:, 32:32 + k]
        ow = torch.full((m, n + 8), -3.0, device=DEV)
        out = ow[:, 4:4 + n]
    g = torch.Generator().manual_seed(i)
    rows = torch.unique(torch.cat([torch.tensor([0, m - 1]), torch.randint(0, m, (512,), generator=g)])).to(DEV)
    xs = x[rows].double()
    ref = xs @ w.double().t() + (0 if b is None else b.double())
    bound = xs.abs() @ w.double().abs().t()
    err = {}
    for md, tol in (("high", 2.0 ** -14), ("medium", 2.0 ** -6)):
        y = linear_split(x, w, b, mode=md, out=out)
        torch.cuda.synchronize()
        assert y.shape == (m, n) and y.dtype == torch.float32
        d = (y[rows].double() - ref).abs()
        err[md] = float((y[rows].double() - ref).norm() / ref.norm())
        worst = float((d / bound).max())
        print(f"fp32_split {md:6s} m={m} n={n} k={k} bias={b is not None} views={out is not None}: norm-wise {err[md]:.3e}, worst |y-ref|/sum|x||w| {worst:.3e} (bound {tol:.3e})")
        assert bool((d <= tol * bound).all()), (RANDOM[i], md, worst)
        if out is not None:
            assert bool((ow[:, :4] == -3.0).all()) and bool((ow[:, 4 + n:] == -3.0).all())
    assert err["high"] <= err["medium"] / 64 and err["medium"] <= 4e-3, (RANDOM[i], err)


# ---- 3. refusals and dispatch ---------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_and_split_eligible_agrees():
    from zigma_amd.fp32_matmul import linear_split, split_eligible
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, device=DEV, dtype=dtype)
    good = (z(16, 128), z(128, 128))
    assert split_eligible(*good) and linear_split(*good, mode="high").shape == (16, 128)
    refused = {"k = 96": (z(16, 96), z(128, 96)), "n = 200": (z(16, 128), z(200, 128)), "an odd pointer": (z(17, 132)[1:, 1:129], z(128, 128)),
               "an fp16 x": (z(16, 128, dtype=torch.float16), z(128, 128))}
    for why, (x, w) in refused.items():
        assert not split_eligible(x, w), why
        with pytest.raises(RuntimeError):
            linear_split(x, w, mode="high")
    torch.cuda.synchronize()


def test_project_dispatch_at_e640(mode, trace):
    """"high": one zigma_linear_f32_split call per block projection, kernel linear_split3..., passes == 3; "highest": none, and F.linear bit for bit"""
    import zigma_amd.routing as zr
    from zigma_amd.fp32_matmul import reference
    from zigma_amd.linear import project
    g = torch.Generator().manual_seed(3)
    shapes = {"in_proj": (2560, 640), "out_proj": (640, 1280), "to_q": (512, 640), "to_out": (640, 512)}
    ops = {}
    for role, (n, k) in shapes.items():
        ops[role] = (torch.randn(8, 256, k, generator=g).to(DEV), (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV),
                     torch.randn(n, generator=g).to(DEV) if role == "to_out" else None)
    with torch.no_grad():
        for role, (x, w, b) in ops.items():
            y0 = project(role, x, w, b)
            assert torch.equal(y0, F.linear(x, w, b)), role
        assert split_calls(trace) == []
        mode("high")
        for role, (x, w, b) in ops.items():
            del trace[:]
            y = project(role, x, w, b)
            calls = split_calls(trace)
            assert len(calls) == 1 and len(trace) == 1, (role, [t[:2] for t in trace])
            _, kern, P = calls[0]
            n, k = shapes[role]
            assert kern.startswith("linear_split3") and kern.startswith(zr.kernel_name("split3")) and (P.passes, P.m, P.n, P.k) == (3, 2048, n, k)
            # against the same three products accumulated in float64 only the fp32 accumulation is left: its 2^-16 share of the element-wise bound
            ref = reference(x.reshape(-1, k), w, b, "high").view(8, 256, n)
            bound = (x.reshape(-1, k).double().abs() @ w.double().abs().t()).view(8, 256, n)
            assert bool(((y.double() - ref).abs() <= 2.0 ** -16 * bound).all()), role
        # the gated add of a split route stays outside the kernel: residual + gate * y
        x, w, b = ops["to_out"]
        res, gate = torch.randn(8, 256, 640, generator=g).to(DEV), torch.randn(8, 640, generator=g).to(DEV)
        y = project("to_out", x, w, b)
        assert torch.equal(project("to_out", x, w, b, residual=res, gate=gate), torch.addcmul(res, gate.unsqueeze(1), y))
        mode("medium")
        del trace[:]
        project("in_proj", *ops["in_proj"])
        assert [(t[1], t[2].passes) for t in split_calls(trace)] == [("linear_split1_128x128", 1)]
        # under autograd every mode is today's path
        mode("high")
        del trace[:]
    x, w, _ = ops["in_proj"]
    wg = w.clone().requires_grad_(True)
    yg = project("in_proj", x, wg)
    assert split_calls(trace) == [] and yg.requires_grad and torch.equal(yg.detach(), F.linear(x, w))


# ---- 4. model level -----------------------------------------------------------------------------------------------------------------------------------
def test_model_forward_in_the_three_modes(mode, trace):
    from zigma_amd.graphs import GraphedForward
    from zigma_amd.model_zigma import ZigMa
    depth = 2
    torch.manual_seed(0)
    model = ZigMa(in_channels=4, embed_dim=128, depth=depth, img_dim=8, has_text=True, d_context=32, n_context_token=8, scan_type="zigzagN8", use_pe=2,
                  device=DEV, dtype=torch.float32).eval()
    with torch.no_grad():
        for blk in model.blocks:
            blk.adaLN_modulation[-1].weight.normal_(std=0.3)
            blk.adaLN_modulation[-1].bias.normal_(std=0.3)
    g = torch.Generator().manual_seed(1)
    x, t, y = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.rand(2, generator=g).to(DEV), torch.randn(2, 8, 32, generator=g).to(DEV)
    v = {}
    with torch.no_grad():
        v["highest"] = model(x, t, y)
        assert split_calls(trace) == []
        for md in ("high", "medium"):
            mode(md)
            del trace[:]
            v[md] = model(x, t, y)
            calls = split_calls(trace)
            assert all(c[1].startswith("linear_split3" if md == "high" else "linear_split1") for c in calls)
            # every block projection: in_proj (4E x E), out_proj (E x 2E), to_q (512 x E), to_out (E x 512) per block ...
            nk = [(c[2].n, c[2].k) for c in calls]
            for shape in ((512, 128), (128, 256), (128, 512)):
                assert nk.count(shape) == (2 * depth if shape == (512, 128) else depth), (md, nk)
            # ... plus the text rows the kernel can take: the batched K / V of all blocks (k = E); the y_embedder's k = d_context = 32 is below its limits
            assert sorted(set(nk) - {(512, 128), (128, 256), (128, 512)}) == [(depth * 2 * 512, 128)] and len(calls) == 4 * depth + 1, (md, nk)
        mode("high")
        graphed = GraphedForward(model, x, t, y)
        del trace[:]
        vg = graphed(x, t, y)
        assert torch.equal(vg, v["high"])                                   # bit for bit: the weight planes come from the cache, not from the capture
        assert torch.equal(model(x, t, y), v["high"])
    torch.cuda.synchronize()
    d = {md: float((v[md].double() - v["highest"].double()).norm() / v["highest"].double().norm()) for md in ("high", "medium")}
    print(f"fp32_split model level: d_high {d['high']:.3e}, d_medium {d['medium']:.3e}")
    assert d["medium"] <= 1e-2 and d["high"] <= d["medium"] / 64, d


def test_mode_is_back_to_highest():
    import zigma_amd
    assert zigma_amd.get_float32_matmul_precision() == "highest"
