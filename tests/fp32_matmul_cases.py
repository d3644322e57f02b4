"""Shared cases of the fp32-by-bf16-splitting projection (zigma_amd/fp32_matmul.py, csrc/linear_split.hip): test_fp32_matmul_cpu.py checks the torch
model on them, test_gpu_fp32_matmul.py the kernel.

Exact cases: small integers, so every bf16 product and every partial sum is an integer below 2^24 — exact in fp32 in ANY order of accumulation
(asserted per output: sum_k |x||w| < 2^24).  The expectations are formed in int64 from the planes of fp32_matmul.split.
  a: x in [-1023, 1023] (10 bits: about half of the x_lo are non-zero), w in [-2, 2] (w_lo = 0)  -> "high" is the int64 product: the x_lo w_hi term
  b: the roles swapped                                                                        -> the x_hi w_lo term
  c: both in [-362, 362]                                                                      -> "high" is sum(x w - x_lo w_lo): lo x lo is omitted
"""
import torch

# (kind, m, n, k)
EXACT = (("a", 136, 128, 1280), ("a", 8, 384, 192), ("b", 264, 128, 640), ("c", 136, 256, 64))
_RANGE = {"a": (1023, 2), "b": (2, 1023), "c": (362, 362)}

# (m, n, k): one tile / a partly filled second token tile / the four block projections' (n, k) at E = 640 and E = 768 / a long k
RANDOM = ((8, 128, 64), (136, 128, 192), (1024, 640, 1280), (2048, 2560, 640), (2048, 3072, 768), (1024, 512, 1536))
RANDOM_BIAS = (1, 3, 5)            # bias on every second case
RANDOM_VIEWS = (1, 4)              # x and out are views of wider rows on these two

_cache = {}


def exact_case(i):
    """{kind, x, w (fp32, CPU), high, medium, full (int64 expectations)} of EXACT[i]; computed once"""
    if i in _cache:
        return _cache[i]
    from zigma_amd.fp32_matmul import split
    kind, m, n, k = EXACT[i]
    rx, rw = _RANGE[kind]
    g = torch.Generator().manual_seed(1000 + i)
    x = torch.randint(-rx, rx + 1, (m, k), generator=g)
    w = torch.randint(-rw, rw + 1, (n, k), generator=g)
    assert int((x.abs() @ w.abs().t()).max()) < 2 ** 24
    (xh, xl), (wh, wl) = split(x.float()), split(w.float())
    xh, xl, wh, wl = (t.double().to(torch.int64) for t in (xh, xl, wh, wl))
    assert torch.equal(xh + xl, x) and torch.equal(wh + wl, w)             # at most 10 bits: hi + lo is the value
    full = x @ w.t()
    high = xh @ wh.t() + xl @ wh.t() + xh @ wl.t()
    medium = xh @ wh.t()
    assert torch.equal(high, full - xl @ wl.t())
    if kind == "a":
        assert torch.equal(high, full) and torch.equal(medium, xh @ w.t()) and float((xl != 0).float().mean()) > 0.4
        assert float((medium != full).float().mean()) > 0.95
    elif kind == "b":
        assert torch.equal(high, full) and float((wl != 0).float().mean()) > 0.4 and float((medium != full).float().mean()) > 0.95
    else:
        assert float((high != full).float().mean()) > 0.5
    _cache[i] = dict(kind=kind, x=x.float(), w=w.float(), high=high, medium=medium, full=full)
    return _cache[i]


def random_case(i, device="cpu"):
    """(x, w, bias | None) of RANDOM[i]: x ~ N(0, 1), w ~ N(0, 1) k^-1/2, generated on the CPU with a fixed seed"""
    m, n, k = RANDOM[i]
    g = torch.Generator().manual_seed(2000 + i)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    b = torch.randn(n, generator=g) if i in RANDOM_BIAS else None
    return x.to(device), w.to(device), None if b is None else b.to(device)
