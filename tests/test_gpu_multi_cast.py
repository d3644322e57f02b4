"""GPU tests of zigma_multi_cast_fwd (csrc/multi_cast.hip): many fp32 tensors rounded to bf16 / fp16 in one launch, through zigma_amd.amp.

Reference: `tensor.to(dtype)` on the device, compared BIT for bit (int16 views, so that -0 and +0 differ).  Sources are windows of a NaN-filled buffer,
destinations windows of a sentinel-filled one; whatever the kernel reads or writes outside its windows shows."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 0x5A5A

# fp32 bit patterns every tensor of the sweep starts with (as far as it is long enough)
SPECIALS = [
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                      # +-0, +-inf
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                      # bf16 ties: to even downwards / upwards, both signs
    0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,                      # ... and their neighbours
    0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3F801001, 0x3F802FFF,      # fp16 ties (13 dropped bits) and neighbours
    0x00000001, 0x007FFFFF, 0x00400000, 0x80000001, 0x00008000, 0x00018000, 0x807FFFFF,       # fp32 denormals (bf16 denormal results, a tie among them)
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000,                      # the largest fp32 (bf16: inf), the largest bf16, the tie above it
    0x477FE000, 0x477FF000, 0x477FEFFF, 0xC77FF000, 0x47C35000,          # fp16: 65504, the tie to inf, just below it, 1e5
    0x33800000, 0x33000000, 0x33000001, 0x33C00000, 0xB3C00000, 0x32FFFFFF,      # fp16 subnormal results: 2^-24, the tie to 0, above it, 3 * 2^-25, below 2^-25
    0x38800000, 0x387FFFFF, 0x387FF000, 0x37280000, 0x3727C5AC,          # 2^-14 and just below (rounds up to the smallest normal), a tie, 1e-5
]


def _values(n, gen):
    """n fp32 values without NaN: the specials, then random bit patterns and random normal values of many magnitudes"""
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    normal = (torch.randn(n, generator=gen) * torch.pow(10.0, torch.randint(-9, 6, (n,), generator=gen).float())).view(torch.int32)
    v = torch.where(torch.rand(n, generator=gen) < 0.5, bits, normal)
    sp = torch.tensor(SPECIALS, dtype=torch.int64).to(torch.int32)[:n]
    v[:sp.numel()] = sp
    f = v.view(torch.float32)
    return torch.where(torch.isnan(f), torch.ones_like(f), f)


def _layout(dtype, seed):
    """>= 300 tensors in one NaN-filled source and one sentinel-filled destination buffer: the sizes around every path of the kernel, source windows at
    element offsets 0 ... 3, destination windows at odd element offsets (never 16-byte aligned: the element-wise path), and 48 more on 16-byte boundaries
    (the 8-elements-per-lane path and its tail)"""
    from zigma_amd import amp
    C = amp.CHUNK
    sizes = [0, 1, 7, 8, 9, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5]
    plan = [(n, i % 4, 1 + 2 * (i % 4)) for i, n in enumerate(sizes * 26)] + [(n, 0, 0) for n in sizes * 4]
    gen = torch.Generator().manual_seed(seed)
    s_at = d_at = 0
    wins = []
    for n, so, do in plan:
        s0, d0 = -(-s_at // 4) * 4 + so, -(-d_at // 8) * 8 + 8 + do
        wins.append((s0, d0, n))
        s_at, d_at = s0 + n + 3, d0 + n + 5
    src = torch.full((s_at + 16,), float("nan"))
    for s0, _, n in wins:
        src[s0:s0 + n] = _values(n, gen)
    src = src.to(DEV)
    dst = torch.full((d_at + 16,), SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    srcs = [src[s0:s0 + n] for s0, _, n in wins]
    dsts = [dst[d0:d0 + n] for _, d0, n in wins]
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    return src, dst, srcs, dsts, wins


def _check(dst, srcs, dsts, wins, dtype):
    outside = torch.ones(dst.numel(), dtype=torch.bool, device=DEV)
    for (_, d0, n), s, d in zip(wins, srcs, dsts):
        assert torch.equal(d.view(torch.int16), s.to(dtype).view(torch.int16)), (d0, n)
        outside[d0:d0 + n] = False
    assert bool((dst.view(torch.int16)[outside] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_over_many_tensors_is_bit_equal_to_to(dtype):
    from zigma_amd import _lib, amp
    src, dst, srcs, dsts, wins = _layout(dtype, 11)
    assert len(srcs) >= 300
    n_wide = sum(1 for s, d in zip(srcs, dsts) if s.numel() >= 8 and s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0)
    assert n_wide >= 24 and all(d.data_ptr() % 4 == 2 for d in dsts[:312] if d.numel())
    trace = []
    _lib.TRACE = trace
    try:
        keep = amp.cast_tensors(srcs, dsts)
    finally:
        _lib.TRACE = None
    assert [t[:2] for t in trace] == [("zigma_multi_cast_fwd", "multi_cast_bf16" if dtype == torch.bfloat16 else "multi_cast_f16")]      # ONE launch
    _check(dst, srcs, dsts, wins, dtype)
    first = dst.clone()
    amp.cast_tensors(srcs, dsts)
    assert torch.equal(first.view(torch.int16), dst.view(torch.int16))
    # the overflow / subnormal cases really are in the set
    big = torch.tensor([0x7F7FFFFF, 0x477FF000, 0x33800000], dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV).to(dtype)
    assert bool(torch.isinf(big[0])) and (dtype == torch.bfloat16 or (bool(torch.isinf(big[1])) and float(big[2]) == 2.0 ** -24))
    del keep


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_nan_and_one_entry(dtype):
    from zigma_amd import amp
    pats = torch.tensor([0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0xFFC00000, 0x7FFFFFFF, 0x3F800000] * 3, dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)
    out = torch.zeros(pats.numel(), device=DEV, dtype=dtype)
    amp.cast_tensors([pats], [out])                                   # count 1, the aligned path and its tail
    assert torch.equal(torch.isnan(out), torch.isnan(pats)) and float(out[5]) == 1.0
    out2 = torch.zeros(pats.numel() + 1, device=DEV, dtype=dtype)[1:]
    amp.cast_tensors([pats], [out2])                                  # ... and element by element
    assert torch.equal(torch.isnan(out2), torch.isnan(pats)) and float(out2[5]) == 1.0


def test_count_zero_refusals_and_rows_outside_the_table():
    """count 0 launches nothing and is ZIGMA_OK; every refusal comes back with its status before anything is launched; a chunk-map row that points
    outside the table (or past a tensor's end) is skipped — the destination keeps its sentinel in all of them"""
    from zigma_amd import _lib
    L = _lib.lib()
    src = torch.randn(64, device=DEV)
    dst = torch.full((64,), SENTINEL, dtype=torch.int16, device=DEV)
    table = torch.tensor([[src.data_ptr(), dst.data_ptr(), 64]], dtype=torch.int64).to(DEV)
    cmap = torch.tensor([[0, 0]], dtype=torch.int64).to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        P = _lib.MultiCastParams()
        P.table, P.chunk_map, P.n_entries, P.n_chunks, P.out_dtype, P.chunk, P.flags = table.data_ptr(), cmap.data_ptr(), 1, 1, _lib.BF16, 4096, 0
        for k, v in kw.items():
            setattr(P, k, v)
        rc = L.zigma_multi_cast_fwd(ctypes.byref(P), stream)
        torch.cuda.synchronize()
        return rc

    OK, NULL, SHAPE, DTYPE, UNSUPPORTED = 0, -1, -2, -3, -6
    cases = [(dict(n_entries=0), OK), (dict(n_chunks=0), OK), (dict(n_entries=0, n_chunks=0, table=None, chunk_map=None), OK),
             (dict(table=None), NULL), (dict(chunk_map=None), NULL),
             (dict(n_entries=-1), SHAPE), (dict(n_chunks=-1), SHAPE), (dict(chunk=0), SHAPE), (dict(chunk=12), SHAPE), (dict(chunk=-4096), SHAPE),
             (dict(out_dtype=_lib.F32), DTYPE), (dict(out_dtype=7), DTYPE), (dict(out_dtype=-1), DTYPE),
             (dict(flags=1), UNSUPPORTED), (dict(flags=1, n_entries=0), UNSUPPORTED), (dict(out_dtype=7, n_chunks=0), DTYPE), (dict(n_entries=-1, out_dtype=7), SHAPE)]
    for kw, want in cases:
        assert call(**kw) == want, (kw, want)
        assert bool((dst == SENTINEL).all()), kw
    for row in ([1, 0], [-1, 0], [0, 64], [0, -8], [0, 1 << 40]):
        cmap.copy_(torch.tensor([row], dtype=torch.int64))
        assert call() == OK and bool((dst == SENTINEL).all()), row
    cmap.copy_(torch.tensor([[0, 0]], dtype=torch.int64))
    assert call() == OK
    assert torch.equal(dst.view(torch.bfloat16), src.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="status -3"):
        from zigma_amd import amp
        amp.multi_cast(table, cmap, 1, 1, torch.float32, src.device)
