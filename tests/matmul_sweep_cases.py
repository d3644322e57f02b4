"""Case tables of the sweep of the two matrix-core kernels outside zigma_linear_fwd: linear_split_kernel (csrc/linear_split.hip, "split": fp32
projections as bf16 split products, C ABI zigma_linear_f32_split) and wgrad_kernel / wgrad_reduce_kernel (csrc/wgrad.hip, "wgrad": dW = dY^T X,
C ABI zigma_linear_wgrad).

Plain numpy, importable without a GPU.  Seeded generators — split_cases(), wgrad_cases(), production_cases() — yield dicts of PARAMETERS with
stable ids; inputs(case) makes the numbers from the case's seed (the split: fp32 x and bias and the two bf16 weight planes as bit patterns;
wgrad: values already rounded to the operand type); fields(case) is the layout the GPU test builds (every operand a window of a NaN-filled
buffer: rows, cols, lead, pitch, NaN rows below) and the kernel string, restated from the host code's choice (the passes; wgrad_bk and
wgrad_slabs); split_reference / wgrad_reference evaluate in float64; split_model / wgrad_model are the fp32 numpy models of the kernels' order of accumulation.
tests/test_matmul_sweep_cases_cpu.py checks coverage, pins the references and the model; tests/test_gpu_matmul_sweep.py runs the kernels.

The split's definition (include/zigma_hip.h): hi = bf16_rne(a) clamped to the largest finite bf16, lo = bf16_rne(a - float(hi)); a non-finite a:
hi = bf16(a), lo = 0.  split() below is that function on bit patterns (held bit for bit against zigma_amd.fp32_matmul.split by the CPU test).

Limits — the project's own, none raised:
  split  element-wise |y - x w^T - bias| <= 2^-14 sum|x||w| ("high", 3 passes) / 2^-6 sum|x||w| ("medium", 1 pass) against the TRUE float64
         product, 2^-16 sum|x||w| against the float64 sums of the bf16-plane products (fp32_matmul.reference restated on the case's own planes),
         and row-wise rowwise_worst <= ROW_GUARD with the fp32 IO_BOUND against the plane reference on `benign` and `model` (the `edges` rows
         cancel by construction and are measured element-wise only);
  wgrad  norm-wise BOUND16 / BOUND32 of tests/test_gpu_wgrad.py, row-wise rowwise_worst <= ROW_GUARD over every output row, element-wise
         elementwise_worst <= ROW_GUARD (the backward sweep's measure for reduced gradients, max(|ref|, rms)); the `cancel` regime (every token
         paired with one of equal dy and opposite x half the tokens away: the true result is 0) element-wise over sum|dy||x| instead.
The fp32 model must need less than HALF of every limit (norm-wise before the output rounding — one 16-bit rounding alone is 0.65 ... 0.8 of the
norm-wise bound, fwd_fuzz_cases.model_excess — row- and element-wise after it); a case that does not would get another seed and be listed in
SEED_MOVED.  One restriction comes from the output TYPE, not from the kernel: the `model` regime's dy (1e-3 x 2^-10 ... 1) summed over fewer
than 1000 tokens is an fp16 SUBNORMAL result, which no 16-bit output can hold to 3.1e-4 — those fp16 cases take the fp32 output.
"""
import numpy as np

from bwd_fuzz_cases import ROW_GUARD, elementwise_worst, round_to, rowwise_worst  # noqa: F401  (re-exported)
from fwd_fuzz_cases import IO_BOUND, norm_err  # noqa: F401
from linear_cases import SELECT_C, wide_range

KINDS = ("bf16", "f16")
DTYPE_ID = {"f32": 0, "f16": 1, "bf16": 2}          # include/zigma_hip.h
SEED_MOVED = {}                                     # id -> seed
LEAD32, LEAD16 = 4, 8                               # NaN elements (16 bytes) in front of every window
FLT_MAX_BITS, MAX_BF16_BITS = 0x7f7fffff, 0x7f7f0000
FLT_MAX = float(np.array(FLT_MAX_BITS, np.uint32).view(np.float32))

# ---------------------------------------------------------------------------------------------------
# the split: bf16 on bit patterns
# ---------------------------------------------------------------------------------------------------
TOL_TRUE = {3: 2.0 ** -14, 1: 2.0 ** -6}            # against the true product, per passes
TOL_PLANES = 2.0 ** -16                             # against the float64 sums of the plane products
PLANE_QUANTUM = 2.0 ** -133                         # the spacing of bf16 subnormals: what a plane cannot resolve (see split_reference)
SPLIT_REGIMES = ("benign", "model", "edges")
SPLIT_M = (8, 120, 128, 136, 264, 392, 1016, 1032)
SPLIT_N = (128, 256, 384, 640)
SPLIT_K = (64, 128, 192, 320, 1536)
SPLIT_TILES = (1, 2, 3, 7, 8, 9, 15, 16, 24)
X_PADS, OUT_PADS = (0, 4, 64), (0, 4)
# at or above the largest finite bf16 (the slow branch of split8), and the two patterns just below the switch (the fast branch)
BIG = (0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, FLT_MAX_BITS, 0x7f7effff, 0x7f7e8000)
# the finite patterns below 2^100 of test_gpu_multi_cast.SPECIALS: +-0, bf16 ties and neighbours, fp16 ties, fp32 subnormals, fp16 edges
SPECIALS = (0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
            0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3F801001, 0x3F802FFF, 0x00000001, 0x007FFFFF, 0x00400000, 0x80000001, 0x00008000,
            0x00018000, 0x807FFFFF, 0x477FE000, 0x477FF000, 0x477FEFFF, 0xC77FF000, 0x47C35000, 0x33800000, 0x33000000, 0x33000001, 0x33C00000,
            0xB3C00000, 0x32FFFFFF, 0x38800000, 0x387FFFFF, 0x387FF000, 0x37280000, 0x3727C5AC)
EDGE_ROWS = dict(big=0, zero=1, big_neg=2, cancel=3, subnormal=4, lo_subnormal=5, specials=6, pow2=7)        # row r of every block of 8 edge rows


def bf16_bits(a):
    """fp32 -> bf16 bit patterns, round to nearest even (an overflow becomes inf; a NaN stays a quiet NaN)"""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(a), ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split(a):
    """-> (hi, lo) bf16 bit patterns of an fp32 array, by the header's definition"""
    a = np.ascontiguousarray(a, np.float32)
    finite, top = np.isfinite(a), bf16_value(MAX_BF16_BITS >> 16)
    hi = bf16_bits(np.where(finite, np.clip(a, -top, top), a))
    with np.errstate(invalid="ignore"):
        lo = bf16_bits(np.where(finite, a - bf16_value(hi), np.float32(0)).astype(np.float32))
    return hi, lo


def split_fields(c):
    """shape per operand: (rows, cols, lead, pitch, NaN rows below); x has NaN rows from m to the end of its last 128-row tile and one more"""
    m, n, k = c["m"], c["n"], c["k"]
    sh = dict(x=(m, k, LEAD32, k + c["x_pad"], -m % 128 + 1), w_hi=(n, k, LEAD16, k + 8, 1), w_lo=(n, k, LEAD16, k + 24, 1),
              out=(m, n, LEAD32, n + c["out_pad"], 1))
    if c["bias"]:
        sh["bias"] = (1, n, LEAD32, n + 4, 1)
    tiles = -(-m // 128) * (n // 128)
    return dict(shape=sh, kernel=f"linear_split{c['passes']}_128x128", tiles=tiles, remap=tiles % 8 == 0, ragged=m % 128 != 0)


def _scase(t, **kw):
    c = dict(kernel="split", passes=3, bias=False, x_pad=0, out_pad=0, regime="benign", known=None, nonfinite=None, seed=41000 + len(t))
    c.update(kw)
    assert c["m"] % 8 == 0 and c["n"] % 128 == 0 and c["k"] % 64 == 0
    c["id"] = (f"split{c['passes']}-{c['m']}x{c['n']}x{c['k']}" + ("-b" if c["bias"] else "") + f"-x{c['x_pad']}o{c['out_pad']}-{c['known'] or c['regime']}"
               + (f"-{c['regime']}" if c["known"] == "select" else "") + (f"-{c['nonfinite']}" if c["nonfinite"] else ""))
    if any(o["id"] == c["id"] for o in t):          # (a walk that meets a case of an earlier walk)
        return None
    c["seed"] = SEED_MOVED.get(c["id"], c["seed"])
    c.update(kernel_name=split_fields(c)["kernel"])
    t.append(c)
    return c


# (tiles, m, n): both sides of the XCD raster remap (gridDim % 8 == 0), each with a full and a ragged last token tile
TILE_WALK = ((1, 128, 128), (1, 120, 128), (1, 8, 128), (2, 256, 128), (2, 128, 256), (2, 136, 128), (3, 128, 384), (3, 264, 128), (7, 896, 128),
             (7, 888, 128), (8, 1024, 128), (8, 1016, 128), (8, 512, 256), (8, 392, 256), (9, 1152, 128), (9, 1032, 128), (9, 264, 384),
             (15, 384, 640), (15, 264, 640), (16, 1024, 256), (16, 1016, 256), (24, 1024, 384), (24, 1016, 384), (10, 136, 640), (5, 120, 640))


def split_cases():
    """Keys: passes (3 | 1), m, n, k, bias, x_pad / out_pad (elements a row pitch exceeds the row), regime, known (None | "select" | "exact-a" |
    "exact-b" | "exact-c" | "periodic": bit for bit), nonfinite (None | "+inf" | "-inf" | "nan"), kernel_name, seed"""
    t, i = [], 0
    for tiles, m, n in TILE_WALK:
        assert split_fields(dict(m=m, n=n, k=64, x_pad=0, out_pad=0, bias=False, passes=1))["tiles"] == tiles
        for passes in (3, 1):
            _scase(t, passes=passes, m=m, n=n, k=SPLIT_K[i % 5], bias=(i // 2 + i // 5) % 2 == 1, x_pad=X_PADS[i % 3], out_pad=OUT_PADS[(i // 3) % 2],
                   regime=SPLIT_REGIMES[(i + i // 3) % 3])
            i += 1
    for k in SPLIT_K:               # every k-step count (k = 64: one step, no prefetch) on grids of several tile columns, in every regime
        for passes in (3, 1):
            for regime in SPLIT_REGIMES:
                m, n = ((136, 256), (264, 384), (392, 256))[i % 3]
                _scase(t, passes=passes, m=m, n=n, k=k, bias=i % 2 == 0, x_pad=X_PADS[(i + 1) % 3], out_pad=OUT_PADS[i % 2], regime=regime)
                i += 1
    for passes in (3, 1):           # every cell passes x remap x ragged x bias, in the `edges` regime
        for m, n in ((1024, 128), (1016, 128), (256, 128), (264, 128)):
            for bias in (False, True):
                _scase(t, passes=passes, m=m, n=n, k=(128, 192)[bias], bias=bias, x_pad=4, out_pad=4, regime="edges", seed=41500 + len(t) + (not bias))
    # ---- known answers
    for passes in (3, 1):
        for regime in SPLIT_REGIMES:                # selection weights: every column of x shows (n >= k), the edge values included
            for m, n, k in ((136, 128, 64), (264, 256, 192), (1016, 384, 320)):
                _scase(t, passes=passes, m=m, n=n, k=k, regime=regime, known="select", x_pad=X_PADS[(m // 8) % 3], out_pad=OUT_PADS[(n // 128) % 2])
        _scase(t, passes=passes, m=136, n=640, k=1536, regime="edges", known="select", x_pad=4)
        for kind, m, n, k in (("a", 1032, 256, 1536), ("a", 392, 640, 320), ("b", 1016, 384, 192), ("b", 136, 128, 64), ("c", 264, 384, 128), ("c", 1016, 256, 64)):
            _scase(t, passes=passes, m=m, n=n, k=k, known=f"exact-{kind}", bias=m % 16 == 8 and kind != "c", x_pad=X_PADS[k // 64 % 3], out_pad=OUT_PADS[k // 64 % 2])
        for m, n, k, bias in ((1032, 384, 192, False), (1016, 256, 320, True), (392, 640, 64, False), (264, 128, 1536, True)):
            _scase(t, passes=passes, m=m, n=n, k=k, bias=bias, known="periodic", x_pad=X_PADS[n // 128 % 3], out_pad=OUT_PADS[m // 8 % 2])
    # ---- non-finite inputs: one element of one token row
    for j, (what, passes) in enumerate((("+inf", 3), ("-inf", 3), ("nan", 3), ("+inf", 1), ("-inf", 1), ("nan", 1))):
        _scase(t, passes=passes, m=(264, 136)[j % 2], n=256, k=(192, 64)[j % 2], bias=j % 2 == 0, x_pad=4, out_pad=4, nonfinite=what)
    return t


def edge_blocks(m):
    """first rows of the blocks of 8 edge rows: the first tile's, and the last 8 rows (inside a ragged last tile)"""
    return [0] if m < 16 else [0, m - 8]


def big_columns(k):
    """columns of the elements at the clamp: one in every second 16-byte piece of the first and of the last k-step — (column, its mirror in the
    other half of the row); positive patterns on row `big`, negative ones on row `big_neg`"""
    cols = [8 * p + p for p in (1, 3, 5, 7)]
    cols = cols + [k - 64 + c for c in cols] if k > 64 else cols
    return [(c, (c + k // 2) % k) for c in cols]


def _edge_x(rng, x, k):
    m = x.shape[0]
    bits = lambda pats, size: np.array(pats, np.uint32)[rng.integers(0, len(pats), size)].view(np.float32)
    for r0 in edge_blocks(m):
        R = {name: r0 + r for name, r in EDGE_ROWS.items()}
        for j, (c, _) in enumerate(big_columns(k)):
            x[R["big"], c] = np.array(BIG[j % len(BIG)], np.uint32).view(np.float32)
            x[R["big_neg"], c] = np.array(BIG[j % len(BIG)] | 0x80000000, np.uint32).view(np.float32)
        x[R["zero"]] = 0.0
        x[R["cancel"], k // 2:] = x[R["cancel"], :k // 2]
        x[R["subnormal"]] = (rng.integers(1, 0x800000, k).astype(np.uint32) | (rng.integers(0, 2, k).astype(np.uint32) << 31)).view(np.float32)
        x[R["lo_subnormal"]] = (rng.choice([-1.0, 1.0], k) * (1 + rng.random(k)) * 2.0 ** rng.integers(-124, -116, k)).astype(np.float32)
        x[R["specials"]] = bits(SPECIALS, k)
        x[R["specials"], :len(SPECIALS)] = np.array(SPECIALS, np.uint32).view(np.float32)[:k]
        x[R["pow2"]] = (rng.choice([-1.0, 1.0], k) * 2.0 ** rng.integers(-100, 100, k)).astype(np.float32)
    return x


def split_inputs(c):
    """-> dict(x (m, k) fp32, w (n, k) fp32: the value the planes stand for, w_hi / w_lo (n, k) uint16 bf16 patterns, bias (n) fp32 | None)"""
    rng = np.random.default_rng(c["seed"])
    m, n, k, known = c["m"], c["n"], c["k"], c["known"]
    rn = lambda *s: rng.standard_normal(s, dtype=np.float32)
    bias = None
    if known and known.startswith("exact"):         # fp32_matmul_cases.EXACT's three kinds: every product and partial sum an integer below 2^24
        rx, rw = {"a": (1023, 2), "b": (2, 1023), "c": (362, 362)}[known[-1]]
        x, w = rng.integers(-rx, rx + 1, (m, k)).astype(np.float32), rng.integers(-rw, rw + 1, (n, k)).astype(np.float32)
        bias = rng.integers(-8, 9, n).astype(np.float32) if c["bias"] else None
    elif known == "periodic":
        x, w = np.tile(rn(8, k), (m // 8, 1)), np.tile(rn(16, k) * np.float32(k ** -0.5), (n // 16, 1))
        bias = np.tile(0.3 * rn(16), n // 16) if c["bias"] else None
    else:
        x, w = rn(m, k), rn(n, k) * np.float32(k ** -0.5)
        bias = 0.3 * rn(n) if c["bias"] else None
        if c["regime"] == "model":                  # rows of magnitude 30 with a mean
            x = np.float32(30.0) * (x + rng.uniform(-1, 1, (m, 1)).astype(np.float32))
        if c["regime"] == "edges":
            x = _edge_x(rng, x, k)
            if c["seed"] % 2 == 0:                  # every w row is (b | -b): the rows (a | a) of x cancel in every feature
                w[:, k // 2:] = -w[:, :k // 2]
            w[[2, n - 3]] = 0.0
            for col, mirror in big_columns(k):      # small weights where x is at the clamp: no true sum leaves fp32
                w[:, col] = rng.choice([-1.0, 1.0], n).astype(np.float32) * np.float32(2.0 ** -12) * (1 + rng.random(n, dtype=np.float32))
                w[:, mirror] = -w[:, col]
            w[[2, n - 3]] = 0.0
    if known == "select":           # row j = c_j e_pi(j), w_lo = 0; c in {+-1, 1/2} where x is at the clamp (2 x would leave fp32)
        pi = np.concatenate([rng.permutation(k) for _ in range(-(-n // k))])[:n]
        cj = SELECT_C[rng.integers(0, 5, n)]
        near = np.isin(pi, [col for col, _ in big_columns(k)])
        cj[near] = np.array([1.0, -1.0, 0.5])[rng.integers(0, 3, n)][near]
        top = np.isin(pi, np.nonzero((x.view(np.uint32) == FLT_MAX_BITS).any(0))[0])
        cj[np.nonzero(top)[0][:1]] = 1.0            # FLT_MAX under a unit weight: +inf in "high", by the definition
        w = np.zeros((n, k), np.float32)
        w[np.arange(n), pi] = cj
    if c["nonfinite"]:
        x[c["m"] - 3, k - 5] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[c["nonfinite"]]
    w_hi, w_lo = split(w)
    return dict(x=x, w=w, w_hi=w_hi, w_lo=w_lo, bias=bias)


def nonfinite_at(c):
    return c["m"] - 3, c["k"] - 5


def planes(inp):
    """the four planes as float64 values"""
    xh, xl = split(inp["x"])
    return tuple(bf16_value(b).astype(np.float64) for b in (xh, xl, inp["w_hi"], inp["w_lo"]))


def split_reference(c, inp, rows=None):
    """-> dict(true: x w^T + bias, planes: the float64 sums of the bf16-plane products + bias (fp32_matmul.reference), mag: sum|x||w|, fmt), rows: a
    slice.  fmt = 2^-133 sum|w|: the number format's share of the limit against the TRUE product.  By the header's definition an x below 2^-117 has
    a `lo` on the bf16 SUBNORMAL grid (spacing 2^-133), so hi + lo misses x by up to 2^-134 whatever its size — 2^-7 of an fp32 subnormal — which no
    relative limit over sum|x||w| can hold for a row of such values.  The definition itself reaches half a spacing, and the fp32 model has to stay
    within half of every limit: the term is ONE spacing.  It is 9e-41 per unit of |w| and does not reach any other row."""
    rows = slice(None) if rows is None else rows
    x, w = inp["x"][rows].astype(np.float64), inp["w"].astype(np.float64)
    xh, xl, wh, wl = planes(inp)
    xh, xl = xh[rows], xl[rows]
    b = 0.0 if inp["bias"] is None else inp["bias"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = xh @ wh.T
        if c["passes"] == 3:
            y = y + (xl @ wh.T + xh @ wl.T)
        return dict(true=x @ w.T + b, planes=y + b, mag=np.abs(x) @ np.abs(w).T, fmt=PLANE_QUANTUM * np.abs(w).sum(1))


def split_row_reference(c, inp, r):
    """the plane reference of ONE token row by explicit products and sums (IEEE for inf and NaN whatever a BLAS does with them)"""
    xh, xl, wh, wl = planes(inp)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (xh[r] * wh).sum(1)
        if c["passes"] == 3:
            y = y + ((xl[r] * wh).sum(1) + (xh[r] * wl).sum(1))
    return y if inp["bias"] is None else y + inp["bias"].astype(np.float64)


def split_model(c, inp):
    """the kernel's order in fp32: 16-wide steps into the hi x hi accumulator and, apart, into the cross accumulator (x_lo w_hi, then x_hi w_lo),
    ONE fp32 add of the two, then the bias"""
    f = np.float32
    xh, xl, wh, wl = (p.astype(f) for p in planes(inp))
    acc, crs = np.zeros((c["m"], c["n"]), f), np.zeros((c["m"], c["n"]), f)
    for s in range(0, c["k"], 16):
        acc += xh[:, s:s + 16] @ wh[:, s:s + 16].T
        if c["passes"] == 3:
            crs += xl[:, s:s + 16] @ wh[:, s:s + 16].T
            crs += xh[:, s:s + 16] @ wl[:, s:s + 16].T
    with np.errstate(over="ignore"):        # (FLT_MAX under a unit weight: hi + lo is +inf)
        out = acc + crs if c["passes"] == 3 else acc
    return out if inp["bias"] is None else out + inp["bias"]


def split_known(c, inp):
    """the bit-for-bit expectation (fp32) of a known-answer case | None.  select: c (float(x_hi) + float(x_lo)) ("high") or c float(x_hi)
    ("medium") formed in fp32 — one rounding of the exact value; FLT_MAX under c = +1 is hi = 0x7f7f plus lo = 2^120 = 2^128: +inf, by the
    definition.  exact-*: the plane reference itself.  The accumulators start at +0, so a zero result is +0."""
    if not c["known"] or c["known"] == "periodic":
        return None
    if c["known"] == "select":
        xh, xl, wh, _ = planes(inp)
        j, col = np.nonzero(wh)
        assert len(j) == c["n"] and np.array_equal(j, np.arange(c["n"]))
        v = xh[:, col] + xl[:, col] if c["passes"] == 3 else xh[:, col]
        with np.errstate(over="ignore"):
            return (v * wh[j, col]).astype(np.float32) + np.float32(0)
    return split_reference(c, inp)["planes"].astype(np.float32) + np.float32(0)


def split_need(c, got, ref, mask=None):
    """what `got` needs of each limit, in units of the limit -> dict(true, planes[, rows]); mask: the elements that are measured (default: all)"""
    got = np.asarray(got, np.float64)
    mag = np.maximum(ref["mag"], 1e-300)
    mask = np.ones(got.shape, bool) if mask is None else mask
    with np.errstate(invalid="ignore"):
        worst = lambda err, limit: float(np.max(np.where(mask, err / limit, 0.0)))
        need = dict(true=worst(np.abs(got - ref["true"]), TOL_TRUE[c["passes"]] * mag + ref["fmt"]), planes=worst(np.abs(got - ref["planes"]), TOL_PLANES * mag))
    if c["regime"] != "edges" and not c["known"]:
        need["rows"] = rowwise_worst(got, ref["planes"], IO_BOUND["f32"]) / ROW_GUARD
    return need


# ---------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------
WG_BOUND16, WG_BOUND32 = {"bf16": 2.5e-3, "f16": 3.1e-4}, 2e-5          # tests/test_gpu_wgrad.py: BOUND16 / BOUND32 (held equal by the CPU test)
WG_N = (8, 24, 120, 128, 136, 264)
WG_K = (8, 40, 56, 64, 72, 120, 128, 136, 264)
WG_M = (1, 7, 8, 63, 64, 65, 127, 128, 129, 1000, 1024, 4104)
WG_SLABS = (0, 1, 2, 3, 5)
WG_REGIMES = ("benign", "model", "edges", "cancel")
INTS_NK = ((8, 8), (24, 40), (120, 56), (128, 64), (136, 72), (264, 120), (8, 128), (24, 136), (120, 264), (128, 128), (136, 264), (264, 64))       # per m of WG_M


def wgrad_bk(k):
    return 64 if k <= 64 else 128


def wgrad_slabs(m, n, k, slabs):
    """wgrad_slabs() of csrc/wgrad.hip"""
    if slabs > 0:
        return slabs
    bk = wgrad_bk(k)
    tiles = -(-n // 128) * -(-k // bk)
    return max(1, min(-(-512 // tiles), m // 512, 64))


def wgrad_fields(c):
    """shape per operand: (rows, cols, lead, pitch, NaN rows below): dy and x are column windows with NaN columns to their right and 64 NaN rows
    below; out rows are wider than k"""
    m, n, k = c["m"], c["n"], c["k"]
    S = wgrad_slabs(m, n, k, c["slabs"])
    sh = dict(dy=(m, n, LEAD16, LEAD16 + n + 16, 64), x=(m, k, LEAD16, LEAD16 + k + 8, 64), out=(n, k, LEAD32 if c["out32"] else LEAD16, k + c["out_pad"], 1))
    return dict(shape=sh, S=S, bk=wgrad_bk(k), slab_rows=-(-(-(-m // S)) // 64) * 64, workspace_bytes=S * n * k * 4 if S > 1 else 0,
                kernel=f"wgrad_128x{wgrad_bk(k)}" + ("_splitk" if S > 1 else ""))


def _wcase(t, **kw):
    c = dict(kernel="wgrad", kind="bf16", out32=False, slabs=0, regime="benign", known=None, seed=43000 + len(t))
    c.update(kw)
    if c["regime"] == "model" and c["kind"] == "f16" and c["m"] < 1000 and not c["known"]:
        c["out32"] = True               # (the module docstring: an fp16 subnormal result is the output type's limit)
    c.setdefault("out_pad", 4 if c["out32"] else 8)
    c["id"] = f"wgrad-{c['kind']}-{'f32' if c['out32'] else 'io'}-{c['m']}x{c['n']}x{c['k']}-s{c['slabs']}-{c['known'] or c['regime']}"
    if any(o["id"] == c["id"] for o in t):
        return None
    c["seed"] = SEED_MOVED.get(c["id"], c["seed"])
    f = wgrad_fields(c)
    c.update(kernel_name=f["kernel"], cell=(f["bk"], f["S"] > 1, c["out32"], c["kind"]))
    t.append(c)
    return c


def wgrad_cases():
    """Keys: kind (operand type), out32 (fp32 output; else the operand type), m, n, k, slabs (0: the library's choice), out_pad, regime, known
    (None | "select" | "ints": bit for bit), kernel_name, cell (BK, split-K, out32, kind), seed"""
    t, i = [], 0
    for n in WG_N:                  # every n x k: both sides of the 128 tile and of the BK switch at k = 64 | 72
        for k in WG_K:
            _wcase(t, m=WG_M[(i * 5) % 12], n=n, k=k, slabs=WG_SLABS[(i + i // 5) % 5], kind=KINDS[i % 2], out32=(i // 2) % 2 == 1, regime=WG_REGIMES[(i + i // 4) % 4])
            i += 1
    for mi, m in enumerate(WG_M):   # every m x slabs: sparse integers, equal across all slabs; and a value regime
        n, k = INTS_NK[mi]
        for si, slabs in enumerate(WG_SLABS):
            _wcase(t, m=m, n=n, k=k, slabs=slabs, kind=KINDS[mi % 2], out32=(mi // 2) % 2 == 0, known="ints", seed=43900 + mi)
            _wcase(t, m=m, n=n, k=k, slabs=slabs, kind=KINDS[(mi + si) % 2], out32=(mi + si // 2) % 2 == 0, regime=WG_REGIMES[(mi + si) % 4])
    for kind in KINDS:
        for out32 in (False, True):
            for m, n, k, slabs in ((1, 8, 56, 1), (8, 8, 8, 2), (7, 24, 40, 0), (64, 120, 72, 1), (128, 128, 64, 3), (129, 136, 136, 2), (127, 264, 264, 5)):
                _wcase(t, m=m, n=n, k=k, slabs=slabs, kind=kind, out32=out32, known="select")
            for bk_k in (56, 136):  # every cell BK x direct / split-K x output type x operand type, in every regime
                for slabs in (1, 3):
                    for regime in WG_REGIMES:
                        _wcase(t, m=1000, n=136, k=bk_k, slabs=slabs, kind=kind, out32=out32, regime=regime)
        for known, regime in (("ints", "benign"), (None, "benign"), (None, "edges")):        # slabs above the number of 64-token steps: empty slabs write zero partials
            _wcase(t, m=100, n=120, k=72, slabs=4, kind=kind, out32=kind == "f16", known=known, regime=regime)
        _wcase(t, m=4104, n=128, k=128, slabs=0, kind=kind)                                   # the library's own choice: 8 slabs
    return t


def production_cases():
    """one production shape per kernel, checked on every row: the split at 2048 x 640 x 1280 (out_proj of an fp32 model, "high"), wgrad's in_proj
    at 8192 tokens, bf16"""
    t = []
    _scase(t, passes=3, m=2048, n=640, k=1280, bias=True, seed=46000)
    _wcase(t, m=8192, n=2560, k=640, slabs=0, kind="bf16", seed=46001)
    for c in t:
        c["production"] = True
    return t


def ints_tokens(m):
    """tokens that must carry a non-zero term: the first and last of every 64-token step and of every slab, for every slab count of the sweep"""
    tok = set()
    for a in range(0, m, 64):
        tok |= {a, min(a + 63, m - 1)}
    for S in set(WG_SLABS[1:]) | {4, 8}:
        rows = -(-(-(-m // S)) // 64) * 64
        for a in range(0, m, rows):
            tok |= {a, min(a + rows - 1, m - 1)}
    return sorted(tok)


def wgrad_edges(m, n):
    tok = np.arange(m)
    plain = lambda u: u % 11 not in (1, 4) and u % 13 != 2 and u % 17 != 5
    pairs = np.array([t for t in range(6, m - 1, 16) if plain(t) and plain(t + 1)], np.int64)           # (token t + 1 = token t with x negated)
    return dict(zero_dy=tok[tok % 11 == 1], zero_x=tok[tok % 11 == 4], tiny=tok[tok % 13 == 2], top=tok[tok % 17 == 5], pairs=pairs, zero_cols=[1, n - 2])


def wgrad_inputs(c):
    """-> dict(dy (m, n), x (m, k)) float32 arrays holding values of the operand type"""
    rng = np.random.default_rng(c["seed"])
    m, n, k, kind = c["m"], c["n"], c["k"], c["kind"]
    rn = lambda *s: rng.standard_normal(s, dtype=np.float32)
    if c["known"] == "select":      # dy[t] = c_t e_nu(t), nu injective: out[nu(t)] = c_t x[t], every other row +0
        assert m <= n
        nu, ct = rng.permutation(n)[:m], SELECT_C[rng.integers(0, 5, m)]
        dy = np.zeros((m, n), np.float32)
        dy[np.arange(m), nu] = ct
        return dict(dy=dy, x=round_to(wide_range(rng, m, k), kind), nu=nu, ct=ct)
    if c["known"] == "ints":        # x in +-1 ... 3, never 0; one dy of +-1 per carrying token: every sum a small integer, exact in both types
        tok = np.array(sorted(set(ints_tokens(m)) | set(rng.integers(0, m, 8).tolist())))
        x = (rng.choice([-1.0, 1.0], (m, k)) * rng.integers(1, 4, (m, k))).astype(np.float32)
        dy = np.zeros((m, n), np.float32)
        dy[tok, rng.integers(0, n, len(tok))] = rng.choice([-1.0, 1.0], len(tok))
        return dict(dy=dy, x=x, tok=tok)
    dy, x = rn(m, n), rn(m, k)
    if c["regime"] == "model":      # small gradients with a per-token scale over 2^-10 ... 1 (partly fp16 subnormals), unit rows of x with a mean
        dy = np.float32(1e-3) * dy * (2.0 ** (-10 * rng.random((m, 1)))).astype(np.float32)
        x = x + np.float32(0.5)
        x /= np.sqrt(np.mean(x * x, -1, keepdims=True))
    if c["regime"] == "edges":
        e = wgrad_edges(m, n)
        dy[e["top"], ::3] = np.float32(6e4) * rng.choice([-1.0, 1.0], dy[e["top"], ::3].shape).astype(np.float32)       # the top of the fp16 range ...
        x[e["top"]] *= np.float32(2.0 ** -10)                                                                            # ... against small x
        dy[e["tiny"]] *= np.float32(2.0 ** -18)
        dy[e["zero_dy"]], x[e["zero_x"]] = 0.0, 0.0
        dy[e["pairs"] + 1], x[e["pairs"] + 1] = dy[e["pairs"]], -x[e["pairs"]]
        dy[:, e["zero_cols"]] = 0.0
    if c["regime"] == "cancel":     # every token t < m / 2 paired with token t + m / 2 (another step, another slab): equal dy, opposite x — the true result is exactly 0
        h = m // 2
        dy[h:2 * h], x[h:2 * h] = dy[:h], -x[:h]
        if m % 2:
            x[m - 1] = 0.0
    return dict(dy=round_to(dy, kind), x=round_to(x, kind))


def wgrad_reference(c, inp):
    """-> dict(out: float64 dy^T x on the rounded operands, mag: sum|dy||x|)"""
    dy, x = inp["dy"].astype(np.float64), inp["x"].astype(np.float64)
    return dict(out=dy.T @ x, mag=np.abs(dy).T @ np.abs(x))


def wgrad_model(c, inp):
    """the kernel's order in fp32: 64-token steps inside a slab, the slabs in ascending order; unrounded (fp32)"""
    f = wgrad_fields(c)
    dy, x = inp["dy"].astype(np.float32), inp["x"].astype(np.float32)
    parts = []
    for s in range(f["S"]):
        acc = np.zeros((c["n"], c["k"]), np.float32)
        for a in range(s * f["slab_rows"], min((s + 1) * f["slab_rows"], c["m"]), 64):
            b = min(a + 64, (s + 1) * f["slab_rows"], c["m"])
            acc += dy[a:b].T @ x[a:b]
        parts.append(acc)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def wgrad_bound(c):
    return WG_BOUND32 if c["out32"] else WG_BOUND16[c["kind"]]


def wgrad_need(c, got, ref, norm_of=None):
    """what `got` needs of each limit, in units of the limit -> dict(norm, rows, elements) | dict(cancel); norm_of: another array for the norm-wise figure"""
    got, bound = np.asarray(got, np.float64), wgrad_bound(c)
    if c["regime"] == "cancel" and not c["known"]:
        return dict(cancel=float(np.max(np.abs(got - ref["out"]) / (bound * np.maximum(ref["mag"], 1e-300)))))
    return dict(norm=norm_err(got if norm_of is None else norm_of, ref["out"]) / bound, rows=rowwise_worst(got, ref["out"], bound) / ROW_GUARD,
                elements=elementwise_worst(got, ref["out"], bound) / ROW_GUARD)


def wgrad_known(c, inp):
    """the exact answer (float64; exact in both types) of a known-answer case | None"""
    if not c["known"]:
        return None
    if c["known"] == "select":
        out = np.zeros((c["n"], c["k"]))
        out[inp["nu"]] = inp["ct"][:, None] * inp["x"].astype(np.float64)
        return out
    return inp["dy"].astype(np.float64).T @ inp["x"].astype(np.float64)


def inputs(c):
    return split_inputs(c) if c["kernel"] == "split" else wgrad_inputs(c)


def fields(c):
    return split_fields(c) if c["kernel"] == "split" else wgrad_fields(c)
