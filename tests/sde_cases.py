"""Case table of the SDE step kernel, zigma_sde_step_fwd (csrc/sde_step.hip), and a numpy restatement of everything the header defines:
Philox4x32-10, the map from a quad's four words to its four normals (in float64, and step by step in float32), and one launch
out = c0 a + c1 b + c2 c + cn xi in float64.  Plain numpy, importable without a GPU.  tests/test_sde_cases_cpu.py pins the restatement to the
generator's published known answers and checks the table; tests/test_gpu_sde.py runs the kernels.

Limits.  An output element may miss the float64 value by
    u(dtype) |ref| + 2^-24 (4 sum|terms| + NORMAL_K |cn| max(|xi|, 2^-10))
u = 2^-24 / 2^-8 / 2^-11 for fp32 / bf16 / fp16 (the unit roundoff of the one output rounding; plus 2^-25, half the spacing of fp16's
subnormals, in fp16), 4 units of 2^-24 on the sum of the absolute terms for the product and the three fmas (Higham's gamma_4), and the normal's own limit below.  The norm-wise check is the 2-norm of
the same expression.  No case runs on a raised bound.

The normal.  |kernel - float64 map| <= NORMAL_K 2^-24 max(|xi|, 2^-10).  The issue leaves K to a measurement: twice the worst ratio the
sweep and the distribution draws show on the GPU, rounded up.
"""
import itertools

import numpy as np

from bwd_fuzz_cases import round_to  # noqa: F401  (re-exported)

ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_STRIDE, ERR_UNSUPPORTED = -1, -2, -3, -4, -6          # include/zigma_hip.h
ROW_ABSOLUTE = 1
NORMAL_FLOOR = 2.0 ** -10
# measured on an MI355X: worst |kernel - float64| / (2^-24 max(|xi|, 2^-10)) over the sweep and over the 2^20-normal draws of the distribution tests
NORMAL_WORST_MEASURED = 4.09          # (the sweep's 27 cases stay below 3.1; the 4 x 2^20 normals of the distribution test reach 4.09)
NORMAL_K = 9.0                        # twice that, rounded up.  Above 8: see DESIGN.md 3.6 for which of logf, sqrtf, sincospif costs what
U_OUT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}          # the unit roundoff: 24, 8 and 11 significant bits

KNOWN_ANSWERS = (          # (counter, key) -> output: the Random123 known-answer vectors of philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ---------------------------------------------------------------------------------------------------
# the generator and the map
# ---------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: (..., 4) and key: (..., 2) or (2,) unsigned 32-bit values -> (..., 4) uint32"""
    m32 = np.uint64(0xffffffff)
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & m32 for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & m32 for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def field_words(seed, stream, step, elem_offset, n):
    """the raw words of the quads that elements [elem_offset, elem_offset + n) touch: (ceil(n / 4), 4) uint32"""
    assert elem_offset % 4 == 0
    q = elem_offset // 4 + np.arange(-(-n // 4), dtype=np.uint64)
    ctr = np.stack([q & np.uint64(0xffffffff), q >> np.uint64(32), np.full_like(q, step), np.full_like(q, stream)], -1)
    return philox4x32_10(ctr, (seed & 0xffffffff, seed >> 32))


def _u_x(words):
    w = np.asarray(words, np.uint32).reshape(-1, 2, 2)                           # (quad, pair, (ra, rb))
    return ((w[..., 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24, (w[..., 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -23


def normals_f64(words):
    """(quads, 4) words -> (4 quads,) normals: the header's map in float64"""
    u, x = _u_x(words)
    rho = np.sqrt(-2.0 * np.log(u))
    return np.stack([rho * np.cos(np.pi * x), rho * np.sin(np.pi * x)], -1).reshape(-1)


def normals_f32(words):
    """the same map step by step in float32: u and x are exact, logf, sqrtf, sincospif and the product round once each"""
    f = np.float32
    u, x = _u_x(words)
    rho = np.sqrt(f(-2.0) * np.log(u.astype(f)))
    k, s = np.cos(np.pi * x).astype(f), np.sin(np.pi * x).astype(f)
    return np.stack([rho * k, rho * s], -1).astype(f).reshape(-1)


def normal_ratio(got, ref):
    """worst |got - ref| / (2^-24 max(|ref|, 2^-10))"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (2.0 ** -24 * np.maximum(np.abs(ref), NORMAL_FLOOR)))) if ref.size else 0.0


def field(seed, stream, step, elem_offset, n):
    """-> (words (ceil(n / 4), 4), the n float64 normals of elements [elem_offset, elem_offset + n))"""
    w = field_words(seed, stream, step, elem_offset, n)
    return w, normals_f64(w)[:n]


def launch_f64(coef_row, a, b, c, xi):
    """one launch in float64 -> (out, sum of the absolute terms); an operand that is None is absent, xi None: no noise"""
    out, mag = 0.0, 0.0
    for k, v in zip(coef_row, (a, b, c, xi)):
        if v is not None:
            term = np.float64(k) * np.asarray(v, np.float64)
            out, mag = out + term, mag + np.abs(term)
    return out, mag


def out_allowance(kind, ref, mag, cn, xi):
    """the per-element limit of the module docstring"""
    noise = 0.0 if xi is None else NORMAL_K * abs(float(cn)) * np.maximum(np.abs(xi), NORMAL_FLOOR)
    return U_OUT[kind] * np.abs(ref) + (2.0 ** -25 if kind == "f16" else 0.0) + 2.0 ** -24 * (4.0 * mag + noise)


# ---------------------------------------------------------------------------------------------------
# the sweep's table
# ---------------------------------------------------------------------------------------------------
SDE_N = (1, 3, 4, 5, 255, 256, 1023, 1025, 4 * 256 * 2 + 3)          # 2051: the second workgroup (256 lanes x 8 elements each)
SDE_KINDS = ("f32", "bf16", "f16")
SDE_SUBSETS = tuple(itertools.product((False, True), repeat=3))      # which of a, b, c are present
SDE_OFFSETS = (0, 2 ** 34 - 4, 4 * (2 ** 40 + 12345))                # 2^34 - 4: quad 2^32 - 1, then the carry into the counter's high word
SDE_STEPS = (0, 1, 2 ** 31 - 1)
SDE_STREAMS = (0, 7, 2 ** 32 - 1)
SDE_ROWS_PER_STEP = (1, 3)
SDE_COEF_ROWS = 8
SDE_SEEDS = (0, 1, 0x0123456789abcdef, 2 ** 64 - 1)


def sde_cases():
    """Keys: n, kind, present (a, b, c), alias (out is a), cn0 (the row's cn is 0), state (False: NULL, cn0 absolute rows only), offset, step, stream,
    seed, absolute, rps, row, table_row (the row of the table the call must read: a relative row past the table is the last row), data seed."""
    out = []
    for di, kind in enumerate(SDE_KINDS):
        for j, n in enumerate(SDE_N):
            i = di * len(SDE_N) + j
            present = SDE_SUBSETS[(j + 3 * di) % 8]
            step = SDE_STEPS[(j + di) % 3]
            absolute = (j + di) % 2 == 1
            rps = SDE_ROWS_PER_STEP[(j // 2 + di) % 2]
            row = (j + di) % rps if not absolute else (3 * j + di) % SDE_COEF_ROWS
            cn0 = j % 4 == 3
            c = dict(n=n, kind=kind, present=present, alias=present[0] and (j + di) % 3 != 0, cn0=cn0, state=not (cn0 and absolute and j % 8 == 3),
                     offset=SDE_OFFSETS[(j // 3 + di) % 3], step=step, stream=SDE_STREAMS[(j + 2 * di) % 3], seed=SDE_SEEDS[i % 4], absolute=absolute, rps=rps,
                     row=row, table_row=row if absolute else min(step * rps + row, SDE_COEF_ROWS - 1), data_seed=31000 + i)
            c["id"] = (f"n{n}-{kind}-{''.join(ch for ch, on in zip('abc', present) if on) or 'none'}{'-inplace' if c['alias'] else ''}{'-cn0' if cn0 else ''}"
                       f"{'' if c['state'] else '-nostate'}-o{SDE_OFFSETS.index(c['offset'])}-s{SDE_STEPS.index(step)}-w{SDE_STREAMS.index(c['stream'])}"
                       f"-{'abs' if absolute else 'rel%d' % rps}{row}")
            out.append(c)
    return out


def sde_inputs(c):
    """-> dict(a, b, c: n values already rounded to the case's type, or None; coef: (SDE_COEF_ROWS, 4) float32, rows other than the one the call
    reads are NaN, the coefficients of absent operands are NaN too)"""
    rng = np.random.default_rng(c["data_seed"])
    ops = [round_to(rng.standard_normal(c["n"], dtype=np.float32) * np.float32(1.5), c["kind"]) if on else None for on in c["present"]]
    coef = np.full((SDE_COEF_ROWS, 4), np.nan, np.float32)
    row = rng.uniform(0.25, 1.5, 4).astype(np.float32) * np.where(rng.random(4) < 0.4, -1, 1).astype(np.float32)
    row[3] = 0.0 if c["cn0"] else row[3]
    row[:3] = np.where(c["present"], row[:3], np.nan)
    coef[c["table_row"]] = row
    return dict(a=ops[0], b=ops[1], c=ops[2], coef=coef)


def sde_reference(c, inp):
    """-> dict(words: (ceil(n / 4), 4) uint32 or None where no Philox work is done, xi, out, mag, allow)"""
    row = inp["coef"][c["table_row"]].astype(np.float64)
    words, xi = (None, None) if c["cn0"] else field(c["seed"], c["stream"], c["step"], c["offset"], c["n"])
    out, mag = launch_f64(row, inp["a"], inp["b"], inp["c"], xi)
    out, mag = np.broadcast_to(out, (c["n"],)).astype(np.float64), np.broadcast_to(mag, (c["n"],)).astype(np.float64)
    return dict(words=words, xi=xi, out=out, mag=mag, allow=out_allowance(c["kind"], out, mag, row[3], xi))


# (what is wrong, status): the GPU test builds each from a small valid call; include/zigma_hip.h lists them in the order they are checked
REFUSALS = (("null-block", ERR_NULL), ("n-negative", ERR_SHAPE), ("offset-negative", ERR_SHAPE), ("offset-not-quad", ERR_SHAPE), ("rows_per_step0", ERR_SHAPE),
            ("row-negative", ERR_SHAPE), ("coef_rows0", ERR_SHAPE), ("absolute-row-past-table", ERR_SHAPE), ("flags2", ERR_UNSUPPORTED), ("dtype3", ERR_DTYPE),
            ("null-out", ERR_NULL), ("null-coef", ERR_NULL), ("null-state-relative", ERR_NULL), ("null-state-bits", ERR_NULL), ("a-off-by-one", ERR_STRIDE),
            ("c-off-by-one", ERR_STRIDE), ("out-off-by-one", ERR_STRIDE), ("coef-off-by-one", ERR_STRIDE), ("state-off-by-one", ERR_STRIDE),
            ("bits-off-by-one", ERR_STRIDE))

# the distribution tests: N normals per draw at these coordinates (seed, stream, step)
DIST_N = 2 ** 20
DIST_SEED, DIST_STREAM, DIST_STEP = 0x243f6a8885a308d3, 0, 5
P_BEYOND_3 = 2.6998e-3


def distribution_checks(z, others):
    """z: the N normals at (DIST_SEED, DIST_STREAM, DIST_STEP); others: {name: N normals at a neighbouring coordinate}.  -> list of
    (name, value, bound): five standard errors of each estimator under the null hypothesis (derived, not tuned)."""
    z = np.asarray(z, np.float64)
    N = z.size
    var = float(np.mean(z * z) - np.mean(z) ** 2)
    beyond = float(np.sum(np.abs(z) > 3.0))
    out = [("mean", abs(float(np.mean(z))), 5 / np.sqrt(N)), ("variance", abs(var - 1.0), 5 * np.sqrt(2 / N)),
           ("excess kurtosis", abs(float(np.mean((z - np.mean(z)) ** 4)) / var ** 2 - 3.0), 5 * np.sqrt(24 / N)),
           ("beyond 3 sigma", abs(beyond - N * P_BEYOND_3), 5 * np.sqrt(N * P_BEYOND_3 * (1 - P_BEYOND_3)))]
    pairs = dict(others)
    pairs["even / odd normals of a quad"] = None
    for name, o in pairs.items():
        a, b = (z[0::2], z[1::2]) if o is None else (z, np.asarray(o, np.float64))
        out.append((f"correlation with {name}", abs(float(np.corrcoef(a, b)[0, 1])), 5 / np.sqrt(a.size)))
    return out
