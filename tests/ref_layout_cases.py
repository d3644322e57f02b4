"""Case tables of the sweep of the kernels behind the drop-in call surface: scan_generic_kernel (zigma_selective_scan_fwd as selective_scan_fn,
selective_scan_cuda_fwd and scan_raw reach it) and conv_tok_kernel / conv_generic_kernel (zigma_causal_conv1d_fwd through causal_conv1d_raw and
causal_conv1d_fn).

Plain numpy, importable without a GPU.  scan_generic_cases() / conv_cases() yield dicts of PARAMETERS with stable ids; *_inputs(case) makes the
numbers from the case's seed, already rounded to the operand's type, in the LOGICAL layout of the call surface — (batch, dim, seqlen)
activations, (batch, groups, dstate, seqlen) or constant (dim, dstate) B / C —; how they lie in memory (contiguous, token-major views, padded
pitches, slices of NaN-filled buffers) is the GPU test's to build from the case's layout keys.  *_reference(case, inputs, dt=np.float64)
evaluates everything through oracle.zigma_oracle (selective_scan / causal_conv1d with dt=), the carries chunk by chunk: the decay product of
a carry is prod exp(delta A) from the start of the sequence to the chunk's end, its state h at the chunk's end.
tests/test_ref_layout_cases_cpu.py checks coverage, the references against an independent float64 restatement and the rounding model;
tests/test_gpu_ref_layout.py runs the kernels.

Limits (as in fwd_fuzz_cases).  Every comparison is with the UNROUNDED float64 reference on the same rounded operands.  Norm-wise: IO_BOUND
of the I/O type for out / out_z / the conv output (one rounding of a W-term fp32 sum: the bound of conv_x_proj's u), STATE_BOUND for the two
outputs of a carry, decays (x_prod) and states (x_state).  Row-wise: rowwise_worst <= ROW_GUARD over every (sample, channel) row and every
(sample, position) row of out / out_z, every (sample, position) row of the conv output, every (sample, channel, chunk) row of the carries.
A case whose fp32 numpy model — the same recurrence step by step in fp32 on the same operands, the decay product taken as exp2 of the fp32
running sum of delta times fl32(A log2 e), results rounded to the I/O type — needs more than half a limit carries max(base, 2 x d_model) in
RAISED below (written by `python tests/test_ref_layout_cases_cpu.py`, never from a kernel's output): at most one case in five, never above
8 x the base, only in the `long` and `edges` regimes (RAISED_* below; the CPU test holds the table to them).
"""
import numpy as np

import fwd_fuzz_cases as fc
from fwd_fuzz_cases import IO_BOUND, REGIMES, ROW_GUARD, STATE_BOUND, norm_err, round_to, rowwise_worst  # noqa: F401  (re-exported)
from oracle import zigma_oracle as zo

KINDS = ("f32", "bf16", "f16")
DSTATES = (1, 2, 3, 4, 5, 8, 11, 16, 17, 32, 33, 64, 65, 100, 128, 129, 200, 256)
INSTANTIATIONS = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))     # (lanes per row, states per lane)
SHORT_L, CHUNK_L, CHUNKS, LONG_L = (1, 2, 17, 100, 257), (48, 64, 100, 112), (16, 32, 48), (2048, 2049, 4097)
BC_FORMS = (("var", "var"), ("const", "var"), ("var", "const"), ("const", "const"))
RAISED_SHARE, RAISED_FACTOR, RAISED_REGIMES = 0.2, 8.0, ("long", "edges")
_K = np.float32(1.4426950408889634)

# raised bounds, id -> {output: bound}: max(base, 2 x d_model), d_model measured on the CPU (tests/test_ref_layout_cases_cpu.py writes this table)
RAISED = {}


# cases whose few output elements (one position, one channel row, or a handful of large gated elements that carry the norm), drawn from the
# first seed, leave the float64 reference ITSELF more than 0.9 of the norm-wise bound once it is rounded (one bf16 / fp16 rounding costs up
# to 2^-8 / 2^-11 of an element; the bound is made for rows of many): drawn again, id -> draws skipped.  The CPU test holds every case to 0.9.
RESEED = {
    "dstate-bf16+f32bc-n100-b1-d3-L1-benign-sv-vvg14d_pad-ref-fn": 1,
    "tokview-f16-n16-b2-d136-L1-edges-zbtv-vvg1cols-tok-raw": 1,
    "dstate-bf16+f32bc-n2-b1-d1-L2-long-bsv-cvg14d_pad-ref-fn": 1,
    "dstate-bf16+f32bc-n4-b1-d1-L100-edges-zDbovT-ccg13d-ref-cuda_fwd": 1,
    "dstate-bf16+f32bc-n2-b1-d15-L17-edges-zb-ccg14d_pad-ref-fn": 1,
    "dstate-f16-n1-b1-d1-L1-benign-zDbsovT-vvg14d_pad-ref-raw": 3,
    "dstate-f16+f32bc-n32-b1-d1-L1-edges-DbsT-ccg13d-ref-cuda_fwd": 1,
}


def instantiation(N):
    """(lanes per row, states per lane) of the scan_generic_kernel instantiation that serves dstate N, restated from launch_generic
    (csrc/selective_scan.hip); the CPU test checks it against the launcher's rule, the smallest i with 1 << i >= dstate"""
    for limit, inst in zip((1, 2, 4, 8, 16, 32, 64, 128, 256), INSTANTIATIONS):
        if N <= limit:
            return inst
    raise ValueError(N)


def turned_away(c):
    """why plan_scan's token-major kernels do not take the case (tok_layout_ok of csrc/scan_plan.h restated); empty: they would"""
    why = []
    if c["bform"] != "var" or c["cform"] != "var":
        why.append("constant B / C")
    if c["G"] != 1:
        why.append("groups")
    if c["bck"] != c["kind"]:
        why.append("bc_dtype")
    if c["dim"] % 64:
        why.append("dim % 64")
    if c["N"] not in (8, 16):
        why.append("dstate")
    if c["layout"] == "ref" and c["L"] > 1:
        why.append("channel stride")
    return why


def _scan_case(table, sec, **kw):
    c = dict(sec=sec, kind="bf16", bck=None, N=16, B=1, dim=3, L=17, layout="ref", olayout=None, bform="var", cform="var", G=1, bc_layout="4d_pad",
             const_t=False, z=True, D=True, bias=True, softplus=True, both=False, tables=False, views=True, chunk=0, api="raw", regime="benign")
    c.update(kw)
    c["bck"] = c["bck"] or c["kind"]
    if c["api"] != "raw":           # the drop-in entry points allocate their outputs, take no row tables and no chunk length
        c.update(tables=False, olayout=None, chunk=0, both=c["api"] == "cuda_fwd")
    if c["bform"] == "const" and c["cform"] == "const":
        c["G"] = 1
    if c["G"] != 1 and c["bc_layout"] == "3d":
        c["bc_layout"] = "4d_pad"
    if not c["z"]:
        c["both"] = False
    c["olayout"] = c["olayout"] or c["layout"]
    c["carries"] = bool(c["chunk"]) or c["api"] in ("cuda_fwd", "fn_last")
    opts = "".join(ch for ch, on in (("z", c["z"]), ("D", c["D"]), ("b", c["bias"]), ("s", c["softplus"]), ("o", c["both"]), ("t", c["tables"]),
                                     ("v", c["views"]), ("T", c["const_t"])) if on)
    c["id"] = (f"{sec}-{c['kind']}{'' if c['bck'] == c['kind'] else '+f32bc'}-n{c['N']}-b{c['B']}-d{c['dim']}-L{c['L']}-{c['regime']}-{opts}-"
               f"{c['bform'][0]}{c['cform'][0]}g{c['G']}{c['bc_layout']}-{c['layout']}{'' if c['olayout'] == c['layout'] else '>' + c['olayout']}-{c['api']}"
               + (f"-c{c['chunk']}" if c["chunk"] else ""))
    c["seed"] = 21000 + len(table) + 1000 * RESEED.get(c["id"], 0)
    c["kernel_name"], c["inst"] = "scan_generic", instantiation(c["N"])
    assert turned_away(c), c["id"]
    table.append(c)
    return c


# (batch, dim, groups where B / C vary) with batch * dim no multiple of any rows-per-wave count: odd, above one
ODD_ROWS = ((1, 3, 1), (5, 3, 3), (3, 5, 5), (1, 15, 3), (3, 3, 1), (1, 9, 3))
# ... and with 2 groups: 18 rows, no multiple of 64, 32, 16, 8 or 4 (the instantiations of up to 16 lanes per row)
EVEN_ROWS = ((3, 6, 2), (3, 6, 3), (3, 6, 6), (3, 6, 1))
TOK_VIEWS = ((96, 16, False, 1), (136, 16, False, 1), (64, 16, True, 1), (128, 8, True, 1), (128, 16, False, 2), (64, 8, False, 2))   # (dim, N, fp32 B / C, groups)


def scan_generic_cases():
    """scan_generic_kernel.  Keys: sec (dstate | tokview | chunks | long), kind (I/O type), bck (type of variable B / C), N, B, dim, L, layout /
    olayout (of u, delta, z / of out, out_z: `ref` contiguous (B, D, L), `tok` token-major views), bform / cform (var | const), G (groups),
    bc_layout (3d: (B, N, L) through the entry point's own unsqueeze; 4d_pad: (B, G, N, L) views of padded pitch; cols: columns of token-major
    rows), const_t (constant B / C are transposed views), z / D / bias / softplus, both (z: out as well as out_z), tables (z_row_index /
    out_row_index, two different permutations), views (operands and outputs are slices of NaN-filled buffers), chunk (chunk_len through
    scan_raw(x=...); 0: 2048), api (raw | fn | fn_last | cuda_fwd), carries (the carry tensor is checked), regime, inst, kernel_name, seed."""
    out = []
    for kind in KINDS:
        i = 0
        for N in DSTATES + (1, 2):          # every instantiation twice: at its power of two on ONE row, below the next one on an odd number of rows
            lanes = instantiation(N)[0]
            one_row = N & (N - 1) == 0 and not (N <= 2 and i >= len(DSTATES))
            bform, cform = BC_FORMS[(i + i // 4) % 4]
            if one_row:
                Bsz, dim, G = 1, 1, 1
            else:
                geo = ODD_ROWS if lanes >= 32 or i % 2 else EVEN_ROWS
                Bsz, dim, G = geo[(i // 2) % len(geo)]
            bias, softplus = ((True, True), (True, False), (False, True), (False, False))[(i // 2) % 4]
            api = ("raw", "fn", "raw", "cuda_fwd", "raw", "fn_last")[i % 6]
            _scan_case(out, "dstate", kind=kind, bck="f32" if kind != "f32" and i % 2 else kind, N=N, B=Bsz, dim=dim, G=G, L=SHORT_L[(i + i // 5) % 5],
                       bform=bform, cform=cform, bc_layout=("4d_pad", "3d")[(i // 3) % 2], const_t=i % 3 == 0, z=i % 4 != 1, D=i % 3 != 1, bias=bias,
                       softplus=softplus, both=i % 8 == 0, tables=i % 4 == 2, views=i % 5 != 4, olayout="tok" if i % 10 == 4 else None, api=api,
                       regime=REGIMES[(i + i // 4) % 4])
            i += 1
        j = 0
        for dim, N, f32bc, G in TOK_VIEWS:   # token-major views the token-major plan turns away, with and without the two row tables
            if f32bc and kind == "f32":
                dim, f32bc = dim + 32, False
            for tables in (False, True):
                _scan_case(out, "tokview", kind=kind, bck="f32" if f32bc else kind, N=N, B=1 + j % 2, dim=dim, G=G, L=SHORT_L[(j + 2) % 5], layout="tok",
                           bc_layout=("cols", "4d_pad")[j % 3 == 2], z=tables or j % 4 != 0, D=j % 3 != 0, bias=j % 5 != 1, softplus=j % 4 != 3,
                           both=j % 4 == 1, tables=tables, views=j % 3 != 1, olayout="ref" if j % 6 == 5 else None, regime=REGIMES[j % 4])
                j += 1
        for j, (L, chunk) in enumerate((L, ch) for L in CHUNK_L for ch in CHUNKS):      # 1 ... 7 chunks (48 steps in chunks of 48: one), ragged and whole last chunks
            Bsz, dim, G = (ODD_ROWS + EVEN_ROWS)[j % 10] if j % 4 else (1, 96, 1)
            N = (3, 16, 33, 8, 100, 5, 17, 2, 65, 11, 4, 129)[j]
            bform, cform = BC_FORMS[j % 4] if j % 4 else ("var", "var")
            _scan_case(out, "chunks", kind=kind, bck="f32" if kind != "f32" and j % 3 == 1 else kind, N=N, B=Bsz, dim=dim, G=G, L=L, chunk=chunk,
                       layout="ref" if j % 4 else "tok", bform=bform, cform=cform, bc_layout="cols" if j % 4 == 0 else "4d_pad", z=j % 3 != 2, D=j % 2 == 0,
                       bias=j % 4 != 2, softplus=j % 5 != 3, both=j % 6 == 0, tables=j % 4 == 3, views=j % 3 != 0, regime=REGIMES[(j + 1) % 4])
        k0 = KINDS.index(kind)
        for j, L in enumerate(LONG_L):      # the reference's own chunk length: one, two and three chunks; the carry at an exact chunk end is the last state
            Bsz, dim = ((2, 4), (1, 5), (1, 8))[(j + k0) % 3]
            _scan_case(out, "long", kind=kind, bck="f32" if kind != "f32" and j == 1 else kind, N=(16, 5, 8)[(j + k0) % 3], B=Bsz, dim=dim, L=L,
                       api=("cuda_fwd", "fn_last")[(j + k0) % 2], bc_layout=("3d", "4d_pad")[j % 2], z=j != 1, views=j != 2,
                       regime="long")         # (small steps: after thousands of them the decay product of a carry is still an fp32 number)
    return out


def _tables(rng, L, period=0):
    return fc._tables(rng, L, period or L)


def scan_inputs(c):
    """logical numpy operands of a scan case, rounded to their types: u, delta, z (B, dim, L); A (dim, N) f32; Bm / Cm (B, G, N, L) in the B / C type
    or constant (dim, N) f32; D, bias (dim,) f32 | None; zi, oi int32 (L,) | None"""
    kind, bck, Bsz, dim, L, N, G, reg = c["kind"], c["bck"], c["B"], c["dim"], c["L"], c["N"], c["G"], c["regime"]
    rng = np.random.default_rng(c["seed"])
    rn = lambda *s: rng.standard_normal(s)
    edges = reg == "edges"
    u, z = rn(Bsz, dim, L), rn(Bsz, dim, L)
    if reg == "benign":
        A = -(0.5 * rng.random((dim, N)) + 1e-3)
    elif reg == "long":
        A = -(0.05 + 0.95 * rng.random((dim, N)))
    else:
        A = -np.arange(1, N + 1)[None] * np.exp(0.2 * rn(dim, N))
    if c["bias"]:
        bias = {"benign": 0.5 * rng.random(dim), "long": 0.1 * rn(dim), "edges": np.clip(0.1 * rn(dim), -0.2, 0.2)}.get(reg, rn(dim) - 3.0)
        if not c["softplus"]:
            bias = (0.5 if reg == "benign" else 0.005) * rng.random(dim)
    else:
        bias = np.zeros(dim)
    b3 = bias[None, :, None]
    if c["softplus"]:
        if reg == "benign":
            delta = rng.random((Bsz, dim, L)) - 0.3
        elif reg == "long":
            delta = np.log(np.expm1(rng.uniform(0.005, 0.05, (Bsz, dim, L)))) - b3
        else:
            delta = rn(Bsz, dim, L) - (3.0 if edges or not c["bias"] else 0.0)
    else:           # no softplus: the step itself, positive
        if reg == "benign":
            delta = 0.5 * rng.random((Bsz, dim, L))
        elif reg == "long":
            delta = rng.uniform(0.005, 0.05, (Bsz, dim, L))
        else:
            delta = zo.softplus(rn(Bsz, dim, L) + rn(dim)[None, :, None] - 3.0)
    scale = N ** -0.5 if N > 16 else 1.0            # y sums over dstate products: the outputs keep the size of u
    mk = lambda form: 0.5 * rn(dim, N) if form == "const" else rn(Bsz, G, N, L) * (0.5 if edges else 1.0) * scale
    Bm, Cm = mk(c["bform"]), mk(c["cform"])
    if edges:
        n = Bsz * dim * L
        k = max(1, n // 12)
        at = rng.permutation(n)
        fl = lambda a: a.reshape(-1)
        # delta + bias on both sides of the softplus threshold of 20 (those inputs scaled down: the outputs stay of the size of the others), far below
        # zero (log1p(exp(x)) = exp(x) to fp32), around the kernel's series / log switch; without softplus the same large steps
        # (the steps of ~20 about once per channel row and band, and a first state that decays slowly: a carry's decay product, exp(A sum(step)), stays
        # an fp32 number in at least one state of every row)
        A[:, 0] = -0.25
        for band, (lo, hi) in enumerate(((19.75, 19.75), (20.25, 20.25), (-18.0, -18.0), (-6.0, -3.0))):
            idx = at[band * k:band * k + (min(k, Bsz * dim) if band < 2 else k)]
            if c["softplus"]:
                fl(delta)[idx] = rng.uniform(lo, hi, idx.size)
            elif band < 2:
                fl(delta)[idx] = lo
            if band < 2:
                fl(u)[idx] *= 0.05
        for band, v in enumerate((12.0, -12.0, 30.0, -30.0)):      # strongly negative and positive gate pre-activations
            fl(z)[at[::-1][band * k:(band + 1) * k]] = v
        if Bsz * dim > 1:
            u[0, dim - 1] = 0.0                      # a channel whose input is zero throughout
        if kind == "f16" and L > 2:                 # subnormal operands (below 6.1e-5)
            u[-1, 0, 1] = 3e-6
    rt, rb = (lambda a: round_to(a, kind)), (lambda a: round_to(a, bck))
    zi, oi = _tables(rng, L) if c["tables"] else (None, None)
    return dict(u=rt(u), delta=rt(delta), z=rt(z) if c["z"] else None, A=A.astype(np.float32),
                Bm=Bm.astype(np.float32) if c["bform"] == "const" else rb(Bm), Cm=Cm.astype(np.float32) if c["cform"] == "const" else rb(Cm),
                D=(1 + 0.2 * rn(dim)).astype(np.float32) if c["D"] else None, bias=bias.astype(np.float32) if c["bias"] else None, zi=zi, oi=oi)


def pre_softplus(c, inp, dt=np.float64):
    pre = inp["delta"].astype(dt)
    return pre if inp["bias"] is None else pre + inp["bias"].astype(dt)[None, :, None]


def step_sizes(c, inp, dt=np.float64):
    pre = pre_softplus(c, inp, dt)
    return zo.softplus(pre) if c["softplus"] else pre


def chunk_len(c):
    return c["chunk"] or 2048


def scan_reference(c, inp, dt=np.float64):
    """-> dict: out (B, dim, L) the ungated y where the call writes it, out_z where there is a gate, x_prod / x_state (B, dim, chunk, N) where the
    carries are checked — all as the call lays them out logically (results at row oi[l], the gate read at row zi[l]).  dt=np.float32: the
    rounding model (module docstring)."""
    L, N = c["L"], c["N"]
    args = (inp["A"], inp["Bm"], inp["Cm"], inp["D"], None, inp["bias"], c["softplus"])
    y = zo.selective_scan(inp["u"], inp["delta"], *args, dt=dt)
    ref = {}
    place = lambda a: a if inp["oi"] is None else _scatter(a, inp["oi"])
    if c["z"]:
        zs = inp["z"].astype(dt) if inp["zi"] is None else inp["z"].astype(dt)[:, :, inp["zi"]]
        ref["out_z"] = place(y * zo.silu(zs))
    if not c["z"] or c["both"]:
        ref["out"] = place(y)
    if c["carries"]:
        ch = chunk_len(c)
        n_chunks = -(-L // ch)
        step, A = step_sizes(c, inp, dt), inp["A"].astype(dt)
        ref["x_prod"], ref["x_state"] = (np.zeros((c["B"], c["dim"], n_chunks, N), dt) for _ in range(2))
        H, cum = np.zeros((c["B"], c["dim"], N), dt), np.zeros((c["B"], c["dim"]), dt)
        A2 = (inp["A"] * _K).astype(np.float32)
        for k in range(n_chunks):
            s = slice(k * ch, min((k + 1) * ch, L))
            bc = lambda M: M if M.ndim == 2 else M[..., s]
            if dt is np.float64:        # chunk by chunk: h_end = exp(A sum(step)) h_start + h_end(from 0)
                _, hl = zo.selective_scan(inp["u"][..., s], inp["delta"][..., s], inp["A"], bc(inp["Bm"]), bc(inp["Cm"]), None, None, inp["bias"],
                                          c["softplus"], return_last_state=True, dt=dt)
                st = step[..., s].sum(-1, dtype=dt)
                H = np.exp(st[..., None] * A[None]) * H + hl
                cum = cum + st
                ref["x_prod"][:, :, k] = np.exp(cum[..., None] * A[None])
            else:                       # the model: the recurrence itself in fp32 up to the chunk's end, exp2 of the fp32 running sum
                e = slice(0, s.stop)
                be = lambda M: M if M.ndim == 2 else M[..., e]
                _, H = zo.selective_scan(inp["u"][..., e], inp["delta"][..., e], inp["A"], be(inp["Bm"]), be(inp["Cm"]), None, None, inp["bias"],
                                         c["softplus"], return_last_state=True, dt=dt)
                for l in range(s.start, s.stop):
                    cum = (cum + step[..., l]).astype(np.float32)
                ref["x_prod"][:, :, k] = np.exp2((cum[..., None] * A2[None]).astype(np.float32))
            ref["x_state"][:, :, k] = H
    return ref


def _scatter(a, rows):
    full = np.empty_like(a)
    full[:, :, rows] = a
    return full


STATE_KEYS = ("x_prod", "x_state")


def base_bound(c, key):
    return STATE_BOUND if key in STATE_KEYS else IO_BOUND[c["kind"]]


def bound_of(c, key):
    return max(base_bound(c, key), RAISED.get(c["id"], {}).get(key, 0.0))


def out_kind(c, key):
    return "f32" if key in STATE_KEYS else c["kind"]


def row_views(key, a):
    """the row families an output is checked over, each with the row on the last axis"""
    a = np.asarray(a, np.float64)
    return (a, a.transpose(0, 2, 1)) if key in ("out", "out_z") else (a.transpose(0, 2, 1),) if key == "conv" else (a,)


def row_ratio(key, got, ref, bound):
    return max(rowwise_worst(g, r, bound) for g, r in zip(row_views(key, got), row_views(key, ref)))


def need(key, got, ref):
    """the smallest bound `got` passes with, norm-wise and over every row family"""
    return max(norm_err(got, ref), row_ratio(key, got, ref, 1.0) / ROW_GUARD)


def model_excess(key, model, ref, kind):
    """fc.model_excess over this sweep's row families -> (excess, d_model): what decides whether a case is raised (the fp32 model before the output
    rounding norm-wise, the rounded model row by row in units of the guard), and the smallest bound the rounded model passes with"""
    rounded = round_to(model, kind)
    return max(norm_err(model, ref), row_ratio(key, rounded, ref, 1.0) / ROW_GUARD), need(key, rounded, ref)


# ---------------------------------------------------------------------------------------------------
# the stand-alone conv kernels
# ---------------------------------------------------------------------------------------------------
CONV_TOK_DIM, CONV_TOK_L, CONV_RESET = (4, 8, 252, 256, 260, 516), (1, 2, 3, 15, 16, 17, 31, 33, 100), (16, 32, 48)
CONV_LAYOUTS = ("tok", "half", "cf", "cl", "x_off", "out_off", "pitch")


def conv_tok_ok(c):
    """plan_conv1d's token-major test (csrc/front_plan.h) on what a layout means in the GPU test: `tok` rows of 4-aligned pitch on a 16-byte boundary;
    `half` x the first half of (B, L, 2 dim) rows, out of pitch dim + 8; `cf` the reference's contiguous (B, D, L); `cl` channel-last rows of a
    dim that is no multiple of 4; x_off / out_off: that operand starts 2 elements into its allocation; pitch: rows dim + 2 elements apart"""
    return c["layout"] in ("tok", "half") and c["dim"] % 4 == 0


def _conv_case(table, **kw):
    c = dict(kind="bf16", wkind=None, W=4, silu=True, bias=True, B=2, dim=8, L=17, layout="tok", tab=False, reset=0, api="raw", regime="benign")
    c.update(kw)
    c["wkind"] = c["wkind"] or c["kind"]
    if c["api"] == "fn":
        c.update(tab=False, reset=0)
    c["seed"] = 22000 + len(table)
    c["kernel_name"] = "conv_tok" if conv_tok_ok(c) else "conv_generic"
    assert not c["reset"] or (c["kernel_name"] == "conv_tok" and c["L"] % c["reset"] == 0)
    c["id"] = (f"{c['kernel_name']}-{c['kind']}{'' if c['wkind'] == c['kind'] else '+f32w'}-w{c['W']}{'s' if c['silu'] else ''}{'b' if c['bias'] else ''}-b{c['B']}-d{c['dim']}"
               f"-L{c['L']}-{c['layout']}{'-t' if c['tab'] else ''}{'-r%d' % c['reset'] if c['reset'] else ''}-{c['api']}-{c['regime']}")
    table.append(c)
    return c


def conv_cases():
    """conv_tok_kernel and conv_generic_kernel.  Keys: kind, wkind (type of the taps and the bias), W, silu, bias, B, dim, L, layout (conv_tok_ok),
    tab (x_row_index; with reset: a permutation inside every period), reset (reset_period), api (raw: causal_conv1d_raw into an output the
    test lays out | fn: causal_conv1d_fn), regime (benign | edges: SiLU pre-activations at +-12 and +-30), kernel_name, seed."""
    out = []
    for kind in KINDS:
        i = 0
        sw = lambda i: dict(W=(4, 3, 2)[i % 3], silu=i % 4 != 1, bias=i % 5 != 2, wkind="f32" if kind != "f32" and i % 2 else kind,
                            regime=("benign", "edges")[i % 2])
        for L in CONV_TOK_L:                # conv_tok: every dim over every length region (left padding, the tile of 16, a halo across tiles)
            for dim in (CONV_TOK_DIM[i % 6], CONV_TOK_DIM[(i + 3) % 6]):
                _conv_case(out, kind=kind, B=1 + i % 3, dim=dim, L=L, layout=("tok", "half")[i % 3 == 1], tab=i % 3 == 2, api="fn" if i % 7 == 3 else "raw", **sw(i))
                i += 1
        for period in CONV_RESET:           # restarting sequences: 2 ... 4 periods, with and without a row table that permutes inside the periods
            for table in (False, True):
                _conv_case(out, kind=kind, B=1 + i % 2, dim=CONV_TOK_DIM[i % 6], L=period * (2 + i % 3), layout=("tok", "half")[i % 2], tab=table, reset=period, **sw(i))
                i += 1
        # conv_generic: the reference's layout, channel-last with dim % 4 != 0, misaligned slices; B * D * L below and above one workgroup of 256
        for layout, dim, Bsz, L in (("cf", 5, 2, 17), ("cf", 64, 2, 100), ("cf", 3, 1, 1), ("cf", 12, 3, 33), ("cl", 6, 2, 17), ("cl", 70, 2, 31), ("cl", 6, 1, 2),
                                    ("cl", 70, 3, 100), ("x_off", 8, 2, 17), ("x_off", 256, 1, 16), ("out_off", 8, 2, 15), ("out_off", 260, 2, 33),
                                    ("pitch", 4, 1, 3), ("pitch", 252, 2, 17)):
            _conv_case(out, kind=kind, B=Bsz, dim=dim, L=L, layout=layout, tab=i % 2 == 0, api="fn" if layout == "cf" and i % 4 == 1 else "raw", **sw(i))
            i += 1
    return out


def conv_inputs(c):
    """x (B, dim, L) in the I/O type, w (dim, W) and b (dim,) | None in the tap type, rows int32 (L,) | None"""
    rng = np.random.default_rng(c["seed"])
    Bsz, dim, L = c["B"], c["dim"], c["L"]
    x, w, b = rng.standard_normal((Bsz, dim, L)), 0.5 * rng.standard_normal((dim, c["W"])), 0.5 * rng.standard_normal(dim)
    if c["regime"] == "edges" and c["bias"]:
        n = min(4, dim)
        b[:n] = (12.0, -12.0, 30.0, -30.0)[:n]
        x[:, :n] *= 0.05
    rows = _tables(rng, L, c["reset"])[0] if c["tab"] else None
    while rows is not None and L > 1 and np.array_equal(rows, np.arange(L)):       # (a table that gathers nothing checks nothing)
        rows = _tables(rng, L, c["reset"])[0]
    return dict(x=round_to(x, c["kind"]), w=round_to(w, c["wkind"]), b=round_to(b, c["wkind"]) if c["bias"] else None, rows=rows)


def conv_reference(c, inp, dt=np.float64):
    """-> dict(conv=(B, dim, L)): zo.causal_conv1d on the gathered rows, every period on its own"""
    x = inp["x"] if inp["rows"] is None else inp["x"][:, :, inp["rows"]]
    L, period = c["L"], c["reset"] or c["L"]
    y = np.concatenate([zo.causal_conv1d(x[:, :, a:a + period], inp["w"], inp["b"], "silu" if c["silu"] else None, dt=dt) for a in range(0, L, period)], -1)
    return dict(conv=y)
