"""Case tables of the sweep of add-norm forward and the operators around the blocks: zigma_add_norm_fwd (csrc/add_norm.hip),
zigma_patch_embed_fwd, zigma_timestep_embed_fwd, zigma_final_layer_fwd (csrc/embed.hip) and zigma_skinny_linear_fwd (csrc/skinny_linear.hip).

Plain numpy, importable without a GPU.  Seeded generators — norm_cases() / patch_cases() / timestep_cases() / skinny_cases() / final_cases()
and production_cases() — yield dicts of PARAMETERS with stable ids; *_inputs(case) makes the numbers from the case's seed, already rounded to the
case's I/O type; *_reference(case, inputs) evaluates in float64 on those rounded operands (dt=np.float32: the rounding model, the same
formulas step by step in fp32).  Where the ABI defines a 16-bit intermediate — conv + bias -> bf16 before `+ pos`, LayerNorm -> bf16 before the
final projection, SiLU -> bf16, x + gate * branch -> x-type, y -> x-type before the modulation — the reference rounds at the same point.
tests/test_outer_fwd_cases_cpu.py checks coverage, the references against float64 torch restatements and the rounding model;
tests/test_gpu_outer_fwd.py runs the kernels.

Limits: those of the forward sweep (fwd_fuzz_cases: IO_BOUND norm-wise, rowwise_worst <= ROW_GUARD for every output row, DELTA_FLIPS for the
element-wise checks).  No case runs on a raised bound.
"""
import numpy as np

from bwd_fuzz_cases import EPS, NORM_DTYPES, ROW_GUARD, elementwise_worst, round_to, rowwise_worst  # noqa: F401  (re-exported)
from fwd_fuzz_cases import DELTA_FLIPS, DELTA_FLIPS_MODEL, IO_BOUND, flipped_share, model_excess, need, norm_err, row_ratio  # noqa: F401
from oracle import zigma_oracle as zo

ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_STRIDE = -1, -2, -3, -4          # include/zigma_hip.h
REGIMES = ("benign", "model", "edges")
# Outputs of ONE element: a single 16-bit rounding can cost up to 2^-8 / 2^-11 of it, more than the norm-wise bound, which one rounding meets
# only on average over a row.  These two cases drew such a value (the rounded float64 reference itself missed the bound): they run on another seed.
SEED_MOVED = {("norm", "xf16-rf16-wf16-rms-mod-y-1x1-b1-a1-benign"): 24168, ("final", "1x8-o1-b-benign"): 26000}

# ---------------------------------------------------------------------------------------------------
# add_norm forward
# ---------------------------------------------------------------------------------------------------
NORM_COLS = (1, 5, 8, 64, 98, 128, 256, 260, 384, 512, 640, 768, 772, 896, 1000, 1024, 1028, 1032, 2048, 4092, 4096)
NORM_ROWS = (1, 3, 4, 5, 7, 8, 12, 2053)
NORM_FORMS = ("rms", "ln-w", "ln-wb", "ln")           # RMS; LayerNorm with weight only, weight and bias, no weight
# plain | residual_out only (the first block) | residual in and out | branch and gate with / without x_out | shift and scale with / without y_out | the block form
NORM_OPTIONS = ("plain", "first", "res", "gate-xout", "gate", "mod-y", "mod", "full", "full-y")
NORM_ALIGN = (0, 4, 1)                                 # every pointer and every pitch is off by that many elements
NORM_INSTANTIATIONS = tuple((8, i, 16) for i in range(1, 9)) + ((8, 2, 64), (4, 4, 64), (4, 16, 64), (1, 16, 64), (1, 64, 64))
LEAD, TAIL = 8, 8                                      # NaN elements in front of and behind every row


def norm_pitch(c, n=None):
    return LEAD + c["align"] + (c["cols"] if n is None else n) + TAIL


def norm_uses(c):
    o = c["opt"]
    return dict(branch=o in ("gate-xout", "gate", "full", "full-y"), x_out=o in ("gate-xout", "full", "full-y"), res=o in ("res", "full", "full-y"),
                res_out=o in ("first", "res", "full", "full-y"), mod=o in ("mod-y", "mod", "full", "full-y"), y_out=o not in ("mod", "full"))


def norm_branch(c):
    """(VEC, ITERS, LPR) launch_norm (csrc/add_norm.hip) picks for the layout the GPU test builds: every tensor starts LEAD + align elements into
    an allocator-aligned buffer whose rows are norm_pitch() apart; None: refused"""
    cols, a, u = c["cols"], c["align"], norm_uses(c)
    vec = cols % 4 == 0 and a % 4 == 0
    vec8 = vec and cols % 8 == 0 and a % 8 == 0 and c["xk"] != "f32"
    light = not (u["res"] or u["res_out"]) or c["rk"] != "f32"
    if vec8 and light and cols % 128 == 0 and cols <= 1024 and c["rows"] % 4 == 0 and not c["flags"] & 1:
        return (8, cols // 128, 16)
    if vec8 and cols <= 1024:
        return (8, 2, 64)
    if vec and cols <= 1024:
        return (4, 4, 64)
    if vec and cols <= 4096:
        return (4, 16, 64)
    return (1, 16, 64) if cols <= 1024 else (1, 64, 64) if cols <= 4096 else None


def norm_kernel_name(c):
    b = norm_branch(c)
    return "add_norm_v8x4" if b[2] == 16 else "add_norm_v4" if c["cols"] % 4 == 0 and c["align"] % 4 == 0 else "add_norm_v1"


def _norm_case(table, **kw):
    c = dict(kernel="norm", flags=0, align=0, regime="benign", rpb=0, seed=21000 + len(table))
    c.update(kw)
    c["rpb"] = c["rpb"] or c["rows"]
    w = {"rms": c["wk"], "ln-w": c["wk"], "ln-wb": c["wk"], "ln": None}[c["form"]]
    c["id"] = (f"x{c['xk']}-r{c['rk']}-w{w}-{c['form']}-{c['opt']}-{c['rows']}x{c['cols']}-b{c['rpb']}-a{c['align']}-{c['regime']}"
               + ("-f1" if c["flags"] else ""))
    c["branch"], c["kernel_name"] = norm_branch(c), norm_kernel_name(c)
    c["seed"] = SEED_MOVED.get(("norm", c["id"]), c["seed"])
    table.append(c)
    return c


def norm_cases():
    """Keys: xk / rk / wk (types of x, of the residual stream, of weight and bias; gate / shift / scale have x's), form (NORM_FORMS), opt
    (NORM_OPTIONS), rows, cols, rpb (rows_per_batch), align, flags, regime, branch (the instantiation the launch must pick), kernel_name, seed."""
    out = []
    i = 0
    for li, (xk, rk, wk) in enumerate(NORM_DTYPES):          # every layout x every column count
        for ci, cols in enumerate(NORM_COLS):
            rows = NORM_ROWS[(i + li) % 8]
            if rows * cols > 1_200_000:
                rows = (5, 7, 12)[i % 3]
            _norm_case(out, xk=xk, rk=rk, wk=wk, cols=cols, rows=rows, form=NORM_FORMS[(i + ci // 4) % 4], opt=NORM_OPTIONS[(i + li + ci // 9) % 9],
                       rpb=(0, 1, 3, 6)[(i // 2) % 4], align=NORM_ALIGN[(i + i // 3) % 3], regime=REGIMES[(i + i // 7) % 3])
            i += 1
    j = 0
    for xk in ("bf16", "f16"):                              # four rows per wave: 1 ... 8 pieces of 16 bytes per lane
        for it in range(1, 9):
            for rows in (4, 8, 12, 2052):
                opt = NORM_OPTIONS[j % 9]
                _norm_case(out, xk=xk, rk=xk, wk=("f32", xk)[j % 2], cols=128 * it, rows=rows, form=NORM_FORMS[(j + j // 4) % 4], opt=opt,
                           rpb={4: (0, 1), 8: (3, 1), 12: (6, 3), 2052: (1026, 6)}[rows][j % 2], regime=REGIMES[j % 3])
                j += 1
            for align, flags in ((0, 1), (4, 0), (1, 0)):    # the same shapes pinned to one row per wave, and off by 4 and by 1 element
                _norm_case(out, xk=xk, rk=xk, wk=xk, cols=128 * it, rows=12, rpb=6, form=NORM_FORMS[j % 4], opt=NORM_OPTIONS[(j + 3) % 9], align=align,
                           flags=flags, regime=REGIMES[j % 3])
                j += 1
    for xk in ("bf16", "f16"):          # the instantiations the walk above reaches for one type only: <8,2> wide, <4,16> by pitch, <1,64>
        for k, (cols, align, rows) in enumerate(((1000, 0, 5), (1024, 0, 7), (2048, 4, 3), (4096, 0, 5), (1032, 1, 4), (4092, 1, 3), (4096, 1, 8))):
            _norm_case(out, xk=xk, rk=("f32", xk)[k % 2], wk=(xk, "f32")[k % 2], cols=cols, rows=rows, form=NORM_FORMS[k % 4], opt=NORM_OPTIONS[(2 * k + 7) % 9],
                       rpb=(0, 3)[k % 2], align=align, regime=REGIMES[k % 3])
        k = 0
        for form in NORM_FORMS:         # every norm form x every option combination in each 16-bit type: what the walks above left out
            for opt in NORM_OPTIONS:
                if not any(c["xk"] == xk and c["form"] == form and c["opt"] == opt for c in out):
                    _norm_case(out, xk=xk, rk=("f32", xk)[k % 2], wk=(xk, "f32")[k % 2], cols=(640, 260, 98)[k % 3], rows=(7, 8, 5)[k % 3], form=form, opt=opt,
                               rpb=(0, 3)[k % 2], regime=REGIMES[k % 3])
                    k += 1
    return out


def norm_production_cases():
    t = []
    for cols in (640, 768):             # the block form of the shipped models: 2 x 1024 tokens, bf16 x with the fp32 residual stream
        _norm_case(t, xk="bf16", rk="f32", wk="bf16", cols=cols, rows=2048, rpb=1024, form="rms", opt="full", regime="model", seed=26000 + cols)
    return t


def _norm_batch(c):
    return -(-c["rows"] // c["rpb"])


def norm_inputs(c):
    """x, branch (rows, cols) in x's type; residual in rk; weight / bias in wk; mod (batch, 6 cols): shift | scale | gate are the column windows
    MOD_WINDOWS of it, everything else NaN"""
    rng = np.random.default_rng(c["seed"])
    rows, cols, u, reg, nb = c["rows"], c["cols"], norm_uses(c), c["regime"], _norm_batch(c)
    rn = lambda *s: rng.standard_normal(s)
    x, res = rn(rows, cols), rn(rows, cols) * (30.0 if reg == "model" else 1.0)
    if c["form"] != "rms":
        x += 0.3
    br, mod = rn(rows, cols), np.full((nb, 6 * cols), np.nan)
    for k, win in enumerate(MOD_WINDOWS):
        mod[:, win * cols:(win + 1) * cols] = (0.3, 0.3, 0.5)[k] * rn(nb, cols)
    if reg == "edges":
        pick = rng.permutation(rows)
        if c["form"] != "rms" and u["res"] and c["rk"] == "f32" and rows >= 3:
            res[pick[0]] = 100.0 + rn(cols)         # mean 100, spread 1: only a two-pass variance survives it
        if rows >= 2:
            x[pick[1 % rows]] = br[pick[1 % rows]] = res[pick[1 % rows]] = 0.0          # an all-zero row
        if c["form"] == "rms" and rows >= 4:
            x[pick[2]], br[pick[2]], res[pick[2]] = 1e-4 * rn(cols), 0.0, 0.0            # eps decides
        for k, win in enumerate(MOD_WINDOWS[1:]):                                        # scales and gates of +-4
            mod[:, win * cols:win * cols + min(cols, 4)] = np.array([4.0, -4.0, 4.0, -4.0])[:min(cols, 4)]
    w = b = None
    if c["form"] != "ln":
        w = round_to(1.0 + 0.2 * rn(cols), c["wk"])
    if c["form"] == "ln-wb":
        b = round_to(0.2 * rn(cols), c["wk"])
    return dict(x=round_to(x, c["xk"]), branch=round_to(br, c["xk"]) if u["branch"] else None, residual=round_to(res, c["rk"]) if u["res"] else None,
                mod=round_to(mod, c["xk"]) if u["branch"] or u["mod"] else None, weight=w, bias=b)


MOD_WINDOWS = (0, 1, 5)                 # shift, scale, gate: column windows of the (batch, 6 cols) modulation buffer


def mod_window(c, inp, k, dt=np.float64):
    """(rows, cols): window k of the modulation buffer, the sample's row repeated over its rows_per_batch rows"""
    cols, win = c["cols"], MOD_WINDOWS[k]
    return inp["mod"][:, win * cols:(win + 1) * cols].astype(dt).repeat(c["rpb"], axis=0)[:c["rows"]]


def norm_reference(c, inp, dt=np.float64):
    """-> dict of the outputs the case asks for (x_out, residual_out, y_out, y_mod) and `_terms`, the two summands of y_mod.  x_out and
    residual_out are the float64 sums UNROUNDED (norm_exact() gives the one value they must have bit for bit); the statistics run on the
    unrounded x' + residual, x' = x + gate * branch rounded to x's type."""
    u, cols = norm_uses(c), c["cols"]
    f = lambda a: a.astype(dt)
    ref, x = {}, f(inp["x"])
    if u["branch"]:
        s = x + mod_window(c, inp, 2, dt) * f(inp["branch"])
        if u["x_out"]:
            ref["x_out"] = s
        x = f(round_to(s.astype(np.float32), c["xk"]))
    if u["res"]:
        x = x + f(inp["residual"])
    if u["res_out"]:
        ref["residual_out"] = x
    if c["form"] == "rms":
        xhat = x / np.sqrt((x * x).sum(-1, keepdims=True, dtype=dt) / dt(cols) + dt(EPS))
    else:
        d = x - x.sum(-1, keepdims=True, dtype=dt) / dt(cols)
        xhat = d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=dt) / dt(cols) + dt(EPS))
    y = xhat if inp["weight"] is None else xhat * f(inp["weight"])
    if inp["bias"] is not None:
        y = y + f(inp["bias"])
    if u["y_out"]:
        ref["y_out"] = y
    if u["mod"]:
        a = f(round_to(y.astype(np.float32), c["xk"])) * (dt(1) + mod_window(c, inp, 1, dt))
        ref["y_mod"], ref["_terms"] = a + mod_window(c, inp, 0, dt), (a, mod_window(c, inp, 0, dt))
    return ref


def norm_out_kind(c, key):
    return c["rk"] if key == "residual_out" else c["xk"]


def norm_exact(c, ref):
    """the outputs that have ONE defined value: with 16-bit x the product gate * branch is exact in fp32, so x + gate * branch and x' + residual are
    single fp32 roundings of exact sums -> {key: float32 array}"""
    if c["xk"] == "f32" and norm_uses(c)["branch"]:
        return {}
    return {k: round_to(ref[k].astype(np.float32), norm_out_kind(c, k)) for k in ("x_out", "residual_out") if k in ref}


NORM_REFUSALS = (("cols4097", ERR_SHAPE), ("gate-without-branch", ERR_NULL), ("shift-without-ymod", ERR_NULL), ("mod-dtype", ERR_DTYPE))


# ---------------------------------------------------------------------------------------------------
# patch_embed
# ---------------------------------------------------------------------------------------------------
PE_CP = ((1, 1), (3, 1), (4, 1), (3, 2), (4, 2), (5, 2), (3, 4), (4, 4))           # K = 1, 3, 4, 12, 16, 20, 48, 64
PE_E = (8, 64, 120, 136, 640, 768, 1024, 1032, 2056)
PE_GRID = ((1, 1), (1, 9), (3, 5), (2, 8), (17, 1), (3, 11), (3, 40), (4, 4), (3, 3))          # (gh, gw): L = 1, 9, 15, 16, 17, 33, 120, 16, 9
PE_BATCH = (1, 7, 8, 63, 64)
PE_LONG = ((64, 17, 17, 64), (8, 9, 121, 136), (1, 43, 387, 8))                 # (batch, gh, gw, E): the token loop's second pass in each grid regime
PE_POS = ("none", "contig", "pitched")


def _patch_case(table, **kw):
    c = dict(kernel="patch", known=False, seed=22000 + len(table))
    c.update(kw)
    c["K"], c["L"] = c["C"] * c["p"] ** 2, c["gh"] * c["gw"]
    assert c["K"] * c["E"] * 4 <= 65536
    c["id"] = (f"b{c['B']}-c{c['C']}p{c['p']}-g{c['gh']}x{c['gw']}-e{c['E']}-{'b' if c['bias'] else ''}-pos{c['pos']}" + ("-known" if c["known"] else ""))
    table.append(c)


def patch_cases():
    """Keys: B, C, p, gh, gw (patch grid: height = gh p, width = gw p), E, bias, pos (PE_POS), known (integers: bit for bit), K, L, seed"""
    out, i = [], 0
    for C, p in PE_CP:
        for E in PE_E:
            if C * p * p * E * 4 > 65536:
                continue
            gh, gw = PE_GRID[i % 9]
            if i % 4 == 1:
                gh, gw = gw, gh
            B = PE_BATCH[(i + i // 5) % 5]
            if B * gh * gw * E > 1_000_000:
                B = 7
            _patch_case(out, B=B, C=C, p=p, gh=gh, gw=gw, E=E, bias=i % 3 != 1, pos=PE_POS[(i + i // 3) % 3])
            i += 1
    for k, (B, gh, gw, E) in enumerate(PE_LONG):
        for C, p in ((3, 1), (4, 2), (5, 2))[k:k + 2] if k < 2 else ((3, 2), (1, 1)):
            _patch_case(out, B=B, C=C, p=p, gh=gh, gw=gw, E=E, bias=True, pos=PE_POS[1 + (k + C) % 2])
    for k, (C, p) in enumerate(PE_CP):                      # known answers: one per K
        _patch_case(out, B=(2, 8, 64)[k % 3], C=C, p=p, gh=3, gw=7, E=(64, 136, 120, 1032)[k % 4] if C * p * p <= 12 else (64, 136, 120)[k % 3], bias=True,
                    pos=PE_POS[1 + k % 2], known=True)
    return out


def patch_production_cases():
    t = []
    _patch_case(t, B=64, C=3, p=1, gh=32, gw=32, E=640, bias=True, pos="contig", seed=26100)
    return t


def patch_inputs(c):
    rng = np.random.default_rng(c["seed"])
    B, C, p, E, K, L = c["B"], c["C"], c["p"], c["E"], c["K"], c["L"]
    H, W = c["gh"] * p, c["gw"] * p
    if c["known"]:
        ints = lambda lo, hi, *s: rng.integers(lo, hi + 1, s).astype(np.float32)
        return dict(x=ints(-1, 1, B, C, H, W), w=ints(-2, 2, E, C, p, p), bias=ints(-4, 4, E) if c["bias"] else None,
                    pos=ints(-8, 8, L, E) if c["pos"] != "none" else None)
    bf = lambda a: round_to(a, "bf16")
    return dict(x=bf(rng.standard_normal((B, C, H, W))), w=bf(rng.standard_normal((E, C, p, p)) * K ** -0.5), bias=bf(rng.standard_normal(E)) if c["bias"] else None,
                pos=bf(rng.standard_normal((L, E))) if c["pos"] != "none" else None)


def patch_columns(c, x):
    """(B, L, K): the K = (channel, dy, dx) inputs of every token, tokens row by row over the patch grid"""
    B, C, p, gh, gw = c["B"], c["C"], c["p"], c["gh"], c["gw"]
    return x.reshape(B, C, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * p * p)


def patch_reference(c, inp, dt=np.float64):
    """-> dict(conv: conv + bias unrounded, out).  The conv output is a bf16 tensor: `+ pos` starts from its rounded value."""
    conv = patch_columns(c, inp["x"]).astype(dt) @ inp["w"].reshape(c["E"], c["K"]).astype(dt).T
    if inp["bias"] is not None:
        conv = conv + inp["bias"].astype(dt)
    out = conv if inp["pos"] is None else round_to(conv.astype(np.float32), "bf16").astype(dt) + inp["pos"].astype(dt)
    return dict(conv=conv, out=out)


# ---------------------------------------------------------------------------------------------------
# timestep_embed
# ---------------------------------------------------------------------------------------------------
TS_DIM, TS_BATCH = (2, 64, 65, 256, 257), (1, 3, 64, 300)
TS_FIXED = (0.0, 2.0 ** -20, 1.0, 999.0, 1000.0)
# absolute floor of the element-wise check: 4 x the worst absolute error of the fp32 numpy model over every case (tests/test_outer_fwd_cases_cpu.py
# measures it and `python tests/test_outer_fwd_cases_cpu.py` prints it); it decides only where the value's own bf16 ulp is smaller still
TS_ABS_FLOOR = 3e-07


def timestep_cases():
    """Keys: dim, B, pitch (extra elements in the output's row pitch), seed.  t: the five fixed values, then a seeded draw from [0, 1000], in bf16."""
    out = []
    for i, (dim, B) in enumerate((d, b) for d in TS_DIM for b in TS_BATCH):
        c = dict(kernel="timestep", dim=dim, B=B, pitch=(0, 3, 8)[i % 3], seed=23000 + i)
        c["id"] = f"d{dim}-b{B}-p{c['pitch']}"
        out.append(c)
    return out


def timestep_frequencies(dim):
    """TimestepEmbedder.frequencies(dim, bf16): formed in the model's type, (dim // 2,) float32 holding bf16 values"""
    import torch
    from zigma_amd.model_zigma import TimestepEmbedder
    return TimestepEmbedder.frequencies(dim, torch.bfloat16).float().numpy()


def timestep_inputs(c):
    rng = np.random.default_rng(c["seed"])
    t = np.concatenate([np.array(TS_FIXED), rng.uniform(0.0, 1000.0, max(c["B"] - 5, 0))])
    t = np.roll(t, c["seed"] % 5)[:c["B"]] if c["B"] < 5 else t
    return dict(t=round_to(t, "bf16"), freqs=timestep_frequencies(c["dim"]))


def timestep_reference(c, inp, dt=np.float64):
    arg = inp["t"].astype(dt)[:, None] * inp["freqs"].astype(dt)[None]          # (the product of two bf16 values: exact in fp32)
    out = np.concatenate([np.cos(arg), np.sin(arg)], -1)
    return dict(out=np.concatenate([out, np.zeros((c["B"], c["dim"] % 2), dt)], -1))


def bf16_ulp(v):
    """the spacing of bf16 at |v| (8 significant bits), for normal values"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -126))) - 7)


def timestep_worst(got, ref):
    """max over the elements of |got - ref| / max(one bf16 ulp of ref, TS_ABS_FLOOR): must be <= 1"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(bf16_ulp(ref), TS_ABS_FLOOR)))


# ---------------------------------------------------------------------------------------------------
# skinny_linear
# ---------------------------------------------------------------------------------------------------
SK_K = tuple(range(128, 1025, 128))
SK_M = (1, 2, 15, 16, 17, 33, 63, 64)
SK_N = (16, 48, 128, 144)
SK_WIDE = tuple(16 * (2048 * j + r) for j in (1, 2, 3, 4) for r in (0, 1, 7))       # one to four strips per wave on the full grid of 2048 waves
SK_PRODUCTION = ((64, 640, 69120), (64, 768, 110592))


def _skinny_case(table, **kw):
    c = dict(kernel="skinny", known=False, views=True, seed=24000 + len(table))
    c.update(kw)
    c["id"] = f"m{c['m']}-k{c['k']}-n{c['n']}-{'s' if c['silu'] else ''}{'b' if c['bias'] else ''}" + ("-v" if c["views"] else "") + ("-known" if c["known"] else "")
    table.append(c)


def skinny_cases():
    """Keys: m, k, n, silu, bias, views (x, w, bias and out are windows of NaN-filled buffers with row pitches; x and out have rows beyond m),
    known (integers, no SiLU: bit for bit), seed"""
    out, i = [], 0
    for k in SK_K:
        for n in SK_N:
            _skinny_case(out, m=SK_M[(i + i // 8) % 8], k=k, n=n, silu=i % 2 == 0, bias=(i // 2) % 2 == 0, views=i % 5 != 4)
            i += 1
    for m in SK_M:              # every m on both sides of the double-buffered loop (k <= 640 | above)
        for k in ((256, 768) if m % 2 else (640, 1024)):
            _skinny_case(out, m=m, k=k, n=(48, 144)[i % 2], silu=i % 3 == 0, bias=i % 2 == 1)
            i += 1
    for j, n in enumerate(SK_WIDE):
        _skinny_case(out, m=(2, 16, 1, 17)[j % 4], k=128, n=n, silu=j % 2 == 1, bias=j % 3 != 2, views=j % 2 == 0)
    for j, k in enumerate(SK_K):                            # known answers: every k; one of them on the full grid with two strips per wave and a ragged end
        _skinny_case(out, m=SK_M[(j + 3) % 8], k=k, n=16 * (2 * 2048 + 7) if k == 128 else (144, 1040)[j % 2], silu=False, bias=j % 3 != 1, known=True)
    return out


def skinny_production_cases():
    t = []
    for m, k, n in SK_PRODUCTION:
        _skinny_case(t, m=m, k=k, n=n, silu=True, bias=True, views=False, seed=26200 + k)
    return t


def skinny_inputs(c):
    rng = np.random.default_rng(c["seed"])
    m, k, n = c["m"], c["k"], c["n"]
    if c["known"]:          # 16 non-zero columns of +-1 per sample (others per sample), weights in -3 ... 3: |sum| <= 48, + bias <= 56: exact in bf16
        x = np.zeros((m, k), np.float32)
        for r in range(m):
            x[r, rng.permutation(k)[:16]] = rng.choice(np.array([-1.0, 1.0], np.float32), 16)
        w = rng.integers(-3, 4, (n, k)).astype(np.float32)
        w[:, 0] = (np.arange(n) // 16 * 5 + np.arange(n) % 16) % 7 - 3          # (a column that by itself differs from strip to strip)
        return dict(x=x, w=w, bias=rng.integers(-8, 9, n).astype(np.float32) if c["bias"] else None)
    bf = lambda a: round_to(a, "bf16")
    w = rng.standard_normal((n, k), dtype=np.float32)
    w *= np.float32(k ** -0.5)
    return dict(x=bf(rng.standard_normal((m, k)) * (1.5 if c["silu"] else 1.0)), w=bf(w), bias=bf(rng.standard_normal(n)) if c["bias"] else None)


def skinny_reference(c, inp, dt=np.float64, n_rows=None):
    """act(x) @ w^T + bias; SiLU returns a bf16 tensor.  n_rows: only the first n_rows output features"""
    x = inp["x"].astype(dt)
    if c["silu"]:
        x = round_to(zo.silu(x).astype(np.float32), "bf16").astype(dt)
    n = c["n"] if n_rows is None else min(n_rows, c["n"])
    out = np.empty((c["m"], n), dt)
    for a in range(0, n, 8192):            # (in slabs: the float64 copy of an 85 M element weight is not held at once)
        out[:, a:a + 8192] = x @ inp["w"][a:min(a + 8192, n)].astype(dt).T
    if inp["bias"] is not None:
        out = out + inp["bias"][:n].astype(dt)
    return dict(out=out)


# ---------------------------------------------------------------------------------------------------
# final_layer
# ---------------------------------------------------------------------------------------------------
FL_COLS = (8, 72, 128, 200, 640, 648, 768, 1024, 1032, 2048)
FL_NOUT = (1, 3, 4, 15, 16)
FL_ROWS = (1, 7, 15, 16, 17, 130)
FL_REGIMES = ("benign", "mean50", "constant")
FL_EPS = 1e-6
FL_LONG = (65536 + 23, 64, 3)          # rows, cols, n_out: the second pass of the row loop (4096 workgroups x 16 rows)


def _final_case(table, **kw):
    c = dict(kernel="final", seed=25000 + len(table))
    c.update(kw)
    c["id"] = f"{c['rows']}x{c['cols']}-o{c['n_out']}-{'b' if c['bias'] else ''}-{c['regime']}"
    c["seed"] = SEED_MOVED.get(("final", c["id"]), c["seed"])
    c["np"] = 5 if c["cols"] <= 640 else 8 if c["cols"] <= 1024 else 16         # the instantiation (passes of 128 columns)
    table.append(c)


def final_cases():
    """Keys: rows, cols, n_out, bias, regime (FL_REGIMES), np (the instantiation), seed.  x and out are always windows of NaN-filled buffers."""
    out, i = [], 0
    for cols in FL_COLS:
        for n_out in FL_NOUT:
            _final_case(out, rows=FL_ROWS[(i + i // 6) % 6], cols=cols, n_out=n_out, bias=i % 3 != 2, regime=FL_REGIMES[(i + i // 5) % 3])
            i += 1
    _final_case(out, rows=FL_LONG[0], cols=FL_LONG[1], n_out=FL_LONG[2], bias=True, regime="benign")
    _final_case(out, rows=FL_LONG[0], cols=FL_LONG[1], n_out=FL_LONG[2], bias=False, regime="mean50")
    return out


def final_production_cases():
    t = []
    _final_case(t, rows=65536, cols=640, n_out=3, bias=True, regime="benign", seed=26300)
    return t


def final_inputs(c):
    rng = np.random.default_rng(c["seed"])
    rows, cols, n_out = c["rows"], c["cols"], c["n_out"]
    x = rng.standard_normal((rows, cols), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    if c["regime"] == "mean50":
        x = x / np.float32(1.5) + np.float32(50.0)
    if c["regime"] == "constant":           # every other row constant (all rows but the last where there are few): rstd = rsqrt(eps)
        x[0:max(rows - 1, 1):2] = rng.choice(np.array([-2.0, -0.5, 0.25, 1.0, 2.0], np.float32), (len(range(0, max(rows - 1, 1), 2)), 1))
    bf = lambda a: round_to(a, "bf16")
    return dict(x=bf(x), w=bf(rng.standard_normal((n_out, cols)) * cols ** -0.5), bias=bf(rng.standard_normal(n_out)) if c["bias"] else None)


def final_reference(c, inp, dt=np.float64):
    """y = LayerNorm(x) without affine, a bf16 tensor; out = y @ w^T + bias"""
    x = inp["x"].astype(dt)
    d = x - x.sum(-1, keepdims=True, dtype=dt) / dt(c["cols"])
    y = d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=dt) / dt(c["cols"]) + dt(FL_EPS))
    out = round_to(y.astype(np.float32), "bf16").astype(dt) @ inp["w"].astype(dt).T
    return dict(y=y, out=out if inp["bias"] is None else out + inp["bias"].astype(dt))


# ---------------------------------------------------------------------------------------------------
# refusals: (entry point, what is wrong, status); the GPU test builds each from a valid small call
# ---------------------------------------------------------------------------------------------------
REFUSALS = ([("zigma_patch_embed_fwd", "f16", ERR_DTYPE), ("zigma_patch_embed_fwd", "f32", ERR_DTYPE), ("zigma_patch_embed_fwd", "above-64KB", ERR_SHAPE),
             ("zigma_timestep_embed_fwd", "f16", ERR_DTYPE), ("zigma_timestep_embed_fwd", "f32", ERR_DTYPE),
             ("zigma_skinny_linear_fwd", "f16", ERR_DTYPE), ("zigma_skinny_linear_fwd", "f32", ERR_DTYPE), ("zigma_skinny_linear_fwd", "m65", ERR_SHAPE),
             ("zigma_skinny_linear_fwd", "k1152", ERR_SHAPE), ("zigma_skinny_linear_fwd", "n24", ERR_SHAPE), ("zigma_skinny_linear_fwd", "x-off-by-one", ERR_STRIDE),
             ("zigma_skinny_linear_fwd", "w-off-by-one", ERR_STRIDE), ("zigma_skinny_linear_fwd", "out-off-by-one", ERR_STRIDE),
             ("zigma_skinny_linear_fwd", "bias-off-by-one", ERR_STRIDE),
             ("zigma_final_layer_fwd", "f16", ERR_DTYPE), ("zigma_final_layer_fwd", "f32", ERR_DTYPE), ("zigma_final_layer_fwd", "n_out17", ERR_SHAPE),
             ("zigma_final_layer_fwd", "cols2056", ERR_SHAPE)]
            + [("zigma_add_norm_fwd", what, status) for what, status in NORM_REFUSALS])
