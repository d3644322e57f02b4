"""Case tables of the backward-kernel sweep (zigma_selective_scan_bwd, zigma_causal_conv1d_bwd, zigma_add_norm_bwd).

Plain numpy, importable without a GPU (torch is imported only inside the float64 autograd restatements).  Three seeded generators,
scan_cases() / conv_cases() / norm_cases(), yield dicts of PARAMETERS (shape, dtype kind, option switches, seed); *_inputs() makes the
numbers from the seed on demand, already rounded to the case's I/O type, so the kernel and the float64 oracle (oracle/zigma_oracle.py)
see the same values.  test_bwd_fuzz_cases_cpu.py asserts that the tables cover every cell they are meant to cover, that the oracle agrees
with float64 torch autograd on exactly these inputs, and that rounding the oracle's result to the I/O type stays inside every limit;
test_gpu_bwd_fuzz.py runs the kernels.

Layouts: everything here is token-major, (batch, position, channel), as the kernels take it.  Scan: u, delta, B, C, du, ddelta, dB, dC are
in SCAN order; z / dz live at row zi[k] and out / dout at row oi[k] of their tensors (the forward's z_row_index / out_row_index).  Conv: dout
is in scan order, x is read at row perm[k] and dx scattered back through perm.
"""
import numpy as np

from oracle import zigma_oracle as zo

KINDS = ("f32", "bf16", "f16")
R_COLS = 8                      # dt_rank columns in front of the B | C columns of the x_dbl-shaped buffers of the scan cases
EPS = 1e-5                      # the norm cases' epsilon


def round_to(a, kind):
    a = np.asarray(a, dtype=np.float32)
    return zo.bf16_round(a) if kind == "bf16" else zo.fp16_round(a) if kind == "f16" else a


# ---------------------------------------------------------------------------------------------------
# bounds (norm-wise, rel_err): the existing tests' of the same kernel (tests/test_gpu_backward.py); fp16-typed outputs get the bf16
# bound / 8 (three more mantissa bits, the convention of tests/test_gpu_fp16.py), fp32 sums keep the bf16 bound in fp16.
# ---------------------------------------------------------------------------------------------------
def scan_bounds(kind):
    io = {"f32": 5e-5, "bf16": 1e-2, "f16": 1e-2 / 8}[kind]
    sums = {"f32": 5e-5, "bf16": 2e-3, "f16": 2e-3}[kind]
    return dict(du=io, ddelta=io, dz=io, dA=sums, dB=sums, dC=sums, dD=sums, ddelta_bias=sums)


def conv_bounds(kind):
    return dict(dx={"f32": 2e-5, "bf16": 5e-3, "f16": 5e-3 / 8}[kind], dweight={"f32": 2e-5, "bf16": 1e-4, "f16": 1e-4}[kind],
                dbias={"f32": 2e-5, "bf16": 1e-4, "f16": 1e-4}[kind])


def norm_bounds(c):
    typed = {"f32": 2e-5, "bf16": 5e-3, "f16": 5e-3 / 8}          # an output stored in that type (the norm kernel borrows conv's 16-bit bound)
    sums = 2e-5 if (c["xk"], c["rk"], c["wk"] or c["xk"]) == ("f32", "f32", "f32") else 1e-4
    return dict(dx=typed[c["xk"]], dresidual=typed[c["rk"]], dweight=sums, dbias=sums)


ROW_GUARD = 4.0                 # row-wise / element-wise limit in units of the norm-wise bound (a guard; the rounded reference needs < 1)


def rowwise_worst(got, ref, bound):
    """max over ALL rows (last axis = the row) of |got_row - ref_row| / (bound * max(|ref_row|, rms of the row norms))"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.linalg.norm((got - ref).reshape(-1, ref.shape[-1]), axis=1)
    rn = np.linalg.norm(ref.reshape(-1, ref.shape[-1]), axis=1)
    den = bound * np.maximum(np.maximum(rn, np.sqrt(np.mean(rn * rn))), 1e-300)
    return float(np.max(d / den))


def elementwise_worst(got, ref, bound):
    """max over ALL elements of |got - ref| / (bound * max(|ref|, rms(ref))): the reduced gradients"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = bound * np.maximum(np.maximum(np.abs(ref), np.sqrt(np.mean(ref * ref))), 1e-300)
    return float(np.max(np.abs(got - ref) / den))


ROW_OUTPUTS = ("du", "ddelta", "dz", "dB", "dC", "dx", "dresidual")       # checked row by row; everything else element by element


def worst_ratio(key, got, ref, bound):
    return rowwise_worst(got, ref, bound) if key in ROW_OUTPUTS else elementwise_worst(got, ref, bound)


# ---------------------------------------------------------------------------------------------------
# scan backward
# ---------------------------------------------------------------------------------------------------
SCAN_L = (1, 3, 15, 16, 17, 48, 100, 257)
SCAN_LONG = (2048 + 37, 4096 + 32)      # the forward's chunk edge; the length from which the forward splits the sequence


def _scan_id(c):
    f = "".join(ch for ch, on in (("z", c["z"]), ("D", c["D"]), ("b", c["bias"]), ("s", c["softplus"]), ("t", c["tables"]),
                                  ("g", c["dbc_slices"]), ("h", c["dz_half"]), ("x", c["bc_slices"]), ("p", c["pad"]),
                                  ("k", c["ckpt"] == "fwd")) if on)
    return f"{c['kind']}-n{c['N']}-b{c['B']}-d{c['dim']}-L{c['L']}-{f or 'plain'}" + (f"-r{c['reset']}" if c["reset"] else "")


def scan_cases():
    """~60 cases.  Keys: kind, N, B, dim, L, z / D / bias / softplus, tables (both row tables, two different permutations; needs z),
    dbc_slices (dB / dC written into columns of one fp32 (B, L, R + 2N) buffer), dz_half (dz into the upper half of a (B, L, 2 dim) buffer),
    bc_slices (B / C read from columns of one (B, L, R + 2N) buffer), pad (extra elements in the row pitch of u / delta / dout),
    ckpt ("fwd": the forward kernel writes the checkpoints, needs z | "own": the backward's phase 1), carries (the forward gets the
    chunk-carry tensor: it splits the sequence), reset (reset_period), twice (also run a second time: bit-identical), seed."""
    rng = np.random.default_rng(20241)
    out = []

    def add(**kw):
        c = dict(kernel="scan", carries=False, reset=0, twice=False)
        c.update(kw)
        if not c["z"]:
            c.update(tables=False, dz_half=False, ckpt="own")
        c["seed"] = 7000 + len(out)
        c["id"] = _scan_id(c)
        out.append(c)

    flip = lambda: bool(rng.integers(0, 2))
    for i in range(48):
        opts = int(rng.integers(0, 16))
        add(kind=KINDS[i % 3], N=(16, 8)[(i // 3) % 2], L=SCAN_L[i % 8], B=1 + (i // 2) % 3, dim=(64, 128, 192)[(i // 5) % 3],
            z=bool(opts & 1), D=bool(opts & 2), bias=bool(opts & 4), softplus=bool(opts & 8), tables=flip(), dbc_slices=flip(),
            dz_half=flip(), bc_slices=flip(), pad=8 * int(rng.integers(0, 2)), ckpt=("fwd", "own")[int(rng.integers(0, 2))])
    for j, (reset, tables, kind) in enumerate((r, t, k) for r in (16, 32) for t in (False, True) for k in KINDS):
        add(kind=kind, N=(16, 8)[j % 2], L=(48, 100, 257, 17)[j % 4], B=1 + j % 3, dim=(128, 64, 192)[j % 3], z=tables or flip(), D=flip(),
            bias=flip(), softplus=flip(), tables=tables, dbc_slices=flip(), dz_half=flip(), bc_slices=flip(), pad=8 * (j % 2),
            ckpt=("fwd", "own")[(j // 3) % 2], reset=reset)
    # the two long cases: forward-written checkpoints through the forward's sequence split
    add(kind="f32", N=16, L=SCAN_LONG[0], B=1, dim=64, z=True, D=True, bias=True, softplus=True, tables=False, dbc_slices=True, dz_half=True,
        bc_slices=True, pad=0, ckpt="fwd", carries=True)
    add(kind="bf16", N=16, L=SCAN_LONG[1], B=1, dim=64, z=True, D=True, bias=True, softplus=True, tables=True, dbc_slices=False, dz_half=False,
        bc_slices=False, pad=8, ckpt="fwd", carries=True)
    add(kind="f16", N=16, L=SCAN_LONG[0], B=1, dim=64, z=True, D=False, bias=True, softplus=True, tables=True, dbc_slices=True, dz_half=True,
        bc_slices=True, pad=0, ckpt="own")
    for kind in KINDS:          # determinism: the first gated case of every I/O type runs twice
        next(c for c in out if c["kind"] == kind and c["z"] and c["L"] >= 48)["twice"] = True
    return out


def scan_inputs(c, L=None):
    """token-major numpy inputs of a scan case (L: a truncated length for the CPU checks of the long cases)"""
    L = L or c["L"]
    kind, Bsz, dim, N = c["kind"], c["B"], c["dim"], c["N"]
    rng = np.random.default_rng(c["seed"])
    r = lambda *s: round_to(rng.standard_normal(s), kind)
    inp = dict(u=r(Bsz, L, dim), delta=round_to(0.5 * rng.random((Bsz, L, dim)), kind), A=(-0.5 * rng.random((dim, N)) - 0.05).astype(np.float32),
               Bm=r(Bsz, L, N), Cm=r(Bsz, L, N), dout=r(Bsz, L, dim), z=None, D=None, delta_bias=None, zi=None, oi=None)
    if c["z"]:
        inp["z"] = r(Bsz, L, dim)
    if c["D"]:
        inp["D"] = rng.standard_normal(dim).astype(np.float32)
    if c["bias"]:
        inp["delta_bias"] = (0.5 * rng.random(dim)).astype(np.float32)
        inp["delta_bias"][0] = 25.0                         # the softplus pass-through branch
    if c["tables"]:
        inp["zi"], inp["oi"] = rng.permutation(L).astype(np.int32), rng.permutation(L).astype(np.int32)
        if L > 1 and np.array_equal(inp["zi"], inp["oi"]):
            inp["oi"] = np.roll(inp["oi"], 1)
    return inp


def scan_reference(c, inp, out=None):
    """float64 oracle in the layout of the kernel's outputs.  `out`: the forward's ungated y as the KERNEL was given it (token-major, at rows
    oi) — dz is then formed from it, which is the kernel's documented contract; everything else never sees a kernel result."""
    sc = lambda a, idx: a if (a is None or idx is None) else a[:, idx]            # token order -> scan order
    cf = lambda a, s: np.ascontiguousarray(np.asarray(a, np.float64)[:, s].transpose(0, 2, 1))      # (B, l, C) -> (B, C, l)
    z_s, dout_s = sc(inp["z"], inp["zi"]), sc(inp["dout"], inp["oi"])
    L = inp["u"].shape[1]
    period = c["reset"] or L
    parts = []
    for a in range(0, L, period):        # reset_period: independent sequences, the gradients of the parameters add up
        s = slice(a, min(a + period, L))
        parts.append(zo.selective_scan_bwd(cf(inp["u"], s), cf(inp["delta"], s), inp["A"], cf(inp["Bm"], s), cf(inp["Cm"], s), inp["D"],
                                           None if z_s is None else cf(z_s, s), inp["delta_bias"], cf(dout_s, s), c["softplus"]))
    ref = {}
    for k in ("du", "ddelta", "dB", "dC", "dz"):
        ref[k] = None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=-1).transpose(0, 2, 1)
    for k in ("dA", "dD", "ddelta_bias"):
        ref[k] = None if parts[0][k] is None else sum(p[k] for p in parts)
    if z_s is not None:
        dz_s = ref["dz"]
        if out is not None:
            zf, of = np.asarray(z_s, np.float64), np.asarray(sc(out, inp["oi"]), np.float64)
            sg = zo.sigmoid(zf)
            dz_s = np.asarray(dout_s, np.float64) * of * sg * (1.0 + zf * (1.0 - sg))
        if inp["zi"] is not None:
            full = np.empty_like(dz_s)
            full[:, inp["zi"]] = dz_s
            dz_s = full
        ref["dz"] = dz_s
    return ref


def torch_scan(u, delta, A, Bm, Cm, D, z, delta_bias, softplus, zi=None, oi=None, reset=0):
    """The whole operator in plain torch (any dtype / device), token-major, tables and reset_period included: what autograd differentiates."""
    import torch
    import torch.nn.functional as F
    dl = delta if delta_bias is None else delta + delta_bias
    if softplus:
        dl = F.softplus(dl)
    Bsz, L, dim = u.shape
    h, ys = torch.zeros(Bsz, dim, A.shape[1], dtype=u.dtype, device=u.device), []
    for l in range(L):
        if reset and l % reset == 0:
            h = torch.zeros_like(h)
        d = dl[:, l, :, None]
        h = torch.exp(d * A) * h + d * u[:, l, :, None] * Bm[:, l, None, :]
        ys.append((h * Cm[:, l, None, :]).sum(-1))
    y = torch.stack(ys, 1)
    if D is not None:
        y = y + u * D
    if z is not None:
        y = y * F.silu(z if zi is None else z.index_select(1, zi))
    return y if oi is None else torch.zeros_like(y).index_copy(1, oi, y)


# ---------------------------------------------------------------------------------------------------
# conv backward
# ---------------------------------------------------------------------------------------------------
CONV_DIM = (4, 100, 256, 260, 1280)
CONV_L = (1, 2, 3, 15, 16, 17, 127, 128, 129, 300)


def conv_cases():
    """~55 cases.  Keys: kind (I/O type), wkind (weight / bias type: the I/O type or f32), W, silu, bias, B, dim, L, table, x_pad (extra
    elements in x's row pitch), dx_pad (0: the wrapper allocates dx; else a preallocated dx with that much pitch padding), reset, twice, seed."""
    rng = np.random.default_rng(20242)
    combos = [(k, wk, W, s) for k in KINDS for wk in ((k,) if k == "f32" else (k, "f32")) for W in (2, 3, 4) for s in (False, True)]
    combos += [(k, k, W, s) for k in KINDS for W in (2, 3, 4) for s in (True, False)]
    out = []

    def add(**kw):
        c = dict(kernel="conv", reset=0, twice=False)
        c.update(kw)
        c["seed"] = 8000 + len(out)
        c["id"] = (f"{c['kind']}-w{c['wkind']}-W{c['W']}-{'silu' if c['silu'] else 'lin'}-b{c['B']}-d{c['dim']}-L{c['L']}"
                   + ("-bias" if c["bias"] else "") + ("-tab" if c["table"] else "") + (f"-xp{c['x_pad']}" if c["x_pad"] else "")
                   + (f"-dxp{c['dx_pad']}" if c["dx_pad"] else "") + (f"-r{c['reset']}" if c["reset"] else ""))
        out.append(c)

    for i, (kind, wkind, W, silu) in enumerate(combos):
        add(kind=kind, wkind=wkind, W=W, silu=silu, bias=bool(rng.integers(0, 2)), B=1 + i % 3, dim=CONV_DIM[(3 * i + i // 10) % 5],
            L=CONV_L[(7 * i + i // 10) % 10], table=bool(rng.integers(0, 2)), x_pad=4 * int(rng.integers(0, 3)), dx_pad=(0, 4, 12)[int(rng.integers(0, 3))])
    for j, kind in enumerate(KINDS + KINDS):      # reset_period 16, a table that permutes inside every sequence; whole and ragged last sequence
        add(kind=kind, wkind=("f32" if j >= 3 else kind), W=(4, 3, 2)[j % 3], silu=j % 2 == 0, bias=j % 2 == 0, B=2, dim=(256, 260, 100)[j % 3],
            L=(80, 129, 300)[j % 3], table=True, x_pad=4 * (j % 2), dx_pad=(0, 4)[j // 3], reset=16)
    for kind in KINDS:
        max((c for c in out if c["kind"] == kind), key=lambda c: min(c["L"], 130) * min(c["dim"], 300))["twice"] = True
    return out


def conv_inputs(c):
    rng = np.random.default_rng(c["seed"])
    Bsz, L, dim, W = c["B"], c["L"], c["dim"], c["W"]
    inp = dict(x=round_to(rng.standard_normal((Bsz, L, dim)), c["kind"]), dout=round_to(rng.standard_normal((Bsz, L, dim)), c["kind"]),
               w=round_to(rng.standard_normal((dim, W)) * 0.5, c["wkind"]), b=None, perm=None)
    if c["bias"]:
        inp["b"] = round_to(rng.standard_normal(dim) * 0.2, c["wkind"])
    if c["table"]:
        period = c["reset"] or L
        inp["perm"] = np.concatenate([a + rng.permutation(min(period, L - a)) for a in range(0, L, period)]).astype(np.int32)
    return inp


def conv_reference(c, inp):
    x = inp["x"] if inp["perm"] is None else inp["x"][:, inp["perm"]]
    L = x.shape[1]
    period = c["reset"] or L
    dxs, dw, db = [], 0.0, None
    for a in range(0, L, period):
        s = slice(a, min(a + period, L))
        pdx, pdw, pdb = zo.causal_conv1d_bwd(x[:, s].transpose(0, 2, 1), inp["w"], inp["b"], inp["dout"][:, s].transpose(0, 2, 1),
                                             "silu" if c["silu"] else None)
        dxs.append(pdx.transpose(0, 2, 1))
        dw = dw + pdw
        db = pdb if pdb is None else (pdb if db is None else db + pdb)
    dx = np.concatenate(dxs, axis=1)
    if inp["perm"] is not None:
        full = np.empty_like(dx)
        full[:, inp["perm"]] = dx            # dx[row[k]] = dx'[k]
        dx = full
    return dict(dx=dx, dweight=dw, dbias=db)


def torch_conv(x, w, b, silu, perm=None, reset=0):
    import torch
    import torch.nn.functional as F
    xs = x if perm is None else x.index_select(1, perm)
    L, W = xs.shape[1], w.shape[1]
    outs = []
    for a in range(0, L, reset or L):
        seg = xs[:, a:a + (reset or L)]
        xp = F.pad(seg, (0, 0, W - 1, 0))
        o = sum(w[:, t] * xp[:, t:t + seg.shape[1]] for t in range(W))
        outs.append(o if b is None else o + b)
    o = torch.cat(outs, 1)
    return F.silu(o) if silu else o


# ---------------------------------------------------------------------------------------------------
# norm backward
# ---------------------------------------------------------------------------------------------------
NORM_COLS = (1, 5, 64, 98, 256, 260, 640, 768, 772, 1000, 2048)
NORM_ROWS = (1, 3, 7, 2048, 2053, 4 * 2048 + 5)
NORM_BRANCHES = ((4, 3), (4, 8), (1, 4), (1, 12), (1, 32))
# the dispatch of zigma_add_norm_bwd is (x type) x (residual: f32 | x's) x (weight: f32 | x's) = 12 slots; for x = f32 the four slots are one
# and the same triple, so nine distinct triples exist and the table holds all of them
NORM_DTYPES = [("f32", "f32", "f32")] + [(k, r, w) for k in ("bf16", "f16") for r in ("f32", k) for w in ("f32", k)]
NORM_WANTS = ((True, False), (False, True), (True, True))


def norm_branch(cols, pitch_pad):
    """(VEC, ITERS) of launch_norm_bwd (csrc/norm_bwd.hip) for contiguous, allocator-aligned operands whose xsum / dy / dresidual_out rows
    carry pitch_pad extra elements; None: refused (cols > 2048)."""
    vec = cols % 4 == 0 and (cols + pitch_pad) % 4 == 0
    if vec and cols <= 768:
        return (4, 3)
    if vec and cols <= 2048:
        return (4, 8)
    return (1, 4) if cols <= 256 else (1, 12) if cols <= 768 else (1, 32) if cols <= 2048 else None


def norm_cases():
    """~60 cases.  Keys: xk / rk / wk (types of x = dy = dx, of the residual stream = xsum = dresidual(_out), of the weight; wk None: no
    weight), rms, rows, cols, bias, dres_out, want_dx, want_dres, pitch_pad, branch (expected launch branch), error (the call must raise), seed."""
    rng = np.random.default_rng(20243)
    out = []

    def add(**kw):
        c = dict(kernel="norm", error=False, twice=False)
        c.update(kw)
        if c["cols"] == 1:
            # one column: RMSNorm's ds = wdy (1 - xhat^2) rstd with xhat^2 = 1 - eps / (x^2 + eps) cancels to ~eps in any fp32 evaluation
            # (LayerNorm's is exactly 0); the incoming residual gradient keeps the result well conditioned
            c["dres_out"] = True
        c["branch"] = norm_branch(c["cols"], c["pitch_pad"])
        c["seed"] = 9000 + len(out)
        c["id"] = (f"x{c['xk']}-r{c['rk']}-w{c['wk']}-{'rms' if c['rms'] else 'ln'}-{c['rows']}x{c['cols']}" + ("-bias" if c["bias"] else "")
                   + ("-dro" if c["dres_out"] else "") + f"-{'x' if c['want_dx'] else ''}{'r' if c['want_dres'] else ''}"
                   + (f"-p{c['pitch_pad']}" if c["pitch_pad"] else ""))
        out.append(c)

    for i in range(44):
        xk, rk, wk = NORM_DTYPES[i % 9]
        cols, rows = NORM_COLS[i % 11], NORM_ROWS[(i + i // 11) % 6]
        if rows * cols > 6_500_000:
            rows = 3
        want = NORM_WANTS[i % 3]
        add(xk=xk, rk=rk, wk=None if i % 7 == 3 else wk, rms=bool((i // 2) % 2), rows=rows, cols=cols, bias=bool(rng.integers(0, 2)),
            dres_out=bool(rng.integers(0, 2)), want_dx=want[0], want_dres=want[1], pitch_pad=8 * int(rng.integers(0, 2)))
    # a pitch that is not a multiple of 4 under cols % 4 == 0: the scalar branches (1, 12) and (1, 32)
    for j, (cols, rms) in enumerate((cc, r) for cc in (260, 640, 768, 772, 1000, 2048) for r in (True, False)):
        xk, rk, wk = NORM_DTYPES[(2 * j + 1) % 9]
        want = NORM_WANTS[(j + 2) % 3]
        add(xk=xk, rk=rk, wk=wk, rms=rms, rows=(7, 2053, 3, 2048)[j % 4], cols=cols, bias=not rms or j % 4 == 0, dres_out=j % 3 != 0,
            want_dx=want[0], want_dres=want[1], pitch_pad=(1, 3, 2)[j % 3])
    # what a 16-bit model trains with: x 16-bit, fp32 residual stream, 16-bit weight
    for j, (k, cols) in enumerate((k, cc) for k in ("bf16", "f16") for cc in (640, 768)):
        add(xk=k, rk="f32", wk=k, rms=j % 2 == 0, rows=(2053, 2048)[j % 2], cols=cols, bias=j % 2 == 1, dres_out=True, want_dx=True, want_dres=True,
            pitch_pad=0)
    add(xk="bf16", rk="f32", wk="bf16", rms=True, rows=3, cols=2049, bias=False, dres_out=False, want_dx=True, want_dres=False, pitch_pad=0, error=True)
    for k in KINDS:
        next(c for c in out if c["xk"] == k and c["rows"] >= 2048 and c["wk"])["twice"] = True
    return out


def norm_inputs(c):
    rng = np.random.default_rng(c["seed"])
    rows, cols = c["rows"], c["cols"]
    inp = dict(xsum=round_to(rng.standard_normal((rows, cols)) + (0.0 if c["rms"] else 0.3), c["rk"]), dy=round_to(rng.standard_normal((rows, cols)), c["xk"]),
               w=None, dres_out=None)
    if c["wk"]:
        inp["w"] = round_to(1.0 + 0.2 * rng.standard_normal(cols), c["wk"])
    if c["dres_out"]:
        inp["dres_out"] = round_to(rng.standard_normal((rows, cols)), c["rk"])
    return inp


def norm_reference(c, inp):
    """the oracle sees x = xsum (what the kernel reads) and no residual; dx and dresidual are the same values in two types"""
    ds, dw, db, _ = zo.fused_add_norm_bwd(inp["xsum"], inp["w"], np.zeros(c["cols"]) if c["bias"] else None, None, inp["dy"], inp["dres_out"],
                                          eps=EPS, rms=c["rms"])
    return dict(dx=ds if c["want_dx"] else None, dresidual=ds if c["want_dres"] else None, dweight=dw, dbias=db)


def torch_norm(x, w, b, eps, rms):
    import torch
    if rms:
        xhat = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    else:
        mu = x.mean(-1, keepdim=True)
        xhat = (x - mu) * torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    y = xhat if w is None else xhat * w
    return y if b is None else y + b
