"""Case tables of the sweep of the text-conditioning side's kernels: zigma_cross_attn_fwd (bf16, fp16), zigma_cross_attn_bwd (bf16) and
zigma_scale_reduce_bwd (bf16).

Plain numpy, importable without a GPU (torch is imported only inside xattn_model, the rounding model).  Three seeded generators,
xattn_fwd_cases() / xattn_bwd_cases() / glue_cases(), yield dicts of PARAMETERS; *_inputs() makes the numbers from the seed on demand, already
rounded to the case's I/O type, so the kernel and the float64 reference see the same values; *_reference() is the float64 evaluation:
softmax(scale Q K^T) V per head with its analytic gradients, and the glue formulas of include/zigma_hip.h.  test_attn_cases_cpu.py asserts that
the tables cover every cell they are meant to cover, that the references agree with float64 torch autograd on exactly these inputs and that
the inputs leave the rounding model and the rounded reference inside the limits; test_gpu_attn_sweep.py runs the kernels.

What the axes are about (csrc/cross_attn.hip, csrc/cross_attn_bwd.hip): a workgroup takes 4 waves x `tiles` tiles of 16 tokens, tiles = 8 from
seqlen 512 on and 4 below; the forward has the instantiations <5 | 8 key blocks, MASK_ALL> split at n_ctx 64 / 80 / 112, the backward <5> / <8>
split at 80 and one fp32 partial of dK / dV per workgroup of tokens (`chunks`).  Rounding, the comparison helpers and ROW_GUARD are the
backward sweep's (bwd_fuzz_cases).
"""
import numpy as np

from bwd_fuzz_cases import ROW_GUARD, elementwise_worst, round_to, rowwise_worst  # noqa: F401  (re-exported to the two test files)

D = 64                              # head dim
SCALE0 = 64 ** -0.5
ATTN_L = (1, 15, 16, 17, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1025)
FWD_NCTX = (1, 5, 15, 16, 17, 63, 64, 65, 77, 79, 80, 81, 111, 112, 113, 127, 128)
BWD_NCTX = (1, 5, 16, 17, 64, 77, 79, 80, 81, 96, 112, 113, 128)
HEADS = (1, 2, 3, 8)
SCALES = (SCALE0, 0.2, 0.05)
GAINS = (1, 6)                      # on q: 6 -> peaked rows (mean largest probability about 0.7 at 77 keys); 12 breaks the model's cap
Q_ONEHOT, K_ONEHOT = 256.0, 4.0     # known-answer cases: the winning logit leads by 256 * 4 / 8 = 128, exp(-128) is 0 in fp32

# norm-wise base bounds: the existing tests' of the same kernel (test_gpu_parity.py / test_gpu_fp16.py / test_gpu_backward.py)
FWD_BASE = {"bf16": 6e-3, "f16": 7.5e-4}
BWD_BASE = 1e-2
GLUE_BASE = 3e-3
MODEL_MARGIN = 2.0                  # case bound = max(base, 2 x e_model): the kernels round the unnormalised exponentials and sum in another
MODEL_CAP = 2.0                     # order than the model — an error of the model's size, not equal to it; inputs keep e_model <= 2 x base


def case_bound(base, e_model):
    return max(base, MODEL_MARGIN * e_model)


def fwd_inst(n_ctx):
    """<NKB, MASK_ALL> of zigma_cross_attn_fwd's dispatch"""
    return (5, n_ctx <= 64) if n_ctx <= 80 else (8, n_ctx <= 112)


def bwd_inst(n_ctx):
    return 5 if n_ctx <= 80 else 8


def tiles(L):
    return 8 if L >= 512 else 4


def chunks(L):
    """workgroups of tokens per (sample, head) = zigma_cross_attn_bwd_chunks"""
    return -(-L // (64 * tiles(L)))


def ragged(L):
    return L % 16 != 0


FWD_INSTS = ((5, True), (5, False), (8, True), (8, False))
_FWD_PAIR_NCTX = {(5, True): (64, 17), (5, False): (77, 80), (8, True): (81, 112), (8, False): (113, 128)}
_BWD_PAIR_NCTX = {5: (77, 80, 17, 79), 8: (81, 128, 96, 112)}


# cases whose rounding model broke its cap of 2 x base at gain 6 (test_attn_cases_cpu.py): the gain is lowered, never the cap raised
_LOWERED_GAIN = {"f16-b3-L16-h1-n127-pair-g6": 4}          # 48 rows of one head: e_model 1.52e-3 against the cap of 1.5e-3


def _attn_id(c):
    f = "".join(ch for ch, on in (("q", c["q_slice"]), ("o", c.get("do_slice")), ("p", c["pad"])) if on)
    s = "" if c["scale"] == SCALE0 else f"-s{c['scale']}"
    return (f"{c['kind']}-b{c['B']}-L{c['L']}-h{c['H']}-n{c['n_ctx']}-{c['kv']}{'-' + f if f else ''}-g{c['gain']}{s}"
            + (f"-{c['known']}" if c["known"] else ""))


def _attn_table(kernel, kinds, nctx, pair_nctx, inst_of, seed0, reps=1, walk=(5, 3)):
    out = []

    def add(**kw):
        c = dict(kernel=kernel, known=None, twice=False, do_slice=False)
        c.update(kw)
        if kernel == "xattn_fwd":
            c["do_slice"] = False
        if c["L"] >= 511 and c["H"] == 8:
            c["B"] = 1
        if c["scale"] == 0.2:
            c["gain"] = 1               # 6 x 8 x 0.2: logits of deviation 10, past what the model's cap allows
        c["seed"] = seed0 + len(out)
        c["id"] = _attn_id(c)
        if c["id"] in _LOWERED_GAIN:
            c["gain"] = _LOWERED_GAIN[c["id"]]
            c["id"] = _attn_id(c)
        out.append(c)

    for ki, kind in enumerate(kinds):
        # every n_ctx `reps` times per type, the lengths walked with a stride coprime to their number (stride and start
        # chosen so that test_attn_cases_cpu.py's coverage holds)
        for i, n in enumerate(nctx * reps):
            j = i + len(nctx) * reps * ki
            add(kind=kind, n_ctx=n, L=ATTN_L[(walk[0] * j + walk[1]) % 16], H=HEADS[j % 4], B=1 + j % 3, kv=("pair", "halves")[j % 2], q_slice=bool((j // 2) % 2),
                do_slice=bool((j // 3) % 2), pad=bool((j // 4) % 2), scale=SCALES[(0, 0, 0, 1, 0, 2, 0)[j % 7]], gain=GAINS[(j + 1) % 2])
        # the pairing: every instantiation meets a ragged multi-chunk length of the four-tile form (257 / 511) and of the eight-tile form
        # (513 / 1000 / 1025), both gains at each
        for a, inst in enumerate(sorted(pair_nctx, key=str)):
            ns = pair_nctx[inst]
            for r in range(len(ns) // 2):
                g = (a + ki + r) % 2
                add(kind=kind, n_ctx=ns[2 * r], L=(257, 511)[(a + r) % 2], H=(2, 3)[a % 2], B=2, kv=("halves", "pair")[a % 2], q_slice=a % 2 == 0,
                    do_slice=a % 2 == 1, pad=r == 0, scale=SCALE0, gain=GAINS[g], twice=r == 0)
                add(kind=kind, n_ctx=ns[2 * r + 1], L=(1000, 513, 1025)[(a + r) % 3], H=(8, 2)[(a + r) % 2], B=2, kv=("pair", "halves")[a % 2],
                    q_slice=a % 2 == 1, do_slice=a % 2 == 0, pad=r == 1, scale=SCALE0, gain=GAINS[1 - g])
    return out, add


def xattn_fwd_cases():
    """~55 cases.  Keys: kind (bf16 | f16), B, L, H, n_ctx, kv ("pair": K / V = kv[:, :, 0 / 1] of a (B, rows, 2, C) buffer | "halves": the column
    halves of a (B, rows, 2C) buffer; the buffer has 3 rows past n_ctx), q_slice (q = columns 64.. of a (B, rows, 64 + C) buffer), pad (2 more
    rows in q's buffer: a padded batch stride, rows past L), scale, gain (on q), known (None | "onehot+zero": one-hot rows and rows of
    zeros), twice (also run a second time: bit-identical), seed.  Everything of a buffer outside the operand is NaN."""
    out, add = _attn_table("xattn_fwd", ("bf16", "f16"), FWD_NCTX, _FWD_PAIR_NCTX, fwd_inst, 11000, walk=(15, 2))
    for kind in ("bf16", "f16"):
        # (the peaked n_ctx = 127 case of the walk above runs at a lowered gain in fp16: this one keeps gain 6 at that instantiation's edge)
        add(kind=kind, n_ctx=127, L=64, H=2, B=2, kv="halves", q_slice=False, pad=True, scale=SCALE0, gain=6)
        add(kind=kind, n_ctx=64, L=513, H=2, B=1, kv="halves", q_slice=True, pad=True, scale=SCALE0, gain=1, known="onehot+zero")
        add(kind=kind, n_ctx=37, L=255, H=3, B=2, kv="pair", q_slice=False, pad=False, scale=SCALE0, gain=1, known="onehot+zero")
    return out


def xattn_bwd_cases():
    """~37 cases, bf16.  The forward's keys and do_slice (dout = columns 64.. of a wider buffer; pad gives it the 2 more rows too);
    known: "onehot" (dq = dk = 0 exactly, dv exact) | "onehot+zero" (rows of zeros among them: dk = 0 exactly, dq and dv at the ordinary limits)."""
    out, add = _attn_table("xattn_bwd", ("bf16",), BWD_NCTX, _BWD_PAIR_NCTX, bwd_inst, 12000, reps=2, walk=(13, 5))
    add(kind="bf16", n_ctx=64, L=513, H=2, B=1, kv="halves", q_slice=True, do_slice=True, pad=True, scale=SCALE0, gain=1, known="onehot")
    add(kind="bf16", n_ctx=37, L=257, H=3, B=2, kv="pair", q_slice=False, do_slice=False, pad=False, scale=SCALE0, gain=1, known="onehot")
    add(kind="bf16", n_ctx=16, L=65, H=1, B=2, kv="pair", q_slice=False, do_slice=True, pad=False, scale=SCALE0, gain=1, known="onehot+zero")
    return out


def onehot_choice(c):
    """(B, L, H) key index every q row of a known-answer case points at; -1: a row of zeros"""
    b, t, h = np.ogrid[:c["B"], :c["L"], :c["H"]]
    j = (3 * t + 5 * h + b) % c["n_ctx"]
    return np.where(t % 11 == 5, -1, j) if c["known"] == "onehot+zero" else j + 0 * b


def exact_zero(c):
    """gradients of a known-answer case that are analytically zero (float64 leaves exp(-128)-sized noise, the kernel must return 0): one-hot rows
    have dS = 0, and a q row of zeros adds nothing to dk = dS^T q"""
    return {"onehot": ("dq", "dk"), "onehot+zero": ("dk",)}.get(c["known"], ())


def _attn_inputs(c, with_dout):
    rng = np.random.default_rng(c["seed"])
    B, L, H, n, kind = c["B"], c["L"], c["H"], c["n_ctx"], c["kind"]
    C = H * D
    r = lambda *s: round_to(rng.standard_normal(s), kind)
    inp = dict(q=round_to(c["gain"] * rng.standard_normal((B, L, C)), kind), k=r(B, n, C), v=r(B, n, C))
    if with_dout:
        inp["dout"] = r(B, L, C)
    if c["known"]:
        assert n <= D
        k = np.zeros((B, n, H, D), np.float32)
        k[:, np.arange(n), :, np.arange(n)] = K_ONEHOT            # k_j = 4 e_j in every head
        j = onehot_choice(c)
        q = np.zeros((B, L, H, D), np.float32)
        bb, tt, hh = np.nonzero(j >= 0)
        q[bb, tt, hh, j[bb, tt, hh]] = Q_ONEHOT
        inp["q"], inp["k"] = q.reshape(B, L, C), k.reshape(B, n, C)
        if with_dout:
            # multiples of 1/8: every product and every sum of the backward is exact in fp32 whatever the order, so "exactly" is meaningful
            quant = lambda a: (np.clip(np.rint(8 * a), -32, 32) / 8).astype(np.float32)
            inp["v"], inp["dout"] = quant(inp["v"]), quant(inp["dout"])
    return inp


def xattn_fwd_inputs(c):
    return _attn_inputs(c, False)


def xattn_bwd_inputs(c):
    return _attn_inputs(c, True)


def to_heads(a, H):
    """(B, n, H * 64) -> (B, H, n, 64) float64"""
    a = np.asarray(a, np.float64)
    return a.reshape(a.shape[0], a.shape[1], H, D).transpose(0, 2, 1, 3)


def from_heads(a):
    return a.transpose(0, 2, 1, 3).reshape(a.shape[0], a.shape[2], -1)


def head_rows(a, H):
    """(B, n, H * 64) -> (B, n, H, 64): the row of the row-wise limit is one token (or key) of one head"""
    a = np.asarray(a)
    return a.reshape(a.shape[0], a.shape[1], H, D)


def _probs(c, inp):
    qh, kh = to_heads(inp["q"], c["H"]), to_heads(inp["k"], c["H"])
    s = qh @ kh.transpose(0, 1, 3, 2) * c["scale"]
    p = np.exp(s - s.max(-1, keepdims=True))
    return qh, kh, p / p.sum(-1, keepdims=True)


def xattn_fwd_reference(c, inp):
    _, _, p = _probs(c, inp)
    return dict(out=from_heads(p @ to_heads(inp["v"], c["H"])))


def xattn_bwd_reference(c, inp):
    """P = softmax(scale Q K^T); dV = P^T dO; dP = dO V^T; dS = scale P o (dP - rowsum(P o dP)); dQ = dS K; dK = dS^T Q"""
    qh, kh, p = _probs(c, inp)
    vh, doh = to_heads(inp["v"], c["H"]), to_heads(inp["dout"], c["H"])
    dp = doh @ vh.transpose(0, 1, 3, 2)
    ds = c["scale"] * p * (dp - (p * dp).sum(-1, keepdims=True))
    return dict(dq=from_heads(ds @ kh), dk=from_heads(ds.transpose(0, 1, 3, 2) @ qh), dv=from_heads(p.transpose(0, 1, 3, 2) @ doh))


def xattn_known_answers(c, inp):
    """what a known-answer case must return EXACTLY, in float32 before the rounding to the I/O type: out rows (NaN where the row is one of
    zeros: those are held to the ordinary limits only) for the forward; dv for the backward of an "onehot" case (dq = dk = 0)"""
    B, L, H, n = c["B"], c["L"], c["H"], c["n_ctx"]
    j = onehot_choice(c)
    v = inp["v"].reshape(B, n, H, D)
    bb, tt, hh = np.nonzero(j >= 0)
    out = np.full((B, L, H, D), np.nan, np.float32)
    out[bb, tt, hh] = v[bb, j[bb, tt, hh], hh]
    ans = dict(out=out.reshape(B, L, H * D), chosen=j)
    if "dout" in inp:
        dv = np.zeros((B, n, H, D), np.float32)
        np.add.at(dv, (bb, j[bb, tt, hh], hh), inp["dout"].reshape(B, L, H, D)[bb, tt, hh])      # (exact: multiples of 1/8)
        ans["dv"] = dv.reshape(B, n, H * D)
    return ans


def nctx1_worst(c, inp, dq, dk, bound):
    """n_ctx = 1: the probabilities are 1, dS = P o (dP - delta) cancels exactly and the float64 dq, dk are identically zero, so a relative
    limit means nothing.  Per token and head |dq[t]| <= bound scale |dout[t]| |v0| |k0|, per head |dk| <= bound scale sum_t |dout[t]| |v0| |q[t]|:
    the right-hand sides are the sizes of the terms that cancel.  Returns the worst (|dq| / rhs, |dk| / rhs), to be <= 1."""
    H = c["H"]
    nrm = lambda a: np.linalg.norm(np.asarray(a, np.float64).reshape(a.shape[0], a.shape[1], H, D), axis=-1)         # (B, n, H)
    ndo, nq, nk, nv = nrm(inp["dout"]), nrm(inp["q"]), nrm(inp["k"]), nrm(inp["v"])
    rq = bound * c["scale"] * ndo * nv * nk                                   # (B, L, H) by broadcasting the one key
    rk = bound * c["scale"] * (ndo * nq).sum(1, keepdims=True) * nv           # (B, 1, H)
    return float(np.max(nrm(dq) / np.maximum(rq, 1e-300))), float(np.max(nrm(dk) / np.maximum(rk, 1e-300)))


def xattn_model(c, q, k, v, dout=None):
    """The rounding model: the repository's plain compositions of the same operations (library GEMMs and ATen ops, P and dS rounded to the I/O
    type where the kernels round them; no HIP kernel of the project), on torch tensors of the case's I/O type on any device."""
    from zigma_amd import attention
    if dout is None:
        return dict(out=attention._attention_math_plain(q, k, v, c["H"], c["scale"]))
    return dict(zip(("dq", "dk", "dv"), attention.cross_attn_bwd_math(q, k, v, dout, c["H"], c["scale"])))


# ---------------------------------------------------------------------------------------------------
# glue backward
# ---------------------------------------------------------------------------------------------------
GLUE_L = (64, 128, 192, 1088)
GLUE_COLS = (128, 256, 640, 768, 8192)
GLUE_SLICE = 64                     # columns in front of a / dy in their wider buffers


def glue_cases():
    """18 cases, bf16.  Keys: B, L, cols, s_add (0 | 1), want_out, want_sum, a_slice / dy_slice (columns 64.. of a NaN-filled (B, L, 64 + cols)
    buffer), twice, seed; s is always the middle third of a NaN-filled (B, 3 cols) buffer."""
    out = []

    def add(**kw):
        c = dict(kernel="glue", twice=False)
        c.update(kw)
        c["seed"] = 13000 + len(out)
        c["id"] = (f"b{c['B']}-L{c['L']}-c{c['cols']}-add{c['s_add']}-{'o' if c['want_out'] else ''}{'s' if c['want_sum'] else ''}"
                   + ("-a" if c["a_slice"] else "") + ("-d" if c["dy_slice"] else ""))
        out.append(c)

    for i, (L, cols) in enumerate((L, cc) for L in GLUE_L for cc in GLUE_COLS[:4]):
        add(B=1 + i % 3, L=L, cols=cols, s_add=(i + i // 4) % 2, want_out=i % 4 != 2, want_sum=bool((i // 2 + i // 8) % 2), a_slice=i % 2 == 0,
            dy_slice=(i // 2) % 2 == 0, twice=i == 13)
    add(B=1, L=64, cols=8192, s_add=1, want_out=True, want_sum=True, a_slice=True, dy_slice=False)
    add(B=1, L=64, cols=8192, s_add=0, want_out=False, want_sum=False, a_slice=False, dy_slice=True)
    return out


# shapes / types zigma_scale_reduce_bwd refuses: glue_bwd_eligible is False and the entry point raises
GLUE_REFUSALS = (dict(id="L-100", B=2, L=100, cols=128, kind="bf16"), dict(id="cols-192", B=2, L=64, cols=192, kind="bf16"),
                 dict(id="cols-8320", B=1, L=64, cols=8320, kind="bf16"), dict(id="fp16", B=2, L=64, cols=128, kind="f16"))


def glue_inputs(c):
    rng = np.random.default_rng(c["seed"])
    r = lambda *s: round_to(rng.standard_normal(s), "bf16")
    return dict(dy=r(c["B"], c["L"], c["cols"]), a=r(c["B"], c["L"], c["cols"]), s=r(c["B"], c["cols"]))


def glue_reference(c, inp):
    """out = dy (s + s_add);  r1 = sum_L dy a;  r2 = sum_L dy     (include/zigma_hip.h, zigma_scale_reduce_bwd)"""
    dy, a, s = (np.asarray(inp[k], np.float64) for k in ("dy", "a", "s"))
    return dict(out=dy * (s[:, None] + c["s_add"]) if c["want_out"] else None, r1=(dy * a).sum(1), r2=dy.sum(1) if c["want_sum"] else None)


def glue_worst(key, got, ref, bound):
    """out row by row, the reduced sums element by element"""
    return rowwise_worst(got, ref, bound) if key == "out" else elementwise_worst(got, ref, bound)
