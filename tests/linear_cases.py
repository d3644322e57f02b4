"""Case tables of the sweep of the dense projection kernels: the four families behind zigma_linear_fwd — linear_tn_kernel (csrc/linear.hip, "tn":
8 waves), linear4w_kernel (csrc/linear4w.hip, "4w"), linear_ws_kernel (csrc/linear_ws.hip, "ws"), linear_sm_kernel (csrc/linear_sm.hip, "sm") — and
norm_linear_kernel (csrc/norm_linear.hip, "nl") behind zigma_norm_linear_fwd.

Plain numpy, importable without a GPU.  Seeded generators — linear_cases(), norm_linear_cases(), production_cases() — yield dicts of PARAMETERS with
stable ids; inputs(case) makes the numbers from the case's seed, already rounded to the case's I/O type; reference(case, inputs) evaluates in float64
on those rounded operands (dt=np.float32: the rounding model — fp32 accumulation over k in the kernels' 64-wide k-step order, fp32 epilogue, one
output rounding).  fields(case) is the parameter block the GPU test fills (every operand a window of a NaN-filled buffer: byte offset into its
allocation, row pitch); plan(case) restates plan_linear() / plan_norm_linear() on it and names the kernel string and the template instantiation
("leaf") that must serve the case.  tests/test_linear_cases_cpu.py holds plan() against the plans compiled with g++, checks coverage, the
references against float64 torch restatements and the rounding model; tests/test_gpu_linear_sweep.py runs the kernels.

Where the reference rounds: only where the ABI defines a 16-bit intermediate —
  * the gated residual of the 8-wave, the few-token and the unfused forms: out = residual + gate * r16(x w^T + bias);
  * norm_linear: y = r16(LayerNorm(x)), xa = r16(y (1 + scale) + shift), out = xa w^T.
The 4-wave kernel's gated epilogue (EPI 2 / 3) has NO intermediate rounding: it computes residual + gate * (x w^T + bias) from the fp32 accumulator,
and its reference does not round there either.  SiLU acts on the fp32 value before the single output rounding in every family.

Limits: the project's own (fwd_fuzz_cases: IO_BOUND norm-wise against the UNROUNDED reference, rowwise_worst <= ROW_GUARD for EVERY output row —
a gated row over |residual row| + |gate * v row|, every other row over its own norm floored by the rms row norm — DELTA_FLIPS for the element-wise
look at norm_linear's intermediate).  No case runs on a raised bound; a case whose own rounded reference missed a limit would get another seed and
be listed in SEED_MOVED (none needed one: the smallest output row here has 128 elements).
"""
import numpy as np

from bwd_fuzz_cases import ROW_GUARD, round_to, rowwise_worst  # noqa: F401  (re-exported)
from fwd_fuzz_cases import DELTA_FLIPS, IO_BOUND, flipped_share, need, norm_err, row_ratio  # noqa: F401

KINDS = ("bf16", "f16")
DTYPE_ID = {"f16": 1, "bf16": 2}                    # include/zigma_hip.h
REGIMES = ("benign", "model", "edges")
NL_REGIMES = ("benign", "rowscale", "edges")
WS, SM, PIN, NARROW, TWO_STAGE = 0x4000, 0x8000, 0x2000, 0x1000, 0x800       # flags: selectors; the 8-wave kernel, its 256 x 128 tile, two stages on it
SEED_MOVED = {}                                     # (kernel, id) -> seed
GATE_WINDOW = 5                                     # gate: column window 5 of the (batch, 6 n) modulation buffer; shift / scale: windows 3 / 4 of (batch, 6 k)
SHIFT_WINDOW, SCALE_WINDOW = 3, 4
NL_EPS = 1e-6
LEAD = 8                                            # NaN elements in front of every row (16 bytes) unless the case says otherwise
F16_LIMIT = 6e4


# ---------------------------------------------------------------------------------------------------
# layout and plan
# ---------------------------------------------------------------------------------------------------
def fields(c):
    """the parameter block of the case as the GPU test builds it: integer fields, and per operand `off` (bytes from a 256-byte aligned allocation to
    the first element) and `shape` (rows, cols, lead, pitch in elements) of its NaN-filled buffer"""
    m, n, k = c["m"], c["n"], c["k"]
    if c["kernel"] == "nl":
        nb = 1 if c["bcast"] else m // c["rpb"]
        sh = dict(x=(m, k, LEAD, LEAD + k + c["x_pad"]), w=(n, k, LEAD, LEAD + k + c["w_pad"]), out=(m, n, LEAD, LEAD + n + c["out_pad"]),
                  mod=(nb, 6 * k, LEAD, LEAD + 6 * k + 8))
        f = dict(m=m, n=n, k=k, dtype=DTYPE_ID[c["kind"]], flags=0, rows_per_batch=c["rpb"], eps=NL_EPS, x_row_stride=sh["x"][3], w_row_stride=sh["w"][3],
                 out_row_stride=sh["out"][3], mod_batch_stride=0 if c["bcast"] else sh["mod"][3])
        off = dict(x=2 * LEAD, w=2 * LEAD, out=2 * LEAD, shift=2 * (LEAD + SHIFT_WINDOW * k), scale=2 * (LEAD + SCALE_WINDOW * k))
        return dict(f, off=off, shape=sh)
    sh = dict(x=(m, k, LEAD, LEAD + k + c["x_pad"]), w=(n, k, LEAD, LEAD + k + 8), out=(m, n, c["out_lead"], c["out_lead"] + n + c["out_pad"]))
    f = dict(m=m, n=n, k=k, dtype=DTYPE_ID[c["kind"]], flags=c["flags"], silu_from_col=c["silu"], x_row_stride=sh["x"][3], w_row_stride=sh["w"][3],
             out_row_stride=sh["out"][3], res_row_stride=0, gate_batch_stride=0, rows_per_batch=0)
    off = dict(x=2 * LEAD, w=2 * LEAD, out=2 * c["out_lead"], bias=None, residual=None, gate=None)
    if c["bias"]:
        sh["bias"] = (1, n, c["bias_lead"], c["bias_lead"] + n + 8)
        off["bias"] = 2 * c["bias_lead"]
    if c["rpb"]:
        sh["residual"] = (m, n, c["out_lead"], c["out_lead"] + n + c["res_pad"])
        sh["mod"] = (m // c["rpb"], 6 * n, LEAD, LEAD + 6 * n + 8)
        off["residual"], off["gate"] = 2 * c["out_lead"], 2 * (LEAD + GATE_WINDOW * n)
        f.update(res_row_stride=sh["residual"][3], gate_batch_stride=sh["mod"][3], rows_per_batch=c["rpb"])
    return dict(f, off=off, shape=sh)


def _variant4w(f):
    o, m, n, k = f["off"], f["m"], f["n"], f["k"]
    if f["flags"] or f["silu_from_col"] < n or m % 256 or n % 128 or k % 64 or k < 192:
        return -1
    if f["out_row_stride"] % 8 or o["out"] % 16 or m * f["out_row_stride"] * 2 > 0xffffffff:
        return -1
    tiles_n = -(-n // 256)
    if (m // 256) * tiles_n < 256 or tiles_n > 1023:
        return -1
    epi = 1 if n % 256 else 0
    if o["residual"] is not None:
        rpb = f["rows_per_batch"]
        if f["res_row_stride"] != f["out_row_stride"] or f["out_row_stride"] % 128 or rpb < 128 or rpb & (rpb - 1) or m % rpb:
            return -1
        if o["residual"] % 16 or o["gate"] % 16 or f["gate_batch_stride"] % 8:
            return -1
        epi = 2
    if o["bias"] is not None:
        if o["residual"] is None or n > 8192 or o["bias"] % 2:
            return -1
        epi = 3
    return epi


def plan(c):
    """plan_linear() / plan_norm_linear() restated on fields(c) -> dict(family, kernel, leaf); every case of the tables is served (asserted)"""
    f = fields(c)
    o, m, n, k = f["off"], f["m"], f["n"], f["k"]
    assert m > 0 and f["x_row_stride"] % 8 == 0 and f["w_row_stride"] % 8 == 0 and o["x"] % 16 == 0 and o["w"] % 16 == 0
    if c["kernel"] == "nl":
        assert n == 512 and k in (512, 640, 768) and m % 128 == 0 and m % f["rows_per_batch"] == 0 and f["out_row_stride"] % 8 == 0
        assert f["mod_batch_stride"] % 8 == 0 and all(o[a] % 16 == 0 for a in ("out", "shift", "scale"))
        return dict(family="nl", kernel=f"norm_linear_k{k}", leaf=f"nl<{k // 64}>")
    flags, silu = f["flags"], f["silu_from_col"]
    assert k % 64 == 0 and n % 128 == 0 and m % 8 == 0 and silu % 32 == 0 and 0 <= silu and f["out_row_stride"] % 4 == 0 and o["out"] % 8 == 0
    res, bias = o["residual"] is not None, o["bias"] is not None
    if res:
        assert f["rows_per_batch"] % 256 == 0 and m % f["rows_per_batch"] == 0 and f["res_row_stride"] % 8 == 0 and f["gate_batch_stride"] % 8 == 0
        assert o["residual"] % 16 == 0 and o["gate"] % 16 == 0
    assert not bias or (n <= 4096 and o["bias"] % 4 == 0)
    st16 = f["out_row_stride"] % 8 == 0 and o["out"] % 16 == 0
    if flags & WS:
        narrow = k in (1280, 1536)
        pw = 128 if narrow else 256
        assert not bias and not res and (narrow or k in (512, 640)) and (silu >= n or (not narrow and silu % 128 == 0))
        panels = n // pw
        assert n % pw == 0 and n <= 8192 and m % 512 == 0 and st16 and panels <= 32 and m // 512 >= 32 // panels and f["x_row_stride"] % 128 == 0
        sl = silu < n
        return dict(family="ws", kernel="linear_ws_silu" if sl else "linear_ws_128" if narrow else "linear_ws", leaf=f"ws<{k // 16},{int(sl)}>",
                    panels=panels, ranges=32 // panels, tiles_per_xcd=m // 512)
    if flags & SM:
        assert silu >= n and k >= 128 and m % 128 == 0 and st16 and (not bias or o["bias"] % 8 == 0)
        nblk = 5 if n % 160 == 0 else 6 if n % 192 == 0 else 4
        return dict(family="sm", kernel=f"linear_sm_128x{32 * nblk}", leaf=f"sm<{nblk},{int(bias or res)}>")
    epi = _variant4w(f)
    if epi >= 0:
        return dict(family="4w", kernel="linear4w_256x256+128" if n % 256 else "linear4w_256x256", leaf=f"4w<{epi}>")
    wide = n % 256 == 0 and not flags & NARROW and not res
    stages = 2 if wide or flags & TWO_STAGE else 3
    assert not (res and stages == 2), "the two-stage probe form has no gated epilogue"
    tiles = -(-m // 256) * (n // (256 if wide else 128))
    return dict(family="tn", kernel="linear_tn_256x256" if wide else "linear_tn_256x128", leaf=f"tn<{4 if wide else 2},{stages},{int(bias)},{int(res)}>",
                tiles=tiles, grid=256 if tiles >= 256 else -(-tiles // 8) * 8)


TN_LEAVES = tuple(f"tn<{w},{s},{b},{r}>" for w, s, r in ((4, 2, 0), (2, 2, 0), (2, 3, 0), (2, 3, 1)) for b in (0, 1))
LEAVES = (TN_LEAVES + tuple(f"4w<{e}>" for e in range(4)) + tuple(f"ws<{g},0>" for g in (32, 40, 80, 96)) + ("ws<32,1>", "ws<40,1>")
          + tuple(f"sm<{b},{e}>" for b in (4, 5, 6) for e in (0, 1)))
NL_LEAVES = ("nl<8>", "nl<10>", "nl<12>")


# ---------------------------------------------------------------------------------------------------
# zigma_linear_fwd: the case table
# ---------------------------------------------------------------------------------------------------
def _case(table, want, **kw):
    """want: the family the case is meant for (asserted against plan())"""
    c = dict(kernel="lin", kind="bf16", flags=0, bias=False, bias_lead=LEAD, silu=None, rpb=0, x_pad=8, out_lead=LEAD, out_pad=8, res_pad=24, regime="benign",
             known=None, seed=31000 + len(table))
    c.update(kw)
    c["silu"] = c["n"] if c["silu"] is None else c["silu"]
    if want == "ws":
        c["flags"] |= WS
        c["x_pad"] = 120 if (LEAD + c["x_pad"]) % 128 else c["x_pad"]      # pitch = LEAD + k + x_pad: a multiple of 128
    if want == "sm":
        c["flags"] |= SM
    if want == "4w" and c["rpb"]:
        c["out_pad"] = c["res_pad"] = 120                                    # pitch n + 128, the residual rows in the output's pitch
    p = plan(c)
    assert p["family"] == want, (want, p, c)
    c.update(family=p["family"], kernel_name=p["kernel"], leaf=p["leaf"])
    c["id"] = (f"{want}-{c['kind']}-{c['m']}x{c['n']}x{c['k']}" + (f"-f{c['flags'] & 0x3800:x}" if c["flags"] & 0x3800 else "") + ("-b" if c["bias"] else "")
               + (f"{c['bias_lead']}" if c["bias"] and c["bias_lead"] != LEAD else "") + (f"-s{c['silu']}" if c["silu"] < c["n"] else "")
               + (f"-r{c['rpb']}" if c["rpb"] else "") + f"-x{c['x_pad']}o{c['out_lead']}+{c['out_pad']}-{c['known'] or c['regime']}")
    c["seed"] = SEED_MOVED.get(("lin", c["id"]), c["seed"])
    table.append(c)
    return c


def linear_cases():
    """Keys: kind, m, n, k, flags, bias, bias_lead (elements between the bias and its 256-byte aligned allocation), silu (silu_from_col; n: none), rpb
    (rows_per_batch of the gated residual; 0: none), x_pad / out_pad / res_pad (elements a row pitch exceeds lead + row), out_lead, regime, known
    (None | "select" | "ints": bit for bit), family, kernel_name, leaf, seed."""
    t, i = [], 0

    def nxt():
        nonlocal i
        i += 1
        return dict(kind=KINDS[i % 2], regime=REGIMES[(i + i // 2) % 3])
    # ---- 8 waves.  k-steps 1 ... 5 on the three-stage, the gated and the two-stage wide form (g_total below, at and above NST - 1), both types
    for k in (64, 128, 192, 256, 320):
        for kind in KINDS:
            _case(t, "tn", m=264, n=128, k=k, **dict(nxt(), kind=kind))
            _case(t, "tn", m=512, n=256, k=k, rpb=256, bias=k % 128 == 0, **dict(nxt(), kind=kind))
            _case(t, "tn", m=264, n=256, k=k, flags=PIN, **dict(nxt(), kind=kind))
            _case(t, "tn", m=264, n=256, k=k, flags=PIN | NARROW | TWO_STAGE, bias=k % 128 != 0, **dict(nxt(), kind=kind))
    for m in (8, 16, 248, 256, 264, 504, 1040):     # one group of eight, ragged last tiles, a wave without rows
        _case(t, "tn", m=m, n=384, k=192, bias=m % 16 == 8, **nxt())
        _case(t, "tn", m=m, n=512, k=192, flags=PIN, **nxt())
    for m, n, fl, known in ((4352, 4096, 0, "select"), (4344, 4096, 0, None), (4352, 2048, PIN | NARROW, "ints"), (4344, 2048, PIN | NARROW, None)):
        _case(t, "tn", m=m, n=n, k=128, flags=fl, known=known, bias=known == "ints", **nxt())          # 272 tiles on 256 workgroups
    for m, n in ((8, 128), (520, 128), (520, 384)):                          # 1, 3 and 9 tiles: grids of 8, 8 and 16 with idle workgroups
        _case(t, "tn", m=m, n=n, k=128, **nxt())
    for n, fl in ((128, 0), (4096, PIN), (4096, PIN | NARROW)):              # the bias staging: 256 bytes and its full 8 KB; a 4-byte boundary
        _case(t, "tn", m=264, n=n, k=128, flags=fl, bias=True, **nxt())
        _case(t, "tn", m=264, n=n, k=128, flags=fl, bias=True, bias_lead=2, **nxt())
    for s in (0, 32, 96, 224, 256):                                          # SiLU per 32-feature block
        _case(t, "tn", m=264, n=256, k=128, silu=s, bias=s in (32, 224), **dict(nxt(), regime="edges"))
        _case(t, "tn", m=264, n=256, k=128, silu=s, flags=PIN | NARROW, bias=s == 96, **nxt())
    for n, fl in ((256, 0), (384, 0), (256, PIN | NARROW | TWO_STAGE)):      # out 8 bytes into its allocation, pitch % 8 == 4
        _case(t, "tn", m=264, n=n, k=192, flags=fl, out_lead=4, out_pad=8, **nxt())
    for rpb, nb in ((256, 5), (256, 3), (512, 2), (768, 1), (512, 4), (768, 2)):
        for bias in (False, True):
            _case(t, "tn", m=rpb * nb, n=(256, 384)[nb % 2], k=128, rpb=rpb, bias=bias, **nxt())
    for kind in KINDS:                                                       # known answers per instantiation group
        for known in ("select", "ints"):
            ints = known == "ints"
            _case(t, "tn", m=520, n=512, k=320, flags=PIN, known=known, bias=ints, kind=kind)
            _case(t, "tn", m=520, n=384, k=320, known=known, bias=ints, kind=kind)
            _case(t, "tn", m=512, n=384, k=320, rpb=256, known=known, bias=ints, kind=kind)
            _case(t, "tn", m=520, n=384, k=320, flags=PIN | TWO_STAGE, known=known, bias=ints, kind=kind)
    # ---- 4 waves: exactly 256 tiles and 288 (some workgroups get two), a narrow tile column, odd and even k-step counts, EPI 0 ... 3
    for m, n, k, rpb, bias, known in ((2048, 8192, 192, 0, False, None), (2304, 8192, 256, 0, False, "select"), (2048, 8064, 320, 0, False, None),
                                     (2304, 8064, 448, 0, False, "ints"), (2048, 8192, 256, 256, False, None), (2304, 8192, 192, 256, False, None),
                                     (2048, 8192, 448, 512, False, None), (2048, 8192, 320, 2048, False, None), (2304, 8192, 320, 256, False, "ints"),
                                     (2048, 8064, 192, 512, False, "select"), (4096, 4096, 192, 256, True, None), (4096, 4096, 320, 2048, True, None),
                                     (4352, 4096, 256, 256, True, "ints"), (4096, 3968, 448, 512, True, None)):
        _case(t, "4w", m=m, n=n, k=k, rpb=rpb, bias=bias, known=known, **nxt())
    # the 4-wave kernel's neighbours: 255 tiles, k = 128, a bias alone, a residual whose pitch is no multiple of 128 -> the 8-wave kernel
    _case(t, "tn", m=3840, n=4352, k=192, **nxt())
    _case(t, "tn", m=2048, n=8192, k=128, **nxt())
    _case(t, "tn", m=4096, n=4096, k=192, bias=True, **nxt())
    _case(t, "tn", m=2048, n=8192, k=192, rpb=256, out_pad=8, res_pad=8, **nxt())
    # ---- weight-stationary: panel extremes, odd / even tiles per workgroup, SiLU off the panel edge, x pitches k + 128 / k + 256
    for m, n, k, s, xp, known in ((512, 8192, 512, None, 120, None), (16384, 256, 640, None, 248, None), (512, 4096, 1280, None, 120, None),
                                  (16384, 128, 1536, None, 248, None), (512 * 33, 256, 512, None, 120, "select"), (512 * 43, 256, 640, None, 248, None),
                                  (512 * 65, 256, 512, None, 120, None), (2048, 2048, 640, None, 120, None), (2560, 2048, 512, None, 248, "ints"),
                                  (4608, 2048, 640, None, 120, "select"), (8192, 512, 640, 0, 120, None), (8192, 512, 512, 128, 248, None),
                                  (8192, 512, 640, 384, 120, None), (8704, 512, 512, 384, 120, None), (2560, 2048, 640, 1024, 248, "select"),
                                  (512 * 33, 128, 1280, None, 248, "ints"), (2560, 1024, 1536, None, 120, "select"), (4608, 1024, 1280, None, 120, None)):
        _case(t, "ws", m=m, n=n, k=k, silu=s, x_pad=xp, known=known, **dict(nxt(), **({"regime": "edges"} if s is not None and not known else {})))
    # ---- few tokens: NBLK 4 / 5 / 6, 2 ... 5 k-steps and 24, every epilogue form
    j = 0
    for n in (128, 384, 640, 768, 1920):
        for k in (128, 192, 256, 320, 1536):
            m = (128, 256, 384)[j % 3]
            form = j % 4 if m == 256 else (0, 1)[j % 2]                       # plain | bias | gated | both
            _case(t, "sm", m=m, n=n, k=k, bias=form in (1, 3), rpb=256 if form >= 2 else 0, bias_lead=(LEAD, 4)[j % 2], **nxt())
            j += 1
    for kind in KINDS:
        _case(t, "sm", m=768, n=640, k=192, rpb=256, bias=True, bias_lead=4, kind=kind, regime="model")          # three samples
        _case(t, "sm", m=768, n=384, k=256, rpb=256, kind=kind, regime="edges")
        _case(t, "sm", m=384, n=640, k=320, known="select", kind=kind)
        _case(t, "sm", m=768, n=768, k=192, rpb=256, bias=True, known="ints", kind=kind)
        _case(t, "sm", m=256, n=128, k=1536, rpb=256, known="select", kind=kind)
    # ---- every leaf in both types, every form in three regimes: what the walks above left out, at the family's smallest shape
    small = {"tn<4,2,0,0>": dict(m=264, n=256, k=128), "tn<4,2,1,0>": dict(m=264, n=256, k=128, bias=True), "tn<2,2,0,0>": dict(m=264, n=128, k=128, flags=PIN | TWO_STAGE),
             "tn<2,2,1,0>": dict(m=264, n=128, k=128, flags=PIN | TWO_STAGE, bias=True), "tn<2,3,0,0>": dict(m=264, n=128, k=128),
             "tn<2,3,1,0>": dict(m=264, n=128, k=128, bias=True), "tn<2,3,0,1>": dict(m=512, n=128, k=128, rpb=256),
             "tn<2,3,1,1>": dict(m=512, n=128, k=128, rpb=256, bias=True), "4w<0>": dict(m=2048, n=8192, k=192), "4w<1>": dict(m=2048, n=8064, k=192),
             "4w<2>": dict(m=2048, n=8192, k=192, rpb=512), "4w<3>": dict(m=4096, n=4096, k=192, rpb=512, bias=True),
             "ws<32,0>": dict(m=2048, n=2048, k=512), "ws<40,0>": dict(m=2048, n=2048, k=640), "ws<80,0>": dict(m=2048, n=1024, k=1280),
             "ws<96,0>": dict(m=2048, n=1024, k=1536), "ws<32,1>": dict(m=2048, n=2048, k=512, silu=1152), "ws<40,1>": dict(m=2048, n=2048, k=640, silu=1152),
             "sm<4,0>": dict(m=128, n=128, k=128), "sm<4,1>": dict(m=256, n=128, k=128, rpb=256), "sm<5,0>": dict(m=128, n=160 * 4, k=128),
             "sm<5,1>": dict(m=128, n=640, k=128, bias=True), "sm<6,0>": dict(m=128, n=384, k=128), "sm<6,1>": dict(m=256, n=384, k=128, rpb=256, bias=True)}
    for li, leaf in enumerate(LEAVES):
        mine = lambda: [c for c in t if c["leaf"] == leaf and not c["known"]]
        for ki, kind in enumerate(KINDS):
            if not any(c["kind"] == kind for c in mine()):
                _case(t, leaf[:2], kind=kind, regime=REGIMES[(li + ki) % 3], **small[leaf])
        for ri, regime in enumerate(REGIMES):
            if not any(c["regime"] == regime for c in mine()):
                _case(t, leaf[:2], kind=KINDS[(li + ri) % 2], regime=regime, **small[leaf])
    return t


def production_cases():
    """the shapes of the shipped model at 65 536 tokens (8192 for the few-token kernel), bf16"""
    t = []
    _case(t, "ws", m=65536, n=2560, k=640, silu=1280, x_pad=120, seed=36000)                   # in_proj
    _case(t, "4w", m=65536, n=640, k=1280, rpb=1024, seed=36001)                               # out_proj, EPI 2
    _case(t, "4w", m=65536, n=640, k=512, rpb=1024, bias=True, seed=36002)                     # to_out, EPI 3
    _case(t, "sm", m=8192, n=640, k=1280, seed=36003)                                          # out_proj below the tiled kernel's token floor
    _nl_case(t, m=65536, k=640, rpb=1024, seed=36004)
    for c in t:
        c["production"] = True
    return t


# ---------------------------------------------------------------------------------------------------
# zigma_norm_linear_fwd: the case table
# ---------------------------------------------------------------------------------------------------
def _nl_case(table, **kw):
    c = dict(kernel="nl", kind="bf16", n=512, bcast=False, x_pad=0, w_pad=0, out_pad=0, regime="benign", known=None, seed=34000 + len(table))
    c.update(kw)
    p = plan(c)
    c.update(family="nl", kernel_name=p["kernel"], leaf=p["leaf"])
    c["id"] = (f"nl-{c['kind']}-{c['m']}x{c['k']}-r{c['rpb']}" + ("-bc" if c["bcast"] else "") + f"-x{c['x_pad']}w{c['w_pad']}o{c['out_pad']}-{c['known'] or c['regime']}")
    c["seed"] = SEED_MOVED.get(("nl", c["id"]), c["seed"])
    table.append(c)
    return c


def norm_linear_cases():
    """Keys: kind, m, k, n (512), rpb (rows_per_batch), bcast (mod_batch_stride 0: every sample reads one shift / scale row; else the pitch of the
    (batch, 6 k) buffer), x_pad / w_pad / out_pad, regime (NL_REGIMES), known (None | "select": the weight shows the hidden intermediate), seed"""
    t, i = [], 0
    for k in (512, 640, 768):
        for m in (128, 256, 384):
            for rpb in (m, 128, 96, 32, 1):
                if m % rpb or (rpb == 128 and m == 128):
                    continue
                pads = ((0, 0, 0), (640, 8, 512), (8, 136, 8))[i % 3]
                _nl_case(t, m=m, k=k, rpb=rpb, kind=KINDS[i % 2], bcast=i % 4 == 3, x_pad=pads[0], w_pad=pads[1], out_pad=pads[2], regime=NL_REGIMES[(i + i // 2) % 3])
                i += 1
    for k in (512, 640, 768):
        for kind in KINDS:
            for part in (0, 1):          # selection weights: features 0 ... 511 of xa, then the last 512
                _nl_case(t, m=256, k=k, rpb=(128, 32)[part], kind=kind, known="select", part=part, regime=NL_REGIMES[(part + k // 128) % 3],
                         x_pad=8 * part, out_pad=8 * part)
            for regime in NL_REGIMES:
                if not any(c["k"] == k and c["kind"] == kind and c["regime"] == regime and not c["known"] for c in t):
                    _nl_case(t, m=128, k=k, rpb=32, kind=kind, regime=regime)
    return t


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
SELECT_C = np.array([1.0, -1.0, 2.0, -2.0, 0.5])
GATE_C = np.array([1.0, -1.0, 2.0, -2.0, 0.5])


def select_weight(rng, n, k, unit=False, start=0):
    """(n, k): row j = c_j e_pi(j); pi runs through seeded permutations of [0, k), so it is onto [0, k) wherever n >= k"""
    pi = np.concatenate([rng.permutation(k) for _ in range(-(-n // k))])[:n] if not unit else (start + np.arange(n)) % k
    cj = np.ones(n) if unit else SELECT_C[rng.integers(0, 5, n)]
    w = np.zeros((n, k), np.float32)
    w[np.arange(n), pi] = cj
    return w, pi, cj


def wide_range(rng, m, k):
    """distinct rows of large and tiny values, +-(1 + u) 2^e with e in [-8, 8]: halves and doubles of them are exact in both 16-bit types"""
    return (rng.choice([-1.0, 1.0], (m, k)) * (1.0 + rng.random((m, k))) * 2.0 ** rng.integers(-8, 9, (m, k))).astype(np.float32)


def edge_rows(m):
    """rows the `edges` regime rewrites: zero, cancelling, subnormal, mean 4, pre-activation spikes"""
    r = dict(zero=[1], cancel=[3], tiny=[4], mean=[5], spike=[(6, 12.0), (7, 30.0)])
    if m >= 16:
        r["zero"].append(m - 1)
        r["cancel"].append(m // 2)
        r["spike"].append((m - 2, 100.0))
    return r


def inputs(c):
    """-> dict(x (m, k), w (n, k), bias (n) | None, res (m, n) | None, gate (m / rpb, n) | None), float32 arrays holding values of the case's type"""
    if c["kernel"] == "nl":
        return nl_inputs(c)
    rng = np.random.default_rng(c["seed"])
    m, n, k, kind, nb = c["m"], c["n"], c["k"], c["kind"], (c["m"] // c["rpb"] if c["rpb"] else 0)
    rn = lambda *s: rng.standard_normal(s, dtype=np.float32)
    if c["known"] == "select":
        x, (w, _, _) = wide_range(rng, m, k), select_weight(rng, n, k)
        return dict(x=round_to(x, kind), w=w, bias=None, res=round_to(wide_range(rng, m, n), kind) if nb else None,
                    gate=GATE_C[rng.integers(0, 5, (nb, n))].astype(np.float32) if nb else None)
    if c["known"] == "ints":        # x in -4 ... 4; <= 8 weights of +-1 / +-2 per feature, one in the first and one in the last k-step: |sum| <= 64
        x = rng.integers(-4, 5, (m, k)).astype(np.float32)
        w = np.zeros((n, k), np.float32)
        cols = np.concatenate([rng.integers(0, 64, (n, 1)), rng.integers(k - 64, k, (n, 1)), rng.integers(0, k, (n, 6))], 1)
        w[np.arange(n)[:, None], cols] = rng.choice([-2.0, -1.0, 1.0, 2.0], (n, 8))
        return dict(x=x, w=w, bias=rng.integers(-8, 9, n).astype(np.float32) if c["bias"] else None,
                    res=rng.integers(-8, 9, (m, n)).astype(np.float32) if nb else None, gate=GATE_C[rng.integers(0, 5, (nb, n))].astype(np.float32) if nb else None)
    model = c["regime"] == "model"
    x, w = rn(m, k), rn(n, k) * np.float32(k ** -0.5)
    if model:
        x /= np.sqrt(np.mean(x * x, -1, keepdims=True))
    bias = 0.3 * rn(n) if c["bias"] else None
    res = rn(m, n) * np.float32(30.0 if model else 1.0) if nb else None
    gate = (0.1 + 0.02 * rn(nb, n) if model else 0.5 * rn(nb, n)) if nb else None
    if c["regime"] == "edges":
        r, cc, h, sign = edge_rows(m), k - 1, k // 2, np.where(np.arange(n) % 2, 1.0, -1.0).astype(np.float32)
        for row, s in r["spike"]:                                               # with w[:, k - 1] = +-1: pre-activation values of +-12, +-30, +-100
            x[row] = 0.0
            x[row, cc] = s
        x[r["cancel"], h:] = x[r["cancel"], :h]
        if c["seed"] % 2 == 0:          # variant "cancel": every w row is (b | -b), so the rows (a | a) of x cancel in every feature
            w[:, h - 1] = -sign
            w[:, h:] = -w[:, :h]
        else:                           # variant "mean": a mean of 4 on a row of x and on four of w (smaller on w where fp16 does not hold 16 k)
            w[:, cc] = sign
            wm = 4.0
            while 4.0 * wm * k * (4.0 if nb else 1.0) > 3e4:
                wm /= 2.0
            x[r["mean"]] += 4.0
            w[20:24] += wm
        x[r["tiny"]] *= 2.0 ** -18                                              # fp16 subnormals
        w[5] *= 2.0 ** -18
        x[r["zero"]] = 0.0
        w[[2, n - 3]] = 0.0
        if nb:
            gate[:, :4], gate[:, n - 2:] = np.array([4.0, -4.0, 0.0, 4.0], np.float32), 0.0
    f = lambda a: None if a is None else round_to(a, kind)
    return dict(x=f(x), w=f(w), bias=f(bias), res=f(res), gate=f(gate))


def nl_inputs(c):
    """-> dict(x (m, k), w (512, k), shift, scale (batch | 1, k))"""
    rng = np.random.default_rng(c["seed"])
    m, n, k, kind = c["m"], c["n"], c["k"], c["kind"]
    nb = 1 if c["bcast"] else m // c["rpb"]
    rn = lambda *s: rng.standard_normal(s)
    x, w = rn(m, k) + 0.3, rn(n, k) * k ** -0.5
    shift, scale = 0.3 * rn(nb, k), 0.3 * rn(nb, k)
    if c["regime"] == "rowscale":           # mean up to +-8 standard deviations, standard deviations over two decades
        std = 10.0 ** (rng.random((m, 1)) * 2 - 1)
        x = (rng.random((m, 1)) * 16 - 8) * std + std * rn(m, k)
    if c["regime"] == "edges":
        for a in range(0, m, 32):           # in every wave's 32 rows: a constant row, mean 100 with spread 1, an all-zero row
            x[a + 1], x[a + 2], x[a + 3] = (2.5, -0.75)[(a // 32) % 2], 100.0 + rn(k), 0.0
        scale[:, :8] = -1.0                 # the modulate cancels y
        scale[:, 8:12], shift[:, 8:12] = np.array([4.0, -4.0, 4.0, -4.0]), np.array([4.0, 4.0, -4.0, -4.0])
    if c["known"] == "select":
        w = select_weight(rng, n, k, unit=True, start=c["part"] * (k - n))[0]
    f = lambda a: round_to(a, kind)
    return dict(x=f(x), w=f(w), shift=f(shift), scale=f(scale))


# ---------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------
def _product(x, w, dt):
    if dt is np.float64:
        return x.astype(dt) @ w.astype(dt).T
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)          # the kernels' order: one 64-wide k-step after the other into the fp32 accumulator
    for s in range(0, x.shape[1], 64):
        acc += x[:, s:s + 64].astype(np.float32) @ w[:, s:s + 64].astype(np.float32).T
    return acc


def _silu(v):
    with np.errstate(over="ignore"):
        return v / (1 + np.exp(-v))


def gate_rows(c, inp, dt=np.float64):
    return inp["gate"].astype(dt).repeat(c["rpb"], axis=0)


def reference(c, inp, dt=np.float64, rows=None):
    """-> dict(out, v: x w^T + bias after the activation, terms: (residual, gate * v) | None); UNROUNDED except the 16-bit intermediate of the gated
    forms outside the 4-wave kernel.  rows: a slice of the output rows."""
    if c["kernel"] == "nl":
        return nl_reference(c, inp, dt, rows)
    rows = slice(None) if rows is None else rows
    v = _product(inp["x"][rows], inp["w"], dt)
    if inp["bias"] is not None:
        v = v + inp["bias"].astype(dt)
    if c["silu"] < c["n"]:
        v[:, c["silu"]:] = _silu(v[:, c["silu"]:])
    if inp["res"] is None:
        return dict(out=v, v=v, terms=None)
    g, res = gate_rows(c, inp, dt)[rows], inp["res"][rows].astype(dt)
    p = v if c["family"] == "4w" else round_to(v.astype(np.float32), c["kind"]).astype(dt)
    return dict(out=res + g * p, v=v, terms=(res, g * v))


def gated_defined(c, inp, p16):
    """the ONE value out has given the kernel's own plain output p16 (8 waves, few tokens): r16(fl32(fma(gate, p16, residual))), evaluated in float64 —
    gate * p16 has at most 22 significant bits and the sum with the residual fits 53 unless their exponents lie more than 2^30 apart"""
    s = gate_rows(c, inp) * np.asarray(p16, np.float64) + inp["res"].astype(np.float64)
    return round_to(s.astype(np.float32), c["kind"])


def nl_reference(c, inp, dt=np.float64, rows=None):
    """-> dict(y, y_mod (unrounded second stage on the rounded y), xa = r16(y_mod), out, terms of y_mod, gain = 1 + scale per row)"""
    rows = slice(None) if rows is None else rows
    k, kind = c["k"], c["kind"]
    x = inp["x"][rows].astype(dt)
    pick = (lambda a: a.astype(dt).repeat(c["m"], axis=0)[rows]) if c["bcast"] else (lambda a: a.astype(dt).repeat(c["rpb"], axis=0)[rows])
    d = x - x.sum(-1, keepdims=True, dtype=dt) / dt(k)
    y = d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=dt) / dt(k) + dt(NL_EPS))
    a = round_to(y.astype(np.float32), kind).astype(dt) * (dt(1) + pick(inp["scale"]))
    y_mod = a + pick(inp["shift"])
    xa = round_to(y_mod.astype(np.float32), kind)
    return dict(y=y, y_mod=y_mod, xa=xa, out=_product(xa, inp["w"], dt), terms=(a, pick(inp["shift"])), v=None, gain=dt(1) + pick(inp["scale"]))


def ulp16(v, kind):
    """the spacing of the 16-bit type at |v| (normal values)"""
    bits, emin = (7, -126) if kind == "bf16" else (10, -14)
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** emin))) - bits)


def xa_allowance(ref, seen, kind):
    """how far an element of norm_linear's hidden intermediate may lie from the correctly rounded float64 value: ONE ulp at each of its two rounding
    points.  y is rounded first, so a y that fell the other way moves y (1 + scale) + shift by ulp(y) |1 + scale| — many ulps of the RESULT where
    the sum cancels — and the result is then rounded once more: ulp(y16) |1 + scale| + ulp(result)."""
    y16, want = round_to(ref["y"].astype(np.float32), kind).astype(np.float64), ref["xa"].astype(np.float64)
    return ulp16(y16, kind) * np.abs(ref["gain"]) + ulp16(np.maximum(np.abs(seen), np.abs(want)), kind)


def counts(cases):
    out = {}
    for c in cases:
        out[c["family"]] = out.get(c["family"], 0) + 1
    return out
