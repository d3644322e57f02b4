"""ONE routing table for every dense projection with a hand-written kernel.

    route(role, tokens, n, k) -> Route(kernel, fuse_add, row)

role   = which projection is asked for — it fixes the epilogue the call carries:
           "in_proj"  x @ W_in^T            (mamba_simple.py:290-294), no epilogue
           "out_proj" y @ W_out^T           (selective_scan_interface.py:365), optionally the block's gated add n + gate * (.)
           "to_q"     xa @ W_q^T            (model_zigma.py:104-106), no epilogue
           "to_out"   o @ W_o^T + bias      (model_zigma.py:128-135), bias + the block's gated add h + gate * (.)
           "text"     y_embedder and the batched to_k / to_v of all blocks (model_zigma.py:668, :104-112) on rows the caller padded to 256
           "train"    the forward product and dX = dY W of wgrad.LinearTrainFn (the training path of all four block projections)
kernel = which kernel family of zigma_linear_fwd serves it (KERNELS below), or "library" (F.linear = hipBLASLt) — every cell that falls
         to the library is an explicit row of the table or the explicit last row, and tests/test_host_cpu.py::test_routing_table sweeps
         E x tokens and compares the library cells with a reviewed list.
fuse_add = the caller hands the gated residual to the kernel's epilogue (True) or leaves it to the next norm kernel (False).

The table holds POLICY (what is fastest where, with the measurement that decided it).  The shape LIMITS of each kernel family are the library's:
serves(kernel, tokens, n, k) asks plan_linear() (csrc/linear_plan.h, where every refusal and kernel choice of zigma_linear_fwd lives; zigma_linear_fwd_plan)
about the canonical call of that shape — aligned contiguous bf16 operands, no bias, a fresh output — with that family's selector set, and reads the family
and panel width off the kernel it names.  So the table needs the built library, as the Mamba inner's plan does: without it route() raises _lib.lib()'s
"not built" error.  A row never returns a kernel whose limits the shape does not meet.  linear.plan walks candidates() and asks the library about the
call's own block (pointer / stride alignment, bias); a row it refuses there is counted in REFUSED and the walk goes on to the next row (never silent:
tests assert REFUSED stays empty on the shipped shapes).

Knobs (tools / tests; no environment variable of their own — ZIGMA_KNOBS="routing.POLICY=off,routing.DISABLED=in_proj.ws+to_q.sm"):
  POLICY    "auto" the table;  "all" every block projection the tiled kernels can serve runs on them (fused epilogues on; "text" and "train"
            as under "auto");  "off" library only, every role
  DISABLED  row ids skipped ("+"-separated string or a set): A/B of one row against what the table holds below it
"""
import functools
from collections import namedtuple

from . import _knobs, _lib

Route = namedtuple("Route", "kernel fuse_add row")
Row = namedtuple("Row", "id role k n tokens kernel fuse_add why")

KERNELS = ("ws", "ws128", "sm", "tiled", "tiled_halves", "split3", "split1", "library")
#   ws           csrc/linear_ws.hip, 256-feature weight panels resident in registers (k = 512 / 640)
#   ws128        the same kernel's 128-feature-panel form (k = 1280 / 1536)
#   sm           csrc/linear_sm.hip, one 128-token x n/4-feature tile per workgroup (few tokens)
#   tiled        zigma_linear_fwd's default: the generated 4-wave kernel (csrc/linear4w.hip) from 256 tiles on, the 8-wave kernel (csrc/linear.hip) below
#   tiled_halves two launches of `tiled`, one per half of the output columns
#   split3       csrc/linear_split.hip, fp32 operands as three bf16 products (fp32_matmul.PRECISION = "high"); never a row of the table: linear.plan
#                hands fp32 inference calls to it before the table is asked
#   split1       the same kernel with one pass ("medium")
#   library      F.linear

POLICY = "auto"
DISABLED = ""
INF = 1 << 40
REFUSED = []          # (role, tokens, n, k, kernel) of rows a call matched and the tensor-level check of linear.py turned down (the last 64 of them)


# ---- shape limits of the kernel families: the library's plan on the canonical call of a shape ----------------------------------------------------------
SELECTOR = {"ws": _lib.LINEAR_WS, "ws128": _lib.LINEAR_WS, "sm": _lib.LINEAR_SM, "tiled": 0}          # zigma_linear_params_t.flags of the one-launch families


@functools.lru_cache(maxsize=None)
def _canonical(flags, tokens, n, k, bias=False, residual=False):
    """the kernel plan_linear() serves the canonical call of this shape with (None: refused, or nothing to launch): bf16 rows at placeholder addresses, x
    and weight contiguous, a fresh output; bias / residual: the epilogue operands, the gated residual in the output's pitch on samples of the largest power
    of two of rows that divides the tokens.  Memoised: a pure function of its arguments, and the table is walked on every projection call."""
    P = _lib.LinearParams()
    P.m, P.n, P.k, P.dtype, P.flags, P.silu_from_col = tokens, n, k, _lib.BF16, flags, n
    P.x_row_stride, P.w_row_stride, P.out_row_stride = k, k, n
    P.x, P.w, P.out, P.bias = (i * _lib.FRESH_ADDRESS if i else None for i in (1, 2, 3, 4 if bias else 0))
    if residual:
        P.residual, P.gate, P.res_row_stride, P.gate_batch_stride, P.rows_per_batch = 5 * _lib.FRESH_ADDRESS, 6 * _lib.FRESH_ADDRESS, n, n, tokens & -tokens
    status, kernel = _lib.plan("zigma_linear_fwd", P)
    return kernel if status == 0 else None


def family(kernel):
    """the table's name (KERNELS) of the family a kernel that zigma_linear_fwd's plan names belongs to; None for None"""
    if kernel is None:
        return None
    return "ws128" if kernel == "linear_ws_128" else "ws" if kernel.startswith("linear_ws") else "sm" if kernel.startswith("linear_sm_") else "tiled"


def serves(kernel, tokens, n, k):
    """the kernel family `kernel` (KERNELS, or "4w": the generated 4-wave kernel within "tiled") takes the canonical call of this shape"""
    if kernel == "library":
        return True
    if kernel == "tiled_halves":        # (policy: each half is whole 256-feature tiles)
        return n % 512 == 0 and serves("tiled", tokens, n // 2, k)
    got = _canonical(SELECTOR.get(kernel, 0), tokens, n, k)
    return got is not None and got.startswith("linear4w") if kernel == "4w" else family(got) == kernel


serves_tiled, serves_sm = functools.partial(serves, "tiled"), functools.partial(serves, "sm")
serves_4w = functools.partial(serves, "4w")          # the generated one-wave-per-SIMD kernel takes the call (linear4w_variant; smaller calls: the 8-wave kernel)
serves_ws = lambda tokens, n, k: serves("ws", tokens, n, k) or serves("ws128", tokens, n, k)          # in either panel width (linear_ws_panel)


# ---- the table: first matching enabled row whose kernel serves the shape wins ----------------------------------------------------------------
# k / n: a set of values, or (lo, hi) inclusive; tokens: (lo, hi) inclusive.
TABLE = (
    # -- in_proj: E -> 4E, no epilogue
    Row("in_proj.ws", "in_proj", {512, 640}, (1024, 8192), (8192, INF), "ws", False,
        "W_in panels resident in registers, only tokens stream: 33.5 / 52 / 93 / 186 us at 8192 ... 65 536 tokens against 41.5 / 72 / 106 / 200 (library), "
        "profiles/r04_g_linear_ws_probe.jsonl, r05_e_bench_kernel_stats.csv"),
    Row("in_proj.library_k768", "in_proj", {768}, (2048, INF), (65536, INF), "library", False,
        "E = 768 at >= 65 536 tokens: hipBLASLt 262-270 us against 276-303 for the 4-wave kernel (weights of k = 768 do not fit the weight-stationary form: 384 registers per "
        "lane); inside config 3y's forward 23.44-23.55 ms per evaluation with the library against 24.16-24.27 (one launch) / 24.16-24.19 (halves): -3.0 %, round 6 A/B on one box "
        "(DESIGN.md §0).  A plain GEMM without epilogue: the one place the library is the faster kernel"),
    Row("in_proj.tiled_wide_k", "in_proj", (704, INF), (2048, INF), (8192, INF), "tiled", False,
        "E = 768 (every shipped yaml): ONE launch of the 4-wave kernel, 49 / 71 / 139 / 268 us against 60 / 72 / 137 / 263 (library) and 58 / 93 / 141 / 275 as halves, "
        "profiles/r05_b_shapes_probe.jsonl; needs serves_4w (checked below)"),
    Row("in_proj.tiled_narrow", "in_proj", (192, INF), (128, 1024), (8192, INF), "tiled", False,
        "E <= 256: n <= 1024 is where the 4-wave kernel at least ties the library (as to_q); needs serves_4w"),
    Row("in_proj.halves", "in_proj", (64, INF), (2048, INF), (32768, INF), "tiled_halves", False,
        "a half's weight panel stays in an XCD's L2: 2 x 100 us against 215-222 as one launch and 190-200 for the library at E = 640 (round 3)"),
    Row("in_proj.library", "in_proj", (1, INF), (1, INF), (1, INF), "library", False, "below 8192 tokens the library ties or wins (4096: a tie)"),
    # -- out_proj: 2E -> E, optional gated add
    Row("out_proj.sm", "out_proj", (128, INF), (128, INF), (2048, 8192), "sm", False,
        "one round of 128 x n/4 tiles: 18.9 us at 8192 tokens (E = 640) against 22.4 library / 25.3 ws128; E = 768 24.2 against 25.9 / 33.8; its gated add stays in the "
        "next norm kernel (fused: config 5 +2 %), profiles/r05_k_/r05_l_shapes_probe*.jsonl, r05_p_few_token_fuse_ab.jsonl"),
    Row("out_proj.tiled", "out_proj", (192, INF), (128, INF), (16384, INF), "tiled", True,
        "from 256 tiles on the 4-wave kernel carries the gated add: 117-122 us at 65 536 tokens (E = 640) against 116 + the add in the norm kernel; needs serves_4w"),
    Row("out_proj.ws128", "out_proj", {1280, 1536}, (128, 4096), (8193, 32767), "ws128", False,
        "16 384 tokens: two rounds of the few-token kernel's 144 KB workgroups lose in the forward (7.05 vs 6.83 ms); 128-feature panels 38 us, add in the next norm"),
    Row("out_proj.library", "out_proj", (1, INF), (1, INF), (1, INF), "library", False, "shapes none of the above holds (e.g. k = 1024 at 16 384 tokens)"),
    # -- to_q: E -> 512, no epilogue
    Row("to_q.sm", "to_q", (128, INF), (128, INF), (2048, 8192), "sm", False,
        "11.5 us at 8192 tokens against 19.8 (library) / 17.2 (ws) / 20.9 (8-wave), profiles/r05_l_shapes_probe_linear_sm_128.jsonl"),
    Row("to_q.tiled", "to_q", (64, INF), (128, INF), (8192, INF), "tiled", False,
        ">= 32 768 tokens the 4-wave kernel ties the library (46-47 vs 44-47 us at 65 536); 16 384: the 8-wave kernel 22.7-23.7 vs 20.9-21.9 — taken so no library "
        "GEMM is left in the block loop (B = 16 forward 7.17 vs 7.16-7.35 ms)"),
    Row("to_q.library", "to_q", (1, INF), (1, INF), (1, INF), "library", False, "below 2048 tokens"),
    # -- to_out: 512 -> E, bias + gated add
    Row("to_out.sm", "to_out", (128, INF), (128, INF), (2048, 8192), "sm", True, "bias + gated add in the few-token kernel's epilogue (round 5)"),
    Row("to_out.tiled", "to_out", (64, INF), (128, 4096), (8, INF), "tiled", True,
        "the library cannot fuse bias + gated add: 54 us (67 in the forward) against 70 + the add (round 3)"),
    Row("to_out.library", "to_out", (1, INF), (1, INF), (1, INF), "library", False, "shapes the tiled kernels do not serve"),
    # -- text: B x 77 text rows padded to 256, tiled wherever it serves
    Row("text.tiled", "text", (1, INF), (1, INF), (1, INF), "tiled", False, "y_embedder and the batched K / V of all blocks in one launch each"),
    Row("text.library", "text", (1, INF), (1, INF), (1, INF), "library", False, "shapes the tiled kernels do not serve"),
    # -- train: forward product and dX of the training path, weight-stationary where it serves the shape (no bias), then tiled
    Row("train.ws", "train", (1, INF), (1, INF), (1, INF), "ws", False, "round 4: the forward and dX of in_proj (k = 640) and to_q"),
    Row("train.ws128", "train", (1, INF), (1, INF), (1, INF), "ws128", False, "round 4: out_proj's forward (k = 1280)"),
    Row("train.tiled", "train", (1, INF), (1, INF), (1, INF), "tiled", False, "every other product the tiled kernels serve"),
    Row("train.library", "train", (1, INF), (1, INF), (1, INF), "library", False, "shapes the tiled kernels do not serve"),
)
BLOCK_ROLES = ("in_proj", "out_proj", "to_q", "to_out")
ROLES = BLOCK_ROLES + ("text", "train")

_knobs.apply(globals(), "routing")


def _in(v, spec):
    return v in spec if isinstance(spec, (set, frozenset)) else spec[0] <= v <= spec[1]


def _disabled():
    return DISABLED if isinstance(DISABLED, (set, frozenset)) else {s for s in str(DISABLED).split("+") if s}


def candidates(role, tokens, n, k):
    """the routes the table offers a bf16 / fp16 inference call of `role` with `tokens` rows, n output and k input features, best first; the last is the library"""
    if role not in ROLES:
        raise ValueError(f"routing: unknown role {role!r}")
    if POLICY == "off":
        yield Route("library", False, "policy.off")
        return
    if POLICY == "all" and role in BLOCK_ROLES:
        if serves("tiled", tokens, n, k):
            yield Route("tiled", role in ("out_proj", "to_out"), "policy.all")
        yield Route("library", False, "policy.all")
        return
    off = _disabled()
    for row in TABLE:
        if row.role != role or row.id in off or not (_in(k, row.k) and _in(n, row.n) and _in(tokens, row.tokens)):
            continue
        if not serves(row.kernel, tokens, n, k):
            continue
        if row.id in ("in_proj.tiled_wide_k", "in_proj.tiled_narrow", "out_proj.tiled") and not serves("4w", tokens, n, k):
            continue              # (these rows are only faster than what follows them on the 4-wave kernel)
        yield Route(row.kernel, row.fuse_add, row.id)
        if row.kernel == "library":
            return
    raise AssertionError("routing: the table's last row of every role matches everything")


def route(role, tokens, n, k):
    """the table's decision for this shape (the first of candidates())"""
    return next(candidates(role, tokens, n, k))


def kernel_name(route_or_kernel, tokens=None, n=None, k=None, bias=False, residual=False):
    """what zigma_last_kernel() reports for a call served by this route (prefix for the families with several tile shapes); bias / residual: the
    epilogue operands of the call — the 4-wave or the 8-wave kernel is the plan's answer for the canonical call of the shape with them attached"""
    kern = route_or_kernel.kernel if isinstance(route_or_kernel, Route) else route_or_kernel
    if kern in ("tiled", "tiled_halves"):
        if tokens is None:
            return "linear"
        got = _canonical(0, tokens, n // 2 if kern == "tiled_halves" else n, k, bool(bias), bool(residual))
        return got if got is not None and got.startswith("linear4w") else "linear_tn_"
    return {"ws": "linear_ws", "ws128": "linear_ws_128", "sm": "linear_sm_", "split3": "linear_split3_", "split1": "linear_split1_", "library": "library"}[kern]
