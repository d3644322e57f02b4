"""Case tables of the forward Mamba-inner sweep: scan_tok2_kernel, scan_tok_kernel (zigma_selective_scan_fwd), zigma_conv_x_proj_fwd,
zigma_x_proj_fwd (both kernels) and zigma_dt_proj_softplus_fwd.

Plain numpy, importable without a GPU.  Five seeded generators — scan2_cases() / scan1_cases() / conv_xproj_cases() / xproj_cases() /
dtproj_cases() — yield dicts of PARAMETERS with stable ids; *_inputs(case) makes the numbers from the case's seed, already rounded to the
case's I/O type; *_reference(case, inputs) evaluates everything in float64 (the recurrence through zo.selective_scan(..., dt=np.float64),
products and the conv in float64 numpy).  tests/test_fwd_fuzz_cases_cpu.py checks coverage, the references against an independent float64
restatement and the rounding model; tests/test_gpu_fwd_fuzz.py runs the kernels.

Layouts: token-major, (batch, position, channel).  u, the step sizes, B and C are in SCAN order; z lives at row zi[k] and out / out_z at row
oi[k] (z_row_index / out_row_index; two DIFFERENT permutations).  B | C are columns R, R + N of one x_dbl-shaped buffer whose other columns
are NaN unless the in-kernel dt_proj reads them.

Limits.  Every comparison is with the UNROUNDED float64 reference on the same rounded operands.  Norm-wise: IO_BOUND — fp32 2e-5 (the
existing fp32 bound of these kernels), bf16 2.5e-3 (the project's bound for one bf16 output rounding, test_linear_kernel_vs_float64), fp16
that / 8 (three more mantissa bits, the convention of tests/test_gpu_fp16.py); carries and checkpoints (fp32) STATE_BOUND = 2e-5.  Row-wise:
rowwise_worst <= ROW_GUARD over every (sample, position) row of an output and every (chunk | tile, channel) row of the carries and
checkpoints; element-wise for the dt_proj output.  Rounding a float64 result to bf16 / fp16 costs at most 2^-9 / 2^-12 of a row's norm =
0.78 of these bounds; the guard of 4 is the earlier sweeps'.  A case whose fp32 numpy model (same operands, result rounded to the I/O type)
needs more than half a limit carries the bound max(base, 2 x d_model) in RAISED below (written by `python tests/test_fwd_fuzz_cases_cpu.py`,
never from a kernel's output).  Forms whose definition contains a 16-bit delta tensor (DTP-split, the dt_proj kernel) are checked in stages:
the delta element-wise against float64, at most DELTA_FLIPS of its elements off the correctly rounded value, then the scan against float64
on the kernel's OWN delta.
"""
import numpy as np

from bwd_fuzz_cases import ROW_GUARD, elementwise_worst, round_to, rowwise_worst  # noqa: F401  (re-exported to the two test files)
from oracle import zigma_oracle as zo

IO_BOUND = {"f32": 2e-5, "bf16": 2.5e-3, "f16": 2.5e-3 / 8}
STATE_BOUND = 2e-5
DELTA_FLIPS, DELTA_FLIPS_MODEL = 0.02, 0.01
REGIMES = ("benign", "long", "model", "edges")
SCAN2_L, SCAN2_DIM, SCAN2_R = (16, 32, 48, 64, 112, 256), (64, 128, 192), (32, 40, 48, 64)
SCAN2_SPLITS = ((48, 16), (64, 16), (64, 32), (64, 48), (112, 48), (112, 32), (112, 16), (256, 32), (256, 48), (256, 16))   # (L, chunk_len)
SCAN2_R6 = ((24, 4096, 16), (24, 4096, 32), (1300, 64, 16))          # (B, dim, L): 1281 ... 1536 workgroups
SCAN1_L = (1, 3, 15, 16, 17, 31, 33, 100, 257)
R_PLAIN = 8                     # dt columns in front of B | C where no dt_proj reads them (NaN)

# fp32 A with fl32(A * fl32(log2 e)) == -1: a unit step then decays the state by exp2(-1) = 0.5 exactly in the kernels' arithmetic
_K = np.float32(1.4426950408889634)


def _find_a_half():
    a = np.float32(-np.log(2.0))
    cands = [a]
    lo = hi = a
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(0))
        cands += [lo, hi]
    return next(c for c in cands if np.float32(c * _K) == np.float32(-1))


A_HALF = _find_a_half()

# raised bounds, id -> {output: bound}: max(base, 2 x d_model), d_model measured on the CPU (tests/test_fwd_fuzz_cases_cpu.py writes this table)
RAISED = {}


# ---------------------------------------------------------------------------------------------------
# the scan tables
# ---------------------------------------------------------------------------------------------------
def split_served(c):
    """plan_scan's tok2_split_ok / tok_split_ok for a case that passes the carry tensor"""
    n_chunks, slabs = -(-c["L"] // c["chunk"]), c["B"] * (c["dim"] // 64)
    return c["chunk"] % 16 == 0 and 2 <= n_chunks <= 65535 and slabs < 768 and not c["out"] and not c["reset"]


def expected_kernel(c):
    """(zigma_last_kernel(), info[1]) the plan must report: restated from plan_scan (csrc/scan_plan.h); the CPU test checks it against the compiled plan"""
    slabs = c["B"] * (c["dim"] // 64)
    if c["dt"]:
        if c["chunk"]:
            return "scan_tok2_n16_split_dtproj", 0
        r6 = -(-slabs // 1536) < -(-slabs // 1280) and not c["r5"]
        return "scan_tok2_n16_dtproj" + ("_r6" if r6 else "") + ("_acc" if c["acc"] else ""), 0
    hot = c["kind"] != "f32" and c["N"] == 16 and c["L"] % 16 == 0 and c["z"] and not c["v1"] and (not c["chunk"] or split_served(c))
    if hot:
        return "scan_tok2_n16", int(c["ckpt"] and c["out"])
    return f"scan_tok_n{c['N']}", int(c["ckpt"] and c["z"] and c["out"])


def _scan_case(table, seed0, **kw):
    c = dict(kind="bf16", N=16, B=2, dim=64, L=64, z=True, D=True, bias=True, softplus=True, tables=False, zact=False, out=False, ckpt=False,
             chunk=0, dt=False, R=R_PLAIN, pitch=0, acc=False, reset=0, regime="benign", views=True, twice=False, known=False, v1=False, r5=False,
             r6_twin=False)
    c.update(kw)
    if not c["pitch"]:
        c["pitch"] = c["R"] + 2 * c["N"]
    if not c["z"]:
        c.update(zact=False, out=True)
    c["seed"] = seed0 + len(table)
    opts = "".join(ch for ch, on in (("z", c["z"]), ("D", c["D"]), ("b", c["bias"]), ("s", c["softplus"]), ("t", c["tables"]), ("a", c["zact"]),
                                     ("o", c["out"] and c["z"]), ("k", c["ckpt"]), ("v", c["views"]), ("1", c["v1"])) if on)
    c["id"] = (f"{c['form']}-{c['kind']}-n{c['N']}-b{c['B']}-d{c['dim']}-L{c['L']}-{c['regime']}-{opts}" + (f"-c{c['chunk']}" if c["chunk"] else "")
               + (f"-R{c['R']}p{c['pitch']}" if c["dt"] else "") + (f"-r{c['reset']}" if c["reset"] else "") + ("-known" if c["known"] else ""))
    c["kernel_name"], c["info1"] = expected_kernel(c)
    table.append(c)
    return c


SCAN2_PLAIN_FORMS = {      # forms that take a plain delta, one workgroup per (sample, slab) or the split
    "whole": dict(), "whole-bias": dict(softplus=False), "whole-softplus": dict(bias=False), "whole-none": dict(bias=False, softplus=False),
    "tab": dict(tables=True), "zact": dict(zact=True), "out": dict(out=True), "out-ckpt": dict(out=True, ckpt=True, tables=True),
    "reset": dict(tables=True),
}
SCAN2_FORMS = tuple(SCAN2_PLAIN_FORMS) + ("split", "split-tab-zact", "dtp", "dtp-zact-tab", "dtp-acc", "dtp-reset", "dtp-split", "dtp-r6", "dtp-r6-acc")
KNOWN_FORMS = ("whole-none", "tab", "zact", "out-ckpt", "reset", "split", "split-tab-zact")


def scan2_cases():
    """scan_tok2_kernel, bf16 and fp16, every form plan_scan can serve x the four value regimes.  Keys: form, kind, N, B, dim, L, z / D / bias /
    softplus, tables, zact (z holds silu(z)), out (training form: ungated out as well), ckpt, chunk (chunk_len of a sequence split: the carry
    tensor is passed), dt (in-kernel dt_proj: R = dt_rank, pitch = x_dbl row pitch), acc, reset (reset_period), regime, views (operands and
    outputs are slices of NaN-filled buffers), twice, known (known-answer case: bit for bit), r6_twin (also run pinned to five resident
    workgroups: bit-identical), kernel_name / info1 (what the plan must report), seed."""
    out, i = [], 0
    for kind in ("bf16", "f16"):
        for form, kw in SCAN2_PLAIN_FORMS.items():
            for regime in REGIMES:
                L = SCAN2_L[i % 6]
                reset = (16, 32, 64)[i % 3] if form == "reset" else 0
                if reset:
                    L = max(L, 2 * reset) if L % reset == 0 else (L // reset + 2) * reset
                _scan_case(out, 11000, form=form, kind=kind, regime=regime, L=L, dim=SCAN2_DIM[i % 3], B=1 + (i // 2) % 3, D=i % 4 != 3,
                           views=i % 3 != 2, reset=reset, **kw)
                i += 1
        for j in range(12):         # the split family: every (L, chunk_len) pair, ragged last chunks included
            form = ("split", "split-tab-zact", "dtp-split")[j % 3]
            L, chunk = SCAN2_SPLITS[(j + (5 if kind == "f16" else 0)) % 10]
            kw = dict(tables=True, zact=True) if form == "split-tab-zact" else dict(dt=True, R=SCAN2_R[j % 4]) if form == "dtp-split" else {}
            if form == "dtp-split":
                kw["pitch"] = (kw["R"] + 32, kw["R"] + 40, 128)[j % 3]
            _scan_case(out, 11000, form=form, kind=kind, regime=REGIMES[(j // 3) % 4], L=L, chunk=chunk, dim=SCAN2_DIM[j % 3], B=1 + j % 3,
                       views=j % 4 != 3, **kw)
        for j in range(16):         # dt_proj inside the kernel, five resident workgroups
            form = ("dtp", "dtp-zact-tab", "dtp-acc", "dtp-reset")[j % 4]
            R = SCAN2_R[(j + j // 4) % 4]
            kw = dict(dt=True, R=R, pitch=(R + 32, R + 40, 128)[j % 3])
            kw.update(dict(zact=True, tables=True) if form == "dtp-zact-tab" else dict(acc=True, tables=j % 8 < 4) if form == "dtp-acc" else {})
            L = SCAN2_L[(j + 2) % 6]
            if form == "dtp-reset":
                reset = (16, 32, 64)[(j // 4) % 3]
                kw.update(reset=reset, tables=True)
                L = max(L, 2 * reset) if L % reset == 0 else (L // reset + 2) * reset
            _scan_case(out, 11000, form=form, kind=kind, regime=REGIMES[(j // 4) % 4], L=L, dim=SCAN2_DIM[j % 3], B=1 + (j // 2) % 3, D=j % 5 != 4,
                       views=j % 3 != 1, **kw)
        for j in range(8):          # six resident workgroups (1281 ... 1536 of them), plain and accumulating; each also pinned to five
            Bsz, dim, L = SCAN2_R6[(j + j // 4) % 3]
            R = SCAN2_R[j % 4]
            _scan_case(out, 11000, form=("dtp-r6", "dtp-r6-acc")[j // 4], kind=kind, regime=REGIMES[j % 4], B=Bsz, dim=dim, L=L, dt=True, R=R,
                       pitch=(R + 32, 128)[j % 2], acc=j >= 4, tables=j % 2 == 0, views=j % 4 == 0, r6_twin=True)
        for form in KNOWN_FORMS:    # known answers: one per form that takes a plain delta
            kw = dict(SCAN2_PLAIN_FORMS.get(form, {}))
            kw.update(dict(chunk=16) if form.startswith("split") else {})
            kw.update(dict(tables=True, zact=True) if form == "split-tab-zact" else {})
            kw.update(bias=False, softplus=False)
            _scan_case(out, 11000, form=form, kind=kind, regime="known", known=True, L=32, dim=64 if form == "tab" else 128, B=2,
                       reset=16 if form == "reset" else 0, views=form != "zact", **kw)
        done = 0
        for c in out:               # determinism: a table case and a split case per I/O type run twice
            if c["kind"] == kind and not c["known"] and c["form"] in ("tab", "split") and c["L"] >= 48 and done < 2 and not c["twice"]:
                c["twice"], done = True, done + 1
        assert done == 2
    return out


def scan1_cases():
    """scan_tok_kernel: fp32 I/O, ragged lengths, dstate 8, no gate, carries, the probe pin.  Same keys as scan2_cases()."""
    out, rng = [], np.random.default_rng(20251)
    i = 0
    for kind in ("f32", "bf16", "f16"):
        for N in (16, 8):
            for L in SCAN1_L:
                o = int(rng.integers(0, 32))
                z = bool(o & 1)
                c = dict(form="tok", kind=kind, N=N, L=L, B=1 + i % 3, dim=SCAN2_DIM[(i // 2) % 3], z=z, D=bool(o & 2), bias=bool(o & 4), softplus=bool(o & 8),
                         tables=bool(o & 16), regime=REGIMES[i % 4], views=i % 3 != 0, out=z and i % 5 == 0)
                c["v1"] = kind != "f32" and N == 16 and L % 16 == 0 and z      # the hot kernel would take it: pinned to the first generation
                _scan_case(out, 12000, **c)
                i += 1
    for j, (L, N) in enumerate((L, N) for L in (48, 100, 257) for N in (16, 8)):       # fp32 sequence split, ragged last chunk
        _scan_case(out, 12000, form="tok-split", kind="f32", N=N, L=L, chunk=32, B=1 + j % 2, dim=SCAN2_DIM[j % 3], z=j % 3 != 2, tables=j % 2 == 0,
                   regime=REGIMES[j % 4], views=j % 2 == 1)
    for j, kind in enumerate(("f32", "bf16", "f16")):
        # carries without a split: 768 workgroups fill the chip, the carry of every chunk end is still written
        _scan_case(out, 12000, form="tok-carries", kind=kind, N=(16, 8, 16)[j], L=(40, 33, 48)[j], chunk=16, B=768, dim=64, z=j != 1, v1=j == 2,
                   regime=REGIMES[1 + j], views=False)
        # the training form: gate, ungated out and the checkpoints
        _scan_case(out, 12000, form="tok-ckpt", kind=kind, N=(16, 8, 16)[j], L=(100, 48, 33)[j], B=2, dim=128, z=True, out=True, ckpt=True, tables=j != 1,
                   regime=REGIMES[j], views=j != 0)
    return out


# leaves of tests/scan_plan_cases.py that launch a token-major kernel -> the cases of the two tables that reach the same leaf of plan_scan
PLAN_LEAVES = {
    "tok_f32": lambda c: c["form"] == "tok" and c["kind"] == "f32" and c["N"] == 16,
    "tok_dstate8": lambda c: c["form"] == "tok" and c["N"] == 8,
    "tok_ragged_length": lambda c: c["form"] == "tok" and c["kind"] != "f32" and c["N"] == 16 and c["L"] % 16 != 0 and c["z"],
    "tok_no_gate": lambda c: c["form"] == "tok" and c["kind"] != "f32" and c["N"] == 16 and not c["z"] and c["L"] % 16 == 0,
    "tok_probe_v1": lambda c: c["v1"] and c["kernel_name"] == "scan_tok_n16",
    "tok_split": lambda c: c["form"] == "tok-split" and c["N"] == 16,
    "tok_carries_without_split": lambda c: c["form"] == "tok-carries",
    "tok_training_checkpoints": lambda c: c["form"] == "tok-ckpt" and c["kind"] == "f32",
    "tok2_gated": lambda c: c["form"] == "whole",
    "tok2_no_bias_no_softplus": lambda c: c["form"] == "whole-none",
    "tok2_tables_zact_f16": lambda c: c["form"] == "split-tab-zact" or (c["form"] == "zact" and c["kind"] == "f16"),
    "tok2_training_form": lambda c: c["form"] == "out",
    "tok2_training_checkpoints": lambda c: c["form"] == "out-ckpt",
    "tok2_split": lambda c: c["form"] == "split",
    "tok2_split_tables_zact": lambda c: c["form"] == "split-tab-zact",
    "dtp_r5": lambda c: c["form"] == "dtp",
    "dtp_r6": lambda c: c["form"] == "dtp-r6",
    "dtp_r6_pinned_to_r5": lambda c: c["r6_twin"],
    "dtp_acc": lambda c: c["form"] == "dtp-acc",
    "dtp_r6_acc": lambda c: c["form"] == "dtp-r6-acc",
    "dtp_zact_tables": lambda c: c["form"] == "dtp-zact-tab",
    "dtp_f16_reset_period": lambda c: c["form"] == "dtp-reset" and c["kind"] == "f16",
    "dtp_split": lambda c: c["form"] == "dtp-split",
}
# launches the hot kernel too, but only above 65 535 samples (134 MB of output at the smallest shape): tests/test_gpu_parity.py keeps it
PLAN_LEAVES_ELSEWHERE = ("slices_above_65535_samples",)


def _tables(rng, L, period):
    one = lambda: np.concatenate([a + rng.permutation(min(period, L - a)) for a in range(0, L, period)]).astype(np.int32)
    zi, oi = one(), one()
    while L > 1 and np.array_equal(zi, oi):
        oi = one()
    return zi, oi


EDGE_BIAS = ((slice(0, 4), 20.0), (slice(4, 8), -4.5), (slice(8, 12), -18.0))     # the pass-through, the series / log switch, log2(1 + 2^t) = 0


def _known_inputs(c, Bsz):
    """unit steps with A_HALF (decay exactly 0.5), small integers, u alive on steps 12 ... 18 only (across the tile, chunk and reset edge at 16):
    the state spans 10 bits, every product and sum is exact in fp32; the gate is z in {64, 96, 128}, where silu(z) == z in fp32 and float64"""
    L, dim, N, R = c["L"], c["dim"], c["N"], c["R"]
    rng = np.random.default_rng(c["seed"])
    ints = lambda lo, hi, *s: rng.integers(lo, hi + 1, s).astype(np.float32)
    u = np.zeros((Bsz, L, dim), np.float32)
    u[:, 12:19] = ints(-3, 3, Bsz, 7, dim)
    xdbl = np.full((Bsz, L, c["pitch"]), np.nan, np.float32)
    xdbl[..., R:R + 2 * N] = ints(-2, 2, Bsz, L, 2 * N)
    z = rng.choice(np.array([64.0, 96.0, 128.0], np.float32), (Bsz, L, dim))
    zi, oi = _tables(rng, L, c["reset"] or L) if c["tables"] else (None, None)
    return dict(u=u, z=z, gate=z.astype(np.float64), xdbl=xdbl, w=None, delta=np.ones((Bsz, L, dim), np.float32), A=np.full((dim, N), A_HALF, np.float32),
                D=ints(-2, 2, dim) if c["D"] else None, bias=None, zi=zi, oi=oi, out_z0=None)


def scan_inputs(c, batch=None):
    """token-major numpy inputs of a scan case, rounded to its I/O type (batch: fewer samples, for the CPU checks of the wide cases)"""
    Bsz = min(batch or c["B"], c["B"])
    if c["known"]:
        return _known_inputs(c, Bsz)
    kind, L, dim, N, R, reg = c["kind"], c["L"], c["dim"], c["N"], c["R"], c["regime"]
    rng = np.random.default_rng(c["seed"])
    rt = lambda a: round_to(a, kind)
    rn = lambda *s: rng.standard_normal(s)
    edges = reg == "edges"
    u, z = rn(Bsz, L, dim), rn(Bsz, L, dim)
    if edges:
        u[..., :4] *= 0.05          # the channels whose step is ~20: their outputs stay of the size of the others
    bc = rn(Bsz, L, 2 * N) * (0.5 if edges else 1.0)
    if reg == "benign":
        A = -(0.5 * rng.random((dim, N)) + 1e-3)
    elif reg == "long":
        A = -(0.05 + 0.95 * rng.random((dim, N)))
    else:
        A = -np.arange(1, N + 1)[None] * np.exp(0.2 * rn(dim, N))
    rows = rng.permutation(Bsz * L)[:12]                  # (sample, position) rows that carry the edge values
    row = lambda k: divmod(int(rows[k % len(rows)]), L)
    bias = delta = w = None
    if c["softplus"]:
        bias = {"benign": 0.5 * rng.random(dim), "long": -4.2 + 0.3 * rn(dim) if c["dt"] else 0.1 * rn(dim)}.get(reg, rn(dim) - 3.0)
        if edges:
            for sl, v in EDGE_BIAS:
                bias[sl] = v
    else:
        bias = (0.5 if reg == "benign" else 0.005) * rng.random(dim)
    if not c["bias"]:
        bias = np.zeros(dim)
    xdbl = np.full((Bsz, L, c["pitch"]), np.nan)
    if c["dt"]:
        xdbl[..., :R] = rn(Bsz, L, R)
        w = rn(dim, R) * R ** -0.5 * {"benign": 0.5, "long": 0.3}.get(reg, 1.0)
        if edges:
            w[:12] *= 0.25
    elif c["softplus"]:
        if reg == "benign":
            delta = rng.random((Bsz, L, dim)) - 0.3
        elif reg == "long":
            delta = np.log(np.expm1(rng.uniform(0.005, 0.05, (Bsz, L, dim)))) - bias
        else:
            delta = rn(Bsz, L, dim)
            if edges:
                delta[..., :12] = np.clip(0.4 * delta[..., :12], -0.5, 0.5)
                delta[..., 4:8] *= 3.0          # -6 ... -3 around the bias of -4.5
    else:           # no softplus: the step itself, positive
        if reg == "benign":
            delta = 0.5 * rng.random((Bsz, L, dim))
        elif reg == "long":
            delta = rng.uniform(0.005, 0.05, (Bsz, L, dim))
        else:
            delta = zo.softplus(rn(Bsz, L, dim) + rn(dim) - 3.0)
    if edges:
        for k, v in enumerate((12.0, -12.0, 30.0, -30.0)):
            b, l = row(k)
            z[b, l] = v
        (b, l), (b2, l2), (b3, l3) = row(4), row(5), row(6)
        u[b, l], bc[b2, l2, :N], bc[b3, l3, N:] = 0.0, 0.0, 0.0
        if kind == "f16":           # subnormal operands (below 6.1e-5)
            (b, l), (b2, l2) = row(7), row(8)
            u[b, l] = 3e-6 * rn(dim)
            bc[b2, l2, :N] = 2e-6 * rn(N)
            z[row(9)] = 1e-6 * rn(dim)
    xdbl[..., R:R + 2 * N] = bc
    u, xdbl = rt(u), rt(xdbl)
    if c["zact"]:
        z = rt(zo.silu(rt(z).astype(np.float64)))
        gate = z.astype(np.float64)
    else:
        z = rt(z)
        gate = zo.silu(z.astype(np.float64))
    zi, oi = _tables(rng, L, c["reset"] or L) if c["tables"] else (None, None)
    return dict(u=u, z=z if c["z"] else None, gate=gate if c["z"] else None, xdbl=xdbl, w=None if w is None else rt(w),
                delta=None if delta is None else rt(delta), A=A.astype(np.float32), D=(1 + 0.2 * rn(dim)).astype(np.float32) if c["D"] else None,
                bias=bias.astype(np.float32) if c["bias"] else None, zi=zi, oi=oi, out_z0=rt(rn(Bsz, L, dim)) if c["acc"] else None)


def pre_softplus(c, inp, dt=np.float64):
    pre = inp["xdbl"][..., :c["R"]].astype(dt) @ inp["w"].astype(dt).T if c["dt"] else inp["delta"].astype(dt)
    return pre if inp["bias"] is None else pre + inp["bias"].astype(dt)


def step_sizes(c, inp, dt=np.float64):
    """(B, L, dim): the step size the recurrence runs on"""
    pre = pre_softplus(c, inp, dt)
    return zo.softplus(pre) if c["softplus"] else pre


def _cf(a, s, dt):
    return np.ascontiguousarray(np.asarray(a, dt)[:, s].transpose(0, 2, 1))        # (B, l, C) -> (B, C, l)


def _finish(c, inp, y, ref):
    """gate, accumulate and place the scan-order y: out_z / out as the kernel lays them out"""
    def place(a):
        if inp["oi"] is None:
            return a
        full = np.empty_like(a)
        full[:, inp["oi"]] = a
        return full
    if c["z"]:
        g = inp["gate"] if inp["zi"] is None else inp["gate"][:, inp["zi"]]
        yz = place(y * g.astype(y.dtype))
        ref["out_z"] = yz if not c["acc"] else inp["out_z0"].astype(y.dtype) + yz
        if c["acc"]:
            ref["_acc_terms"] = (inp["out_z0"], yz)
    if c["out"]:
        ref["out"] = place(y)
    return ref


def scan_reference(c, inp, step=None, dt=np.float64):
    """Reference of a scan case in the kernel's output layout, except that the carries and checkpoints come as x_prod / x_state (B, chunk, dim, N)
    and ckpt (B, tile, dim, N), the state row last.  step: the kernel's OWN 16-bit delta (staged forms).  dt=np.float32: the rounding model."""
    own = step is not None
    step = step_sizes(c, inp, dt) if step is None else np.asarray(step, dt)
    u, R, N = inp["u"], c["R"], c["N"]
    Bm, Cm, A = inp["xdbl"][..., R:R + N], inp["xdbl"][..., R + N:R + 2 * N], inp["A"].astype(dt)
    Bsz, L, dim = u.shape
    period, chunk = c["reset"] or L, c["chunk"]
    ref = {}
    if c["dt"] and c["chunk"] and not own:
        ref["delta"] = step
    y = np.empty((Bsz, L, dim), dt)
    states = c["ckpt"] or chunk
    if c["ckpt"]:
        ref["ckpt"] = np.zeros((Bsz, -(-L // 16), dim, N), dt)
    if chunk:
        ref["x_prod"], ref["x_state"] = (np.zeros((Bsz, -(-L // chunk), dim, N), dt) for _ in range(2))
    for a in range(0, L, period):
        s = slice(a, min(a + period, L))
        y[:, s] = zo.selective_scan(_cf(u, s, dt), _cf(step, s, dt), A, _cf(Bm, s, dt), _cf(Cm, s, dt), inp["D"], dt=dt).transpose(0, 2, 1)
        if not states:
            continue
        H, cum = np.zeros((Bsz, dim, N), dt), np.zeros((Bsz, dim), dt)         # tile by tile: h_end = exp(A sum(step)) h_start + h_end(from 0)
        for t0 in range(a, s.stop, 16):
            ts = slice(t0, min(t0 + 16, s.stop))
            if c["ckpt"]:
                ref["ckpt"][:, t0 // 16] = H
            _, hl = zo.selective_scan(_cf(u, ts, dt), _cf(step, ts, dt), A, _cf(Bm, ts, dt), _cf(Cm, ts, dt), None, return_last_state=True, dt=dt)
            st = step[:, ts].sum(1, dtype=dt)
            H = np.exp(st[..., None] * A[None]) * H + hl
            cum = cum + st
            if chunk and (ts.stop % chunk == 0 or ts.stop == L):
                ref["x_prod"][:, (ts.stop - 1) // chunk], ref["x_state"][:, (ts.stop - 1) // chunk] = np.exp(cum[..., None] * A[None]), H
    return _finish(c, inp, y, ref)


def known_answer(c, inp, dt=np.float64):
    """the known-answer cases as an explicit recurrence with the decay 0.5 written out; dt=np.float32: step by step in fp32, the decay taken
    the kernel's way, exp2(step * fl32(A * log2 e))"""
    u, R, N = inp["u"].astype(dt), c["R"], c["N"]
    Bm, Cm = inp["xdbl"][..., R:R + N].astype(dt), inp["xdbl"][..., R + N:R + 2 * N].astype(dt)
    Bsz, L, dim = u.shape
    decay = dt(0.5) if dt is np.float64 else np.exp2(inp["delta"][0, 0, 0] * np.float32(inp["A"] * _K))[None]
    ref, y, h = {}, np.empty((Bsz, L, dim), dt), np.zeros((Bsz, dim, N), dt)
    if c["ckpt"]:
        ref["ckpt"] = np.zeros((Bsz, L // 16, dim, N), dt)
    if c["chunk"]:
        ref["x_prod"], ref["x_state"] = (np.zeros((Bsz, L // c["chunk"], dim, N), dt) for _ in range(2))
    for l in range(L):
        if c["reset"] and l % c["reset"] == 0:
            h = np.zeros_like(h)
        if c["ckpt"] and l % 16 == 0:
            ref["ckpt"][:, l // 16] = h
        h = decay * h + (inp["delta"][:, l].astype(dt) * u[:, l])[..., None] * Bm[:, l, None, :]
        y[:, l] = (h * Cm[:, l, None, :]).sum(-1)
        if c["chunk"] and (l + 1) % c["chunk"] == 0:
            ref["x_prod"][:, l // c["chunk"]], ref["x_state"][:, l // c["chunk"]] = dt(0.5) ** (l + 1), h
    if inp["D"] is not None:
        y = y + u * inp["D"].astype(dt)
    return _finish(c, inp, y, ref)


def production_cases():
    """one shape per hot form where the model runs: B = 2, L = 1024, dim = 1280 with the real zigzag tables (in-kernel dt_proj), and B = 1,
    L = 4096, dim = 1280 in 16 chunks (DTP-split, the chunk length split_chunk_len picks)"""
    t = []
    _scan_case(t, 16000, form="production-dtp", kind="bf16", regime="model", B=2, L=1024, dim=1280, dt=True, R=40, pitch=72, tables=True)
    _scan_case(t, 16000, form="production-dtp-split", kind="bf16", regime="model", B=1, L=4096, dim=1280, dt=True, R=40, pitch=72, chunk=256)
    return t


def production_inputs(c):
    inp = scan_inputs(c)
    if c["tables"]:
        paths = zo.zigzag_paths(32)
        inp["zi"], inp["oi"] = paths[1].astype(np.int32), paths[2].astype(np.int32)
        assert not np.array_equal(inp["zi"], inp["oi"])
    return inp


STATE_KEYS = ("ckpt", "x_prod", "x_state")


def base_bound(c, key):
    return STATE_BOUND if key in STATE_KEYS else IO_BOUND[c["kind"]]


def bound_of(c, key):
    return max(base_bound(c, key), RAISED.get(c["id"], {}).get(key, 0.0))


def norm_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def row_ratio(got, ref, bound, terms=None):
    """rowwise_worst; terms = (a, b) for a sum a + b that can cancel: a row's denominator is |a row| + |b row|"""
    if terms is None:
        return rowwise_worst(got, ref, bound)
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rows = lambda a: np.linalg.norm(np.asarray(a, np.float64).reshape(-1, ref.shape[-1]), axis=1)
    rn = rows(terms[0]) + rows(terms[1])
    den = bound * np.maximum(np.maximum(rn, np.sqrt(np.mean(rn * rn))), 1e-300)
    return float(np.max(rows(got - ref) / den))


def need(got, ref, terms=None, elementwise=False):
    """the smallest bound `got` passes with, norm-wise and row by row (or element by element)"""
    worst = elementwise_worst(got, ref, 1.0) if elementwise else row_ratio(got, ref, 1.0, terms)
    return max(norm_err(got, ref), worst / ROW_GUARD)


def model_excess(model, ref, kind, terms=None, elementwise=False):
    """The fp32 numpy model of an output against its float64 reference -> (excess, d_model).  d_model: the smallest bound the model passes
    with once it is rounded to the type the output is stored in, norm-wise and row by row.  excess: what decides whether a case is raised —
    the model's distance BEFORE the output rounding norm-wise, and the rounded model's row by row in units of the guard.  (One bf16 / fp16
    rounding alone is 0.65 ... 0.8 of the norm-wise bound, which is why that bound is what it is: taking the rounded model norm-wise would
    raise every 16-bit case by the same factor and weaken the whole sweep; the arithmetic that can pile up is what the model is for.)"""
    rounded = round_to(model, kind)
    worst = (elementwise_worst(rounded, ref, 1.0) if elementwise else row_ratio(rounded, ref, 1.0, terms)) / ROW_GUARD
    return max(norm_err(model, ref), worst), need(rounded, ref, terms, elementwise)


def flipped_share(got, ref, kind):
    """share of the elements of a 16-bit tensor that are not the correctly rounded float64 value"""
    return float(np.mean(np.asarray(got, np.float32) != round_to(np.asarray(ref, np.float64).astype(np.float32), kind)))


def out_kind(c, key):
    return "f32" if key in STATE_KEYS else c["kind"]


# ---------------------------------------------------------------------------------------------------
# the feeder kernels
# ---------------------------------------------------------------------------------------------------
CX_SHAPES = ((1, 256), (8, 32), (4, 64), (2, 128), (3, 256), (1, 512))         # a 128-position workgroup spans 4, 2, 1 samples
CX_DIM, CX_N, CX_TABLES = (64, 128, 192, 320), (40, 48, 64, 72, 80, 96), ("none", "identity", "reversed", "random")


def conv_xproj_cases():
    """zigma_conv_x_proj_fwd.  Keys: kind, B, L, dim, n, table, flags (0 shipped form; probes 1 = three stages, 2 = eight-wave workgroups of 256
    positions, 3 = both), regime (benign | edges: SiLU pre-activations at +-12 and +-30), seed.  The entry point has no reset_period and no
    output pitch of the caller's; x_half is always the lower half of a (B, L, 2 dim) buffer whose upper half is NaN."""
    out = []
    for kind in ("bf16", "f16"):
        for i in range(24):
            Bsz, L = CX_SHAPES[i % 6]
            c = dict(kernel="conv_xproj", kind=kind, B=Bsz, L=L, dim=CX_DIM[(i + i // 6) % 4], n=CX_N[(i + i // 4) % 6], table=CX_TABLES[(i + i // 8) % 4],
                     flags=(i // 6) % 4, regime=("benign", "edges")[(i + i // 12) % 2], seed=13000 + len(out))
            c["id"] = f"{kind}-b{Bsz}-L{L}-d{c['dim']}-n{c['n']}-{c['table']}-f{c['flags']}-{c['regime']}"
            out.append(c)
    return out


def conv_xproj_inputs(c):
    rng = np.random.default_rng(c["seed"])
    rt = lambda a: round_to(a, c["kind"])
    Bsz, L, dim, n = c["B"], c["L"], c["dim"], c["n"]
    xz = np.full((Bsz, L, 2 * dim), np.nan, np.float32)
    xz[..., :dim] = rng.standard_normal((Bsz, L, dim))
    cb = 0.5 * rng.standard_normal(dim)
    if c["regime"] == "edges":
        cb[:4] = (12.0, -12.0, 30.0, -30.0)
        xz[..., :4] *= 0.05
    perm = {"none": None, "identity": np.arange(L), "reversed": np.arange(L)[::-1].copy(), "random": rng.permutation(L)}[c["table"]]
    return dict(xz=rt(xz), cw=rt(0.5 * rng.standard_normal((dim, 4))), cb=rt(cb), w=rt(rng.standard_normal((n, dim)) * dim ** -0.5),
                perm=None if perm is None else perm.astype(np.int32))


def conv_xproj_reference(c, inp, u_own=None, dt=np.float64):
    """u in float64; x_dbl in float64 from the kernel's OWN u (the definition rounds u to the I/O type before the projection)"""
    dim = c["dim"]
    x = inp["xz"][..., :dim] if inp["perm"] is None else inp["xz"][:, inp["perm"], :dim]
    u = zo.causal_conv1d(x.transpose(0, 2, 1), inp["cw"], inp["cb"], "silu", dt=dt).transpose(0, 2, 1)
    ref = dict(u=u)
    if u_own is not None:
        ref["x_dbl"] = np.asarray(u_own, dt) @ inp["w"].astype(dt).T
    return ref


XP_M, XP_K, XP_N = (1, 15, 16, 17, 257, 300, 1000), (256, 512, 1280, 1536), (33, 40, 72, 96)


def xproj_cases():
    """zigma_x_proj_fwd: x_proj_splitk (k <= 1536 below 16 384 tokens) and x_proj_mfma (reached through k = 2048).  Keys: kind, M, K, n, pad (extra
    NaN elements in the row pitch of u and of the weight), kernel_name, seed."""
    out = []
    for kind in ("bf16", "f16"):
        shapes = [(XP_M[i % 7], XP_K[(i + i // 7) % 4], XP_N[(i + i // 4) % 4]) for i in range(14)] + [(16, 2048, 72), (257, 2048, 33), (512, 2048, 96)]
        for i, (M, K, n) in enumerate(shapes):
            c = dict(kernel="xproj", kind=kind, M=M, K=K, n=n, pad=(0, 8, 24)[i % 3], kernel_name="x_proj_splitk" if K <= 1536 else "x_proj_mfma",
                     seed=14000 + len(out))
            c["id"] = f"{kind}-m{M}-k{K}-n{n}-p{c['pad']}"
            out.append(c)
    return out


def xproj_inputs(c):
    rng = np.random.default_rng(c["seed"])
    return dict(u=round_to(rng.standard_normal((c["M"], c["K"])), c["kind"]), w=round_to(rng.standard_normal((c["n"], c["K"])) * c["K"] ** -0.5, c["kind"]))


def xproj_reference(c, inp, dt=np.float64):
    return dict(x_dbl=inp["u"].astype(dt) @ inp["w"].astype(dt).T)


DT_M, DT_DIM, DT_R = (1, 15, 16, 17, 100, 333), (64, 128, 192), (8, 16, 32, 40, 48)


def dtproj_cases():
    """zigma_dt_proj_softplus_fwd.  Keys: kind, M, dim, R, pitch (x_dbl row pitch: R, R + 32 or 72; columns beyond R are NaN), w_pad (the weight's
    rows lie in a wider NaN-padded buffer), softplus, bias, regime (the scan's; `edges` puts pre-softplus values around 20, at -6 ... -3 and
    below -17), seed."""
    out = []
    for kind in ("bf16", "f16"):
        for i in range(30):
            R = DT_R[i % 5]
            pitch = (R, R + 32, 72)[(i + i // 5) % 3]
            sp, bias = ((True, True), (True, False), (False, True), (False, False))[(i + i // 6) % 4] if i % 4 != 3 else (True, True)
            c = dict(kernel="dtproj", kind=kind, M=DT_M[i % 6], dim=DT_DIM[(i + i // 6) % 3], R=R, pitch=pitch, w_pad=(8, 0, 16)[i % 3], softplus=sp,
                     bias=bias, regime="edges" if i % 4 == 3 else ("benign", "long", "model")[i % 3], seed=15000 + len(out))
            c["id"] = f"{kind}-m{c['M']}-d{c['dim']}-R{R}-p{pitch}-w{c['w_pad']}-{'s' if sp else ''}{'b' if bias else ''}-{c['regime']}"
            out.append(c)
    return out


def dtproj_inputs(c):
    rng = np.random.default_rng(c["seed"])
    M, dim, R, reg = c["M"], c["dim"], c["R"], c["regime"]
    x = np.full((M, c["pitch"]), np.nan)
    x[:, :R] = rng.standard_normal((M, R))
    w = rng.standard_normal((dim, R)) * R ** -0.5 * {"benign": 0.5, "long": 0.3}.get(reg, 1.0)
    bias = {"benign": 0.5 * rng.random(dim), "long": -4.2 + 0.3 * rng.standard_normal(dim)}.get(reg, rng.standard_normal(dim) - 3.0)
    if reg == "edges":
        w[:12] *= 0.25
        for sl, v in EDGE_BIAS:
            bias[sl] = v
    return dict(x=round_to(x, c["kind"]), w=round_to(w, c["kind"]), bias=bias.astype(np.float32) if c["bias"] else None)


def dtproj_reference(c, inp, dt=np.float64):
    pre = inp["x"][:, :c["R"]].astype(dt) @ inp["w"].astype(dt).T
    if inp["bias"] is not None:
        pre = pre + inp["bias"].astype(dt)
    return dict(pre=pre, delta=zo.softplus(pre) if c["softplus"] else pre)
