"""Cases and the numpy restatement of the 16-bit training-step tail (zigma_amd.optim.FusedAdamW16, zigma_optim16_* of include/zigma_hip.h).  Pure numpy:
no GPU, no library.  The arithmetic is that of tests/optim_cases.py (its float64 oracle, its float32 op-by-op evaluation, its error multiples) on bf16
parameters and gradients; what is new is restated here bit for bit:

    bits16     the 16 random bits of every element: Philox4x32-10 (tests/sde_cases.py) on counter (i >> 3, pid, step, stream), key (seed_lo, seed_hi);
               element i & 7 = j takes word j >> 1, low half for even j, high half for odd j
    sr_bf16    (u + r) >> 16 on the float32 bits u, inf / NaN by round-to-nearest
    rne_bf16   round to nearest even, the bits of from_float<BF16> and of torch's `.to(torch.bfloat16)`"""
import numpy as np

import optim_cases as oc
import sde_cases as sc

SENTINEL = oc.SENTINEL
NAN16 = 0x7FC1                                     # the fill of the bf16 buffers: a NaN no rounding produces
ROW_WORDS = 10                                     # int64 words of a zigma_optim16_row_t
NEAREST = 1                                        # ZIGMA_OPTIM16_NEAREST
STREAMS = ("p", "g", "m", "v", "ema")
WIDTH = {"p": 2, "g": 2, "m": 4, "v": 4, "ema": 4}  # bytes per element


# ---- the rounding and its bits --------------------------------------------------------------------------------------------------------------------------
def bits16(n, seed, pid, step, stream):
    """-> n uint16: the random bits of elements 0 ... n - 1 of parameter `pid` at `step`"""
    o = np.arange(-(-n // 8), dtype=np.uint64)
    ctr = np.stack([o & np.uint64(0xffffffff), np.full_like(o, pid & 0xffffffff), np.full_like(o, step), np.full_like(o, stream)], -1)
    w = sc.philox4x32_10(ctr, (seed & 0xffffffff, seed >> 32)).reshape(-1, 4)
    return np.stack([w & np.uint32(0xffff), w >> np.uint32(16)], -1).reshape(-1)[:n].astype(np.uint16)


def _u32(x32):
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    return x32.view(np.uint32)


def rne_bf16(x32):
    """float32 -> the bf16 bits of round-to-nearest-even; a NaN keeps its sign and high payload and is made quiet"""
    u = _u32(x32).astype(np.uint64)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(np.asarray(x32, dtype=np.float32))
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def sr_bf16(x32, bits):
    """the header's rule: exponent field all ones -> rne_bf16; else (u + r) >> 16"""
    u = _u32(x32)
    special = (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    r = ((u.astype(np.uint64) + np.asarray(bits).astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)
    return np.where(special, rne_bf16(x32), r)


def widen(b16):
    """bf16 bits -> float32 (exact)"""
    return (np.asarray(b16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16(x32):
    return widen(rne_bf16(x32))


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------------------------
def sweep_values(seed, first):
    """optim_cases.sweep_values with p and g rounded to bf16 first (float32 arrays that hold bf16 values)"""
    rows = oc.sweep_values(seed, first)
    for r in rows:
        r["p"], r["g"] = round_bf16(r["p"]), round_bf16(r["g"])
    return rows


def row_features(i):
    """(has_ema, aligned, the stream an unaligned row misplaces): the last 3 x 12 rows sit on 16-byte boundaries in every stream, the others misplace ONE
    present stream: a bf16 stream by 1 ... 7 elements, a float32 stream by 1 ... 3"""
    has_ema = i % 5 != 3
    aligned = i >= len(oc.SIZES) * 11
    present = ["p", "g", "m", "v"] + (["ema"] if has_ema else [])
    return has_ema, aligned, present[i % len(present)]


def sweep_layout(rows):
    """windows of every row in five buffers: p and g as uint16 (bf16 bits, NAN16-filled), m, v, ema as float32 (NaN-filled).  -> (buffers, wins: per row
    dict(name -> first element, "n": length; None for an absent stream)).  The hooks' windows are the p windows of two further buffers of p's length."""
    at = {k: 0 for k in STREAMS}
    wins = []
    for i, r in enumerate(rows):
        n = len(r["p"])
        has_ema, aligned, off_stream = row_features(i)
        w = {"n": n}
        for k in STREAMS:
            if k == "ema" and not has_ema:
                w[k] = None
                continue
            q = 16 // WIDTH[k]                                # elements per 16 bytes
            off = 0 if aligned or k != off_stream else 1 + i % (q - 1)
            w[k] = -(-at[k] // q) * q + q + off
            at[k] = w[k] + n + 3
        wins.append(w)
    bufs = {}
    for k in STREAMS:
        q = 16 // WIDTH[k]
        size = -(-at[k] // q) * q + 2 * q
        if WIDTH[k] == 2:
            b = np.full(size, NAN16, dtype=np.uint16)
        else:
            b = np.full(size, np.nan, dtype=np.float32)
        for r, w in zip(rows, wins):
            if w[k] is not None:
                b[w[k]:w[k] + w["n"]] = rne_bf16(r[k]) if WIDTH[k] == 2 else r[k]
        bufs[k] = b
    return bufs, wins


_K = {}


def error_constant(name):
    """K of config `name` (optim_cases.CONFIGS) as optim_cases.error_constant derives it, on THIS sweep's inputs: twice the worst error multiple of the
    numpy float32 evaluation against the float64 oracle.  Never from the kernel.  -> (K, the multiples per stream)"""
    if name not in _K:
        cfg = oc.CONFIGS[name]
        rows = sweep_values(1 + cfg["step0"], cfg["step0"] == 0)
        mult = np.float32(oc.clip_coef(oc.grad_norm64([r["g"] for r in rows]), cfg["max_norm"]))
        kw = dict(step=cfg["step0"] + 1, wd=cfg["wd"], grad_mult=float(mult), **oc.HYPER)
        worst = {}
        for r in rows:
            if not len(r["p"]):
                continue
            old = (r["p"], r["m"], r["v"], r["ema"])
            ref = oc.oracle_step(r["p"], r["g"], r["m"], r["v"], r["ema"], **kw)
            got = oc.step_f32(r["p"], r["g"], r["m"], r["v"], r["ema"], **kw)
            for k, x in oc.error_multiples(got, ref, old, r["g"].astype(np.float64) * float(mult)).items():
                worst[k] = max(worst.get(k, 0.0), x)
        _K[name] = (2.0 * max(worst.values()), worst)
    return _K[name]


# ---- the stalled update: 4096 parameters equal to 1.0 -----------------------------------------------------------------------------------------------------
STALL = dict(n=4096, p0=1.0, g=0.5, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, ema_decay=0.9999, steps=256, seed=2024)


def stall_sigma():
    """-> (sigma of the mean of p over the n elements after `steps` steps of stochastic rounding, the float64 displacement of p).  Every element sees the
    same gradient, so m, v and with them each step's decrement d_t are the same for all (float64 oracle below).  p starts at 1.0 and falls: from the first
    step on x = p - d_t lies in [0.5, 1), where bf16's spacing is ulp = 2^-8, p sits on that grid, and x is rounded away from zero with probability
    1 - f_t, f_t = d_t / ulp (d_t < ulp).  Each rounding is an independent two-point variable of variance f_t (1 - f_t) ulp^2; the steps add up along an
    element, the elements are independent: var(mean) = sum_t f_t (1 - f_t) ulp^2 / n."""
    c = STALL
    ulp = 2.0 ** -8
    p = np.float64(c["p0"])
    m = v = np.float64(0.0)
    var = 0.0
    for t in range(1, c["steps"] + 1):
        p_new, m, v, _ = oc.oracle_step(p, c["g"], m, v, None, step=t, lr=c["lr"], beta1=c["beta1"], beta2=c["beta2"], eps=c["eps"], wd=c["wd"], ema_decay=c["ema_decay"])
        d = float(p - p_new)
        assert 0.0 < d < ulp and 0.5 + ulp < p_new < 1.0
        f = d / ulp
        var += f * (1.0 - f) * ulp * ulp
        p = p_new
    return float(np.sqrt(var / c["n"])), float(c["p0"] - p)


# ---- the distance to the fp32 trajectory: 65 536 small weights ----------------------------------------------------------------------------------------------
DIST = dict(n=65536, std=0.02, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, steps=256, seed=7, data_seed=11)


def dist_inputs():
    """-> (weights N(0, 0.02^2) rounded to bf16, one gradient per element with a sign of its own that persists over all steps (the same tensor every step),
    magnitudes |N(0, 1)| x 1e-3 + 1e-4 rounded to bf16): float32 arrays that hold bf16 values"""
    rng = np.random.RandomState(DIST["data_seed"])
    w = round_bf16((rng.standard_normal(DIST["n"]) * DIST["std"]).astype(np.float32))
    g = round_bf16((rng.choice([-1.0, 1.0], DIST["n"]) * (np.abs(rng.standard_normal(DIST["n"])) * 1e-3 + 1e-4)).astype(np.float32))
    return w, g


def dist_simulation(steps=None, pid=0):
    """float32 AdamW arithmetic (optim_cases.step_f32) with three write-backs of the parameter — float32, round-to-nearest bf16, stochastic rounding with
    bits16 — from the same inputs.  -> (rms distance of nearest to float32, rms distance of stochastic to float32)"""
    c = DIST
    w, g = dist_inputs()
    z = np.zeros_like(w)
    runs = {k: [w.copy(), z.copy(), z.copy()] for k in ("f32", "rne", "sr")}
    for t in range(1, (steps or c["steps"]) + 1):
        kw = dict(step=t, lr=c["lr"], beta1=c["beta1"], beta2=c["beta2"], eps=c["eps"], wd=c["wd"], ema_decay=0.0)
        for k, st in runs.items():
            x, st[1], st[2], _ = oc.step_f32(st[0], g, st[1], st[2], None, **kw)
            st[0] = x if k == "f32" else round_bf16(x) if k == "rne" else widen(sr_bf16(x, bits16(c["n"], c["seed"], pid, t, 0)))
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - runs["f32"][0].astype(np.float64)) ** 2)))
    return rms(runs["rne"][0]), rms(runs["sr"][0])
