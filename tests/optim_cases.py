"""Cases and the float64 oracle of the fused training-step tail (zigma_amd/optim.py, csrc/optim_step.hip).  Pure numpy: no GPU, no library.

The oracle states the formulas of include/zigma_hip.h, in float64:

    g = grad * grad_mult;  p -= lr * wd * p;  m += (g - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g * g
    p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps);  ema += (p - ema) * (1 - decay)

`step_f32` evaluates the same chain op by op in numpy float32 — one rounding per operation, in that order, the constants rounded to float32 from their
float64 values as the launcher does — and `error_constant` turns its distance from the oracle into the constant K the GPU sweep is held to."""
import numpy as np

CHUNK = 4096
SIZES = [0, 1, 7, 8, 9, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
SENTINEL = 0x5A5A
U = 2.0 ** -24                                     # unit roundoff of float32
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.999)
# the sweep's steps: first (m = v = 0, counter 0 -> 1) and later (counter preset to 1000), wd = 0 and > 0, clip inactive (max norm far above) and active
CONFIGS = {
    "first_nowd_noclip": dict(step0=0, wd=0.0, max_norm=1e9),
    "first_wd_clip": dict(step0=0, wd=0.05, max_norm=1.0),
    "later_wd_noclip": dict(step0=1000, wd=0.05, max_norm=1e9),
    "later_nowd_clip": dict(step0=1000, wd=0.0, max_norm=1.0),
}
STREAMS = ("p", "g", "m", "v", "ema")


def grad_norm64(gs):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in gs)))


def clip_coef(norm, max_norm):
    """the formula of torch's clip_grad_norm_; 1 when max_norm <= 0"""
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0


def oracle_step(p, g, m, v, ema, *, step, lr, beta1, beta2, eps, wd, ema_decay, grad_mult=1.0):
    """one step in float64; `step` is the counter AFTER its increment.  ema may be None.  Returns new (p, m, v, ema)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g * grad_mult
    p = p - lr * wd * p
    m = m + (g - m) * (1.0 - beta1)
    v = beta2 * v + (1.0 - beta2) * g * g
    step_size = lr / (1.0 - beta1 ** step)
    bc2_sqrt = np.sqrt(1.0 - beta2 ** step)
    p = p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps)
    if ema is not None:
        ema = np.asarray(ema, dtype=np.float64)
        ema = ema + (p - ema) * (1.0 - ema_decay)
    return p, m, v, ema


def step_f32(p, g, m, v, ema, *, step, lr, beta1, beta2, eps, wd, ema_decay, grad_mult=1.0):
    """the same chain, every operation rounded to float32 once"""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    lr_wd, omb1, b2, omb2, eps32, omd = f(lr * wd), f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps), f(1.0 - ema_decay)
    step_size, bc2_sqrt, mult = f(lr / (1.0 - beta1 ** step)), f(np.sqrt(1.0 - beta2 ** step)), f(grad_mult)
    g = g * mult
    p = p - lr_wd * p
    m = m + (g - m) * omb1
    v = b2 * v + (omb2 * g) * g
    p = p - (step_size * m) / (np.sqrt(v) / bc2_sqrt + eps32)
    if ema is not None:
        ema = np.asarray(ema, dtype=f)
        ema = ema + (p - ema) * omd
    assert all(a.dtype == f for a in (p, m, v))
    return p, m, v, ema


def error_multiples(got, ref, old, g_eff):
    """per stream, the worst |got - ref| as a multiple of 2^-24 times the stream's scale: p: |p_old| + |dp|, m: |m_old| + |g|, v: v_old + g^2,
    ema: |ema_old| + |p_new| (g: the gradient the update saw, grad * grad_mult).  got / ref: (p, m, v, ema) after the step; old: before it."""
    (gp, gm, gv, ge), (rp, rm, rv, re), (op, om, ov, oe) = got, ref, old
    d = lambda a: np.asarray(a, dtype=np.float64)
    g_eff = d(g_eff)
    scales = {"p": np.abs(d(op)) + np.abs(rp - d(op)), "m": np.abs(d(om)) + np.abs(g_eff), "v": d(ov) + g_eff * g_eff}
    pairs = {"p": (gp, rp), "m": (gm, rm), "v": (gv, rv)}
    if re is not None:
        scales["ema"] = np.abs(d(oe)) + np.abs(rp)
        pairs["ema"] = (ge, re)
    out = {}
    for k, (a, b) in pairs.items():
        err, sc = np.abs(d(a) - b), scales[k] * U
        assert np.all(np.isfinite(err)), k
        assert np.all(err[sc == 0] == 0), k                    # (a zero scale: every term of the update is zero, the result exact)
        out[k] = float(np.max(err[sc > 0] / sc[sc > 0])) if np.any(sc > 0) else 0.0
    return out


def sweep_values(seed, first):
    """per row of the sweep, float32 (p, g, m, v, ema) with magnitudes that neither overflow nor underflow in fp32: |p| in 10^[-4, 1], |g| around a
    per-row 10^[-6, 3], m and v what such gradients leave behind (zero on a first step)"""
    rng = np.random.RandomState(seed)
    rows = []
    for n in SIZES * 14:
        gs = 10.0 ** rng.uniform(-6, 3)
        p = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32)
        g = (rng.standard_normal(n) * gs).astype(np.float32)
        m = np.zeros(n, np.float32) if first else (rng.standard_normal(n) * 0.3 * gs).astype(np.float32)
        v = np.zeros(n, np.float32) if first else ((0.05 + rng.uniform(0, 1, n)) * gs * gs).astype(np.float32)
        ema = (p * (1 + 0.01 * rng.standard_normal(n))).astype(np.float32)
        rows.append(dict(p=p, g=g, m=m, v=v, ema=ema))
    return rows


def row_features(i):
    """(has_ema, has_shadow, aligned, the stream an unaligned row misplaces): the last 3 x 12 rows sit on 16-byte boundaries in every stream (the
    8-elements-per-lane path and its tail), the others misplace one present stream by 1 ... 3 elements (element by element)"""
    has_ema, has_shadow = i % 5 != 3, i % 7 != 2
    aligned = i >= len(SIZES) * 11
    present = ["p", "g", "m", "v"] + (["ema"] if has_ema else []) + (["shadow"] if has_shadow else [])
    return has_ema, has_shadow, aligned, present[i % len(present)]


def sweep_layout(rows):
    """windows of every row in six buffers: five float32 ones (NaN-filled) and the 16-bit shadows' (sentinel-filled).  -> (buffers: name -> float32
    array, shadow buffer length, wins: per row dict(name -> first element) with the row's length under "n" and None for an absent stream)"""
    at = {k: 0 for k in STREAMS + ("shadow",)}
    wins = []
    for i, r in enumerate(rows):
        n = len(r["p"])
        has_ema, has_shadow, aligned, off_stream = row_features(i)
        w = {"n": n}
        for k in STREAMS + ("shadow",):
            if (k == "ema" and not has_ema) or (k == "shadow" and not has_shadow):
                w[k] = None
                continue
            q = 8 if k == "shadow" else 4                   # elements per 16 bytes
            off = 0 if aligned or k != off_stream else (1 + 2 * (i % 4) if k == "shadow" else 1 + i % 3)
            w[k] = -(-at[k] // q) * q + q + off
            at[k] = w[k] + n + 3
        wins.append(w)
    bufs = {}
    for k in STREAMS:
        b = np.full(-(-at[k] // 4) * 4 + 16, np.nan, dtype=np.float32)
        for r, w in zip(rows, wins):
            if w[k] is not None:
                b[w[k]:w[k] + w["n"]] = r[k]
        bufs[k] = b
    return bufs, -(-at["shadow"] // 8) * 8 + 16, wins


def flat(rows, wins, k):
    """stream k of all rows that have it, concatenated (float64)"""
    return np.concatenate([np.asarray(r[k], dtype=np.float64) for r, w in zip(rows, wins) if w[k] is not None] or [np.zeros(0)])


_K = {}


def error_constant(name):
    """K of config `name`: twice the worst error multiple of the float32 evaluation against the oracle on the sweep's own inputs (twice: room for fma
    contraction and another legal order of the operations).  Computed from numpy alone, never from the kernel.  -> (K, the multiples per stream)"""
    if name not in _K:
        cfg = CONFIGS[name]
        rows = sweep_values(1 + cfg["step0"], cfg["step0"] == 0)
        mult = np.float32(clip_coef(grad_norm64([r["g"] for r in rows]), cfg["max_norm"]))
        kw = dict(step=cfg["step0"] + 1, wd=cfg["wd"], grad_mult=float(mult), **HYPER)
        worst = {}
        for r in rows:
            if not len(r["p"]):
                continue
            old = (r["p"], r["m"], r["v"], r["ema"])
            ref = oracle_step(r["p"], r["g"], r["m"], r["v"], r["ema"], **kw)
            got = step_f32(r["p"], r["g"], r["m"], r["v"], r["ema"], **kw)
            for k, x in error_multiples(got, ref, old, r["g"].astype(np.float64) * float(mult)).items():
                worst[k] = max(worst.get(k, 0.0), x)
        _K[name] = (2.0 * max(worst.values()), worst)
    return _K[name]
