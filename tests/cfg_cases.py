"""Case table of the guided final layer, zigma_final_layer_cfg_fwd (csrc/embed.hip): LayerNorm + projection of a (conditional, unconditional)
row pair, v_u + s (v_c - v_u) on the fp32 accumulators, one rounding, stored in the unpatchified latent layout.

Plain numpy, importable without a GPU, in the style of outer_fwd_cases.py, whose final_inputs / final_reference make the operands and the
float64 LayerNorm + projection of each half.  cfg_cases() yields dicts of PARAMETERS with stable ids; cfg_inputs(case) makes the numbers from
the case's seed, already rounded to bf16; cfg_reference(case, inputs, y_own=None) evaluates in float64 on those rounded operands, with the
LayerNorm output rounded to bf16 where the ABI rounds it (or, y_own given, on the kernel's / the model's OWN bf16 LayerNorm rows: the staged check
of the forward sweep's 16-bit delta), and writes the result into the latent layout with numpy's reshape + transpose of `unpatchify` /
`unpatchify_video` — not with the kernel's index formula.  cfg_model() is the fp32 step-by-step model, cfg_composed() the composition the kernel
replaces (each half rounded to bf16 before the combination).  tests/test_cfg_cases_cpu.py checks the table, tests/test_gpu_cfg.py runs the kernel.

Limits: IO_BOUND[out dtype] norm-wise; rowwise (a row = one pixel row of the latent) <= ROW_GUARD with terms = ((1 - s) v_u, s v_c), the two
summands that can cancel.  No case runs on a raised bound.
"""
import numpy as np

import outer_fwd_cases as oc
from outer_fwd_cases import DELTA_FLIPS, DELTA_FLIPS_MODEL, IO_BOUND, ROW_GUARD, elementwise_worst, flipped_share, need, norm_err, round_to, row_ratio  # noqa: F401

CFG_COLS = (8, 72, 128, 640, 648, 768, 1032, 2048)           # <5>: <= 640, <8>: <= 1024, <16>: the three instantiations
CFG_PC = ((1, 1), (1, 3), (1, 4), (2, 3), (2, 4), (4, 1), (1, 15))          # (patch, chans): n_out = 1, 3, 4, 12, 16, 16, 15
CFG_SIDE = (1, 3, 4, 5)                                      # tokens per row and column of a frame
CFG_FRAMES = (0, 1, 3)                                       # 0: an image (B, C, H, W); T: a video (B, T, C, H, W)
CFG_BATCH = (1, 2, 3)
CFG_SCALES = (-1.0, 0.0, 1.0, 1.5, 4.0, 7.5)
CFG_HIGH = (4.0, 7.5)                                        # the cases whose every scale is >= 4: where the composed path leaves the bf16 bound
CFG_LONG = dict(cols=64, patch=1, chans=3, side=257, frames=0, batch=1)          # 66 049 rows per half: the second trip of the row loop (4096 workgroups x 16 rows)
CFG_EPS = oc.FL_EPS
# Outputs of a few elements: one 16-bit rounding can cost up to 2^-9 of an element, more than the norm-wise bound, which one rounding meets only on
# average.  For these cases the rounded float64 reference itself missed the bound: they run on another seed (outer_fwd_cases.SEED_MOVED).
SEED_MOVED = {}


def _case(table, **kw):
    c = dict(kernel="cfg", regime="benign", seed=27000 + len(table))
    c.update(kw)
    c["n_out"] = c["patch"] ** 2 * c["chans"]
    c["rps"] = max(c["frames"], 1) * c["side"] ** 2           # rows per sample
    c["rows"] = c["batch"] * c["rps"]                         # rows of each half
    c["np"] = 5 if c["cols"] <= 640 else 8 if c["cols"] <= 1024 else 16
    c["id"] = (f"e{c['cols']}-p{c['patch']}c{c['chans']}-g{c['side']}-{'t%d' % c['frames'] if c['frames'] else 'img'}-b{c['batch']}-{c['out']}"
               f"-{'b' if c['bias'] else ''}-s{'_'.join('%g' % s for s in c['scales'])}-{c['regime']}")
    c["seed"] = SEED_MOVED.get(c["id"], c["seed"])
    table.append(c)


def _scales(i, batch, high):
    pool = CFG_HIGH if high else CFG_SCALES
    return tuple(pool[(i + 5 * k) % len(pool)] if not high else pool[(i + k) % 2] for k in range(batch))


def cfg_cases():
    """Keys: cols, patch, chans, side, frames, batch, out ("f32" | "bf16"), bias, scales (one per sample), regime (oc.FL_REGIMES without the constant
    rows), n_out, rps, rows, np (the instantiation), seed.  Every third case draws all its scales from CFG_HIGH."""
    out, i = [], 0
    for cols in CFG_COLS:
        for patch, chans in CFG_PC:
            batch = CFG_BATCH[(i + i // 3) % 3]
            high = i % 3 == 2
            _case(out, cols=cols, patch=patch, chans=chans, side=CFG_SIDE[(i + i // 4) % 4] if not high else CFG_SIDE[1 + (i // 3) % 3], frames=CFG_FRAMES[(i + i // 7) % 3],
                  batch=batch, out=("f32", "bf16")[(i + i // 14) % 2] if not high else "bf16", bias=i % 4 != 1, scales=_scales(i, batch, high),
                  regime=("benign", "mean50")[(i // 5) % 2])
            i += 1
    _case(out, out="bf16", bias=True, scales=(4.0,), **CFG_LONG)
    _case(out, out="f32", bias=False, scales=(-1.0,), **CFG_LONG)
    return out


def cfg_inputs(c):
    """x_c from outer_fwd_cases.final_inputs; x_u = x_c + fresh noise of about a quarter of its spread (correlated halves: v_c - v_u is small against
    either, which is where guidance amplifies a rounding).  All bf16 values held in float32."""
    inp = oc.final_inputs(c)
    rng = np.random.default_rng(c["seed"] + 500_000)
    xu = inp["x"] + np.float32(0.4) * rng.standard_normal(inp["x"].shape, dtype=np.float32)
    return dict(x_c=inp["x"], x_u=round_to(xu, "bf16"), w=inp["w"], bias=inp["bias"], scale=np.asarray(c["scales"], np.float32))


def unpatchify(c, rows):
    """(batch * rps, n_out) -> (B, C, H, W) | (B, T, C, H, W): reshape + transpose, the permutation of ZigMa.unpatchify / unpatchify_video"""
    B, T, g, p, ch = c["batch"], c["frames"], c["side"], c["patch"], c["chans"]
    if T:
        return rows.reshape(B, T, g, g, p, p, ch).transpose(0, 1, 6, 2, 4, 3, 5).reshape(B, T, ch, g * p, g * p)
    return rows.reshape(B, g, g, p, p, ch).transpose(0, 5, 1, 3, 2, 4).reshape(B, ch, g * p, g * p)


def _row_scale(c, inp, dt):
    return inp["scale"].astype(dt).repeat(c["rps"])[:, None]


def layer_norms(c, inp, dt=np.float64):
    """the UNROUNDED LayerNorm rows of both halves, (2 rows, cols), cond rows first"""
    return np.concatenate([oc.final_reference(c, dict(x=inp[k], w=inp["w"], bias=None), dt)["y"] for k in ("x_c", "x_u")], 0)


def cfg_reference(c, inp, y_own=None):
    """float64 -> dict(y: unrounded LayerNorm rows (2 rows, cols), out: the guided result in the latent layout, terms: ((1 - s) v_u, s v_c) in the
    same layout).  y_own (2 rows, cols): bf16 LayerNorm rows to project instead of the correctly rounded ones."""
    dt = np.float64
    y = layer_norms(c, inp)
    yb = round_to(y.astype(np.float32), "bf16").astype(dt) if y_own is None else np.asarray(y_own, dt)
    v = yb @ inp["w"].astype(dt).T
    if inp["bias"] is not None:
        v = v + inp["bias"].astype(dt)
    vc, vu = v[:c["rows"]], v[c["rows"]:]
    s = _row_scale(c, inp, dt)
    a, b = (1.0 - s) * vu, s * vc
    return dict(y=y, out=unpatchify(c, a + b), terms=(unpatchify(c, a), unpatchify(c, b)))


def _f32_halves(c, inp):
    """the fp32 step-by-step model up to the accumulators: statistics, normalisation and dot products in fp32, the LayerNorm output rounded to bf16"""
    f = np.float32
    y = round_to(layer_norms(c, inp, f), "bf16")
    v = y @ inp["w"].astype(f).T
    if inp["bias"] is not None:
        v = v + inp["bias"].astype(f)
    return y, v[:c["rows"]], v[c["rows"]:]


def cfg_model(c, inp):
    """-> (y: its bf16 LayerNorm rows, out: fma(s, vc - vu, vu) on the fp32 accumulators, rounded ONCE to the case's output type, in the layout)"""
    y, vc, vu = _f32_halves(c, inp)
    d = (vc - vu).astype(np.float32)
    out = (_row_scale(c, inp, np.float64) * d.astype(np.float64) + vu.astype(np.float64)).astype(np.float32)        # (the product is exact in float64: an fma)
    return y, round_to(unpatchify(c, out), c["out"])


def cfg_composed(c, inp):
    """what the torch composition computes: each half's velocity rounded to bf16, cast to the output type, then v_u + s (v_c - v_u) in that type"""
    _, vc, vu = _f32_halves(c, inp)
    vc, vu, s = round_to(vc, "bf16"), round_to(vu, "bf16"), _row_scale(c, inp, np.float32)
    r = lambda a: round_to(a, c["out"])
    return unpatchify(c, r(vu + r(s * r(vc - vu))))


def out_window(c):
    """(buffer shape, window index) of the NaN-filled buffer `out` is a window of: row pitch W + 5, one more pixel row per channel, one more channel
    per frame / sample: row, channel, (frame) and sample strides are all non-compact"""
    B, T, ch, hw = c["batch"], c["frames"], c["chans"], c["side"] * c["patch"]
    lead = (B,) + ((T,) if T else ())
    return lead + (ch + 1, hw + 1, hw + 5), tuple(slice(0, n) for n in lead) + (slice(0, ch), slice(0, hw), slice(2, 2 + hw))


# (what is wrong, status): the GPU test builds each from a small valid call; include/zigma_hip.h lists them in the order they are checked
REFUSALS = (("null-block", oc.ERR_NULL), ("rows-negative", oc.ERR_SHAPE), ("cols4", oc.ERR_SHAPE), ("n_out0", oc.ERR_SHAPE), ("flags1", -6),
            ("f16", oc.ERR_DTYPE), ("f32-in", oc.ERR_DTYPE), ("out-f16", oc.ERR_DTYPE), ("cols12", oc.ERR_SHAPE), ("cols2056", oc.ERR_SHAPE),
            ("n_out17", oc.ERR_SHAPE), ("patch0", oc.ERR_SHAPE), ("n_out-not-p2c", oc.ERR_SHAPE), ("rows-not-samples", oc.ERR_SHAPE),
            ("sample-not-frames", oc.ERR_SHAPE), ("frame-not-grid", oc.ERR_SHAPE), ("null-x_cond", oc.ERR_NULL), ("null-x_uncond", oc.ERR_NULL),
            ("null-weight", oc.ERR_NULL), ("null-scale", oc.ERR_NULL), ("null-out", oc.ERR_NULL), ("x-off-by-one", oc.ERR_STRIDE),
            ("x-pitch-odd", oc.ERR_STRIDE), ("weight-off-by-one", oc.ERR_STRIDE), ("y_out-off-by-one", oc.ERR_STRIDE))
