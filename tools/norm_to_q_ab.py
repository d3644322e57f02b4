"""The pre-attention LayerNorm + modulate + to_q as the two-kernel pair (zigma_add_norm_fwd, zigma_linear_fwd) against the fused kernel
(zigma_norm_linear_fwd), interleaved in one process at the block's shape — B x 1024 tokens, 640 -> 512, bf16, inputs resident — and the whole forward of
the README model with model_zigma.FUSE_NORM_TO_Q off and on, interleaved in the same process (the off path runs exactly the kernels of the pair).
HIP events around five back-to-back calls of a kernel (one repetition) and around every window of `--steps` forwards (default 20, bench.py's timed window); one JSON line per measurement into the file given with `--out` (default norm_to_q_ab.jsonl in the working
directory).  `--batch 32` / `--batch 16`: 32 768 / 16 384 tokens (the forward then runs the pair either way unless --min-tokens lowers the block's floor);
`--reps N` (default 30) kernel repetitions each, `--fwd-reps N` (default 7) timed windows each way,
The kernel figures are WARM (the same input five times over: it stays in the Infinity Cache); what decides the knob is the forward part. `--no-forward` skips the model part."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from zigma_amd import _lib
from zigma_amd.layernorm import block_norm
from zigma_amd.linear import linear
from zigma_amd.norm_linear import norm_linear

DEV = "cuda"


def timed(f, inner=1):
    """us per call: HIP events around `inner` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def stats(v):
    return dict(median=round(statistics.median(v), 2), mean=round(statistics.fmean(v), 2), stdev=round(statistics.stdev(v), 2), min=round(min(v), 2), max=round(max(v), 2), n=len(v))


def kernels(out, batch, reps):
    torch.manual_seed(0)
    L, E, N = 1024, 640, 512
    x = torch.randn(batch, L, E, device=DEV).bfloat16()
    w = (torch.randn(N, E, device=DEV) * E ** -0.5).bfloat16()
    mod = (torch.randn(batch, 6 * E, device=DEV) * 0.5).bfloat16()
    shift, scale = mod[:, 3 * E:4 * E], mod[:, 4 * E:5 * E]
    xa = torch.empty_like(x)
    q = torch.empty(batch * L, N, device=DEV, dtype=x.dtype)
    names = {}

    def norm():
        return block_norm(x, None, None, None, 1e-6, False, residual_in_fp32=False, shift=shift, scale=scale, want_x=True, want_y=False, want_res_out=False)[3]

    fs = {"add_norm": norm, "to_q": lambda: linear(xa, w, out=q), "fused": lambda: norm_linear(x, w, shift, scale, 1e-6, out=q)}
    xa.copy_(norm())
    for k, f in fs.items():
        f()
        names[k] = _lib.last_kernel()
    q_pair = linear(xa, w).float()
    q_fused = norm_linear(x, w, shift, scale, 1e-6).reshape(-1, N).float()
    t = {k: [] for k in fs}
    for _ in range(3):
        for f in fs.values():
            f()
    for _ in range(reps):
        for k, f in fs.items():
            t[k].append(timed(f, inner=5))
    pair = [a + b for a, b in zip(t["add_norm"], t["to_q"])]
    rec = dict(measurement="kernels", tokens=batch * L, k=E, n=N, rows_per_batch=L, dtype="bf16", served=names, us={k: stats(v) for k, v in t.items()}, pair_us=stats(pair),
               fused_over_pair=round(statistics.median(t["fused"]) / statistics.median(pair), 3),
               fused_vs_pair=float((q_fused - q_pair.reshape(-1, N)).norm() / q_pair.norm()))
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def forward(out, batch, reps, min_tokens, steps):
    import zigma_amd.model_zigma as mz
    wl = bench.WORKLOADS["readme_text_b64"]
    m = bench.build_model(wl["model"], DEV, torch.bfloat16)
    x, t, y = bench.make_inputs(wl, batch, DEV, 1234)
    if min_tokens is not None:
        mz.NORM_TO_Q_MIN_TOKENS = min_tokens

    def run(on):
        mz.FUSE_NORM_TO_Q = on
        trace = []
        _lib.TRACE = trace
        with torch.no_grad():
            o = m(x, t, y)
        _lib.TRACE = None
        return o, sum(1 for fn, _, _ in trace if fn == "zigma_norm_linear_fwd")

    def step(on):
        mz.FUSE_NORM_TO_Q = on
        with torch.no_grad():
            m(x, t, y)

    (o_on, n_on), (o_off, n_off) = run(True), run(False)
    for _ in range(3):
        step(False)
        step(True)
    ms = {"off": [], "on": []}
    for _ in range(reps):
        ms["off"].append(timed(lambda: step(False), inner=steps) / 1e3)
        ms["on"].append(timed(lambda: step(True), inner=steps) / 1e3)
    mz.FUSE_NORM_TO_Q = True
    st = lambda v: dict(mean=round(statistics.fmean(v), 4), stdev=round(statistics.stdev(v), 4), min=round(min(v), 4), max=round(max(v), 4), series=[round(a, 4) for a in v])
    gain = statistics.fmean(ms["off"]) - statistics.fmean(ms["on"])
    rec = dict(measurement="forward", model="README model bf16", batch=batch, tokens=batch * 1024, forwards_per_window=steps, fused_calls=dict(on=n_on, off=n_off), ms=dict(off=st(ms["off"]), on=st(ms["on"])),
               gain_ms=round(gain, 4), gain_over_stdev_off=round(gain / max(statistics.stdev(ms["off"]), 1e-9), 2), gain_percent=round(100 * gain / statistics.fmean(ms["off"]), 2),
               on_vs_off=float((o_on.float() - o_off.float()).norm() / o_off.float().norm()))
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fwd-reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="forwards per timed window of the forward part (bench.py's --steps)")
    ap.add_argument("--min-tokens", type=int, default=None, help="override model_zigma.NORM_TO_Q_MIN_TOKENS for the forward part")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default="norm_to_q_ab.jsonl")
    a = ap.parse_args()
    with open(a.out, "a") as fh:
        kernels(fh, a.batch, a.reps)
        if not a.no_forward:
            forward(fh, a.batch, a.fwd_reps, a.min_tokens, a.steps)
