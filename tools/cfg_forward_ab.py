#!/usr/bin/env python
"""What a guided evaluation costs: ZigMa.forward_guided at B = 32 (64 samples through the blocks) against the plain forward at B = 64 — the same
block work — on the README model, in ONE process, the variants alternating round by round (boxes and neighbours differ more than the head costs).

    python tools/cfg_forward_ab.py [--rounds 5 --steps 20 --out profiles/cfg_forward_ab.jsonl]

Variants, each eager and replayed as a hipGraph (zigma_amd.graphs.GraphedForward):
    plain_b64        model.forward, B = 64
    guided_b32       forward_guided, scale 4, the guided final-layer kernel (zigma_final_layer_cfg_fwd)
    guided_b32_torch the same with embed.USE_EMBED_KERNELS = False: the torch composition final_layer -> unpatchify -> cast -> combine.  The knob
                     switches EVERY kernel of zigma_amd/embed.py to torch (patch embedding, timestep features, the skinny projections, the final
                     layer), so this column is not the head alone.
One JSON line per (round, variant) with the milliseconds per evaluation, then a summary line with the min / median / max per variant and bench.py's
box_calib.  Times are host clocks around `steps` evaluations that end in a device synchronise, after a warm-up of every variant.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cfg_forward_ab.py needs a GPU (the HIP path has no CPU fallback)")
    import bench
    from zigma_amd import embed
    from zigma_amd.graphs import GraphedForward
    from zigma_amd.guidance import Guided
    device = torch.device("cuda", 0)
    wl = bench.WORKLOADS["readme_text_b64"]
    model = bench.build_model(wl["model"], device, torch.bfloat16)
    x, t, y = bench.make_inputs(wl, 64, device, seed=1234)
    x, xh, th, yh = x.float(), x[:32].float(), t[:32], y[:32]          # (the samplers' fp32 state: the fp32 form of the head)
    guided = Guided(model, args.scale, y_null=torch.zeros_like(yh))

    def with_knob(value, fn):
        def run(*a):
            old, embed.USE_EMBED_KERNELS = embed.USE_EMBED_KERNELS, value
            try:
                return fn(*a)
            finally:
                embed.USE_EMBED_KERNELS = old
        return run
    eager = {"plain_b64": (model.forward, (x, t, y)), "guided_b32": (guided, (xh, th, yh)), "guided_b32_torch": (with_knob(False, guided), (xh, th, yh))}
    variants = {}
    with torch.no_grad():
        for name, (fn, a) in eager.items():
            variants[name] = (fn, a)
            variants[name + "_graph"] = (GraphedForward(fn, *a), a)          # (captured through the variant's own knob setting; a replay reads no knob)
        for fn, a in variants.values():
            for _ in range(args.warmup):
                fn(*a)
        torch.cuda.synchronize()
        d = (variants["guided_b32"][0](xh, th, yh) - variants["guided_b32_torch"][0](xh, th, yh)).float().norm() / variants["guided_b32"][0](xh, th, yh).float().norm()
        lines, times = [], {k: [] for k in variants}
        for r in range(args.rounds):
            for name, (fn, a) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn(*a)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / args.steps * 1e3
                times[name].append(ms)
                lines.append(dict(round=r, variant=name, ms_per_eval=round(ms, 4), steps=args.steps))
                print(json.dumps(lines[-1]), flush=True)
    summary = dict(summary={k: dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4)) for k, v in times.items()},
                   model="README model (E 640, depth 18, 32 x 32 tokens, text-conditional, bf16), fp32 latents", scale=args.scale,
                   kernel_vs_torch_composition_rel=float(d), box_calib=bench.box_calib(device),
                   note="guided_b32_torch: embed.USE_EMBED_KERNELS=False switches every kernel of zigma_amd/embed.py to torch, not the head alone")
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines + [summary]:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
