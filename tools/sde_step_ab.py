#!/usr/bin/env python
"""What an SDE trajectory costs in its three modes: Sampler.sample_sde with the reference's CPU noise, with device noise (zigma_sde_step_fwd +
zigma_sde_advance, eager) and with device noise replayed as one captured graph per step — on the README model in bf16 with fp32 latents, in ONE
process, the modes alternating round by round (boxes and neighbours differ more than a step's arithmetic costs).

    python tools/sde_step_ab.py [--rounds 5 --steps 50 --batches 8 64 --out profiles/sde_step_ab.jsonl]

Modes, per batch size (50 Euler-Maruyama steps, sigma diffusion, "Mean" last step):
    reference           noise="reference", eager: th.randn on the CPU + a host-to-device copy inside every step, about fifteen eager launches around it
    reference_graphed   the same with zigma_amd.graphs.GraphedForward around the model (B = 8 only): the best the reference path can do
    device              noise="device", eager: the model, one zigma_sde_step_fwd, one zigma_sde_advance per step
    device_graph        noise="device", graph=True: one captured graph per step, replayed
and the step arithmetic alone on the same tensors, the model left out: `arith_device` (the combine + advance launches of one Euler-Maruyama step)
against `arith_torch` (the torch composition of integrators.sde._euler_maruyama_step with a ready model output and a ready increment on the
device: what remains of the reference's step once the CPU draw and the copy are taken away).
One JSON line per (round, batch, mode) with the milliseconds per trajectory, then a summary line with min / median / max per mode and bench.py's
box_calib.  Times are host clocks around whole trajectories that end in a device synchronise, after a warm-up of every mode.
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--arith-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sde_step_ab.py needs a GPU (the HIP path has no CPU fallback)")
    import bench
    from zigma_amd.graphs import GraphedForward
    from zigma_amd.transport import Sampler, create_transport
    from zigma_amd.transport import sde_device as sd
    device = torch.device("cuda", 0)
    wl = bench.WORKLOADS["readme_text_b64"]
    model = bench.build_model(wl["model"], device, torch.bfloat16)
    sampler = Sampler(create_transport())
    kw = dict(sampling_method="Euler", diffusion_form="sigma", last_step="Mean", num_steps=args.steps)
    modes = {}
    for B in args.batches:
        x, t, y = bench.make_inputs(wl, B, device, seed=1234)
        z = torch.randn(x.shape, generator=torch.Generator().manual_seed(B)).to(device)
        modes[(B, "reference")] = (sampler.sample_sde(**kw), model.forward, z, y)
        if B == min(args.batches):
            modes[(B, "reference_graphed")] = (sampler.sample_sde(**kw), GraphedForward(model.forward, z, t.float(), y), z, y)
        modes[(B, "device")] = (sampler.sample_sde(noise="device", seed=B, **kw), model.forward, z, y)
        modes[(B, "device_graph")] = (sampler.sample_sde(noise="device", seed=B, graph=True, **kw), model.forward, z, y)
    lines, times = [], {k: [] for k in modes}
    with torch.no_grad():
        for fn, m, z, y in modes.values():               # warm-up: every mode once (the graph modes capture here)
            assert bool(torch.isfinite(fn(z, m, y=y)[-1]).all())
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for (B, name), (fn, m, z, y) in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(z, m, y=y)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                times[(B, name)].append(ms)
                lines.append(dict(round=r, batch=B, mode=name, ms_per_trajectory=round(ms, 3), ms_per_step=round(ms / args.steps, 4), steps=args.steps))
                print(json.dumps(lines[-1]), flush=True)
        # the step arithmetic alone, on the tensors of a step
        arith = {}
        for B in args.batches:
            z = modes[(B, "device")][2]
            mo, xi = torch.randn_like(z), torch.randn_like(z)
            plan = sd.make_plan(sampler, **kw)
            coef, tms = torch.from_numpy(plan.coef).float().to(device), torch.from_numpy(plan.times).to(device)
            noise, tt, x = sd.DeviceNoise(1, 0, device), torch.empty(1, B, device=device), z.clone()
            drift, diffusion = sampler._sde_drift_and_diffusion(diffusion_form="sigma")
            tb, dt = torch.full((B,), 0.3, device=device), torch.tensor(0.02, device=device)

            def arith_device():
                sd.sde_step(x, x, mo, coef=coef, row=0, rows_per_step=1, state=noise.state)
                sd.sde_advance(noise.state, tms, tt)

            def arith_torch():                           # integrators.sde._euler_maruyama_step with the draw and the model taken out
                dw = xi * torch.sqrt(dt)
                d = drift(x, tb, lambda *_a, **_k: mo)
                mean_x = x + d * dt
                return mean_x + torch.sqrt(2 * diffusion(x, tb)) * dw
            for name, fn in (("arith_device", arith_device), ("arith_torch", arith_torch)):
                per = []
                for r in range(args.rounds):
                    noise.rewind()
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.arith_iters):
                        fn()
                    torch.cuda.synchronize()
                    per.append((time.perf_counter() - t0) / args.arith_iters * 1e3)
                arith[f"b{B}_{name}"] = dict(min=round(min(per), 4), median=round(statistics.median(per), 4), max=round(max(per), 4))
    summary = dict(summary={f"b{B}_{name}": dict(min=round(min(v), 3), median=round(statistics.median(v), 3), max=round(max(v), 3)) for (B, name), v in times.items()},
                   unit="ms per trajectory", step_arithmetic_ms_per_step=arith, steps=args.steps,
                   model="README model (E 640, depth 18, 32 x 32 tokens, text-conditional, bf16), fp32 latents; Euler-Maruyama, sigma diffusion, Mean last step",
                   box_calib=bench.box_calib(device))
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines + [summary]:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
