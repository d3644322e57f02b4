#!/usr/bin/env python
"""Training loop of the reference's train_acc.py (train_acc.py:426-448: flow-matching loss, AdamW) on the MI355X-native
model — synthetic latents, no dataloader / EMA / wandb.  Forward AND backward run on the HIP kernels
(LayerNormFn, MambaInnerTokFn); the projections, attention and optimizer are torch.

    python tools/train.py --config '{...}' --batch 32 --steps 20
    python tools/train.py --config '{...}' --amp bf16 --fused-step --max-grad-norm 2.0      # the step's tail on the own kernels
    python tools/train.py --config '{..., "num_classes": 1000}' --class-dropout 0.1          # label dropout: a model that can be guided

--fused-step: the reference's `opt.step()` / `grad_clip` / `update_ema` (train_acc.py:443-448) as zigma_amd.optim.FusedAdamW — AdamW, global-norm
clipping (before the update), an EMA copy of the model and, under --amp, the 16-bit shadows in one pass, three launches, no host sync.  With a pure
bf16 model (--dtype bf16, no --amp) it is zigma_amd.optim.FusedAdamW16: fp32 moments, an fp32 EMA inside the optimizer and the bf16 parameters written
back with stochastic rounding (--rounding, --opt-seed; every rank passes the same seed, so the replicas stay bit-identical).  Without the flag the
loop is what it was: torch.optim.AdamW(fused=True), no EMA, no clipping.
    python tools/train.py --config '{...}' --dtype bf16 --fused-step --max-grad-norm 2.0      # bf16 parameters, stochastic rounding
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 tools/train.py ...   # data parallel

Multi-GPU = plain data parallelism: one process per GPU, `--batch` samples per rank, gradients averaged by
DistributedDataParallel's bucketed all-reduce (RCCL over xGMI), which torch overlaps with the backward."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--amp", default="off", choices=["off", "bf16", "fp16"],
                    help="mixed precision: the model is fp32 (whatever --dtype says) and the step runs under torch.autocast in this type; fp16 with a GradScaler")
    ap.add_argument("--fused-step", action="store_true", help="AdamW + clip + EMA on the own kernels: zigma_amd.optim.FusedAdamW for an fp32 model (--amp or --dtype fp32, with the shadow refresh), "
                                                               "zigma_amd.optim.FusedAdamW16 for a pure bf16 model")
    ap.add_argument("--rounding", default="stochastic", choices=["stochastic", "nearest"], help="--fused-step with a bf16 model: how the parameter is written back")
    ap.add_argument("--opt-seed", type=int, default=0, help="--fused-step with a bf16 model: seed of the rounding bits (the same on every rank)")
    ap.add_argument("--wd", type=float, default=None, help="weight decay (default: the optimizer's own, 1e-2)")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="--fused-step: clip the global gradient norm to this before the update")
    ap.add_argument("--ema-decay", type=float, default=0.9999, help="--fused-step: decay of the EMA copy")
    ap.add_argument("--time-tail", action="store_true", help="--fused-step: HIP events around every optimizer step (adds no sync inside the loop)")
    ap.add_argument("--class-dropout", type=float, default=None, metavar="P",
                    help="class-conditional models: drop the label to the null class with probability P (ZigMa class_dropout_prob; the model can then be guided: "
                         "tools/sample.py --cfg-scale)")
    ap.add_argument("--bucket-mb", type=int, default=100, help="DDP bucket size: xGMI rings are per-link bound, few large buckets")
    args = ap.parse_args()

    from zigma_amd import amp
    from zigma_amd import sharded_sampling as ss
    from zigma_amd.model_zigma import ZigMa
    from zigma_amd.transport import create_transport
    if not torch.cuda.is_available():
        raise SystemExit("tools/train.py needs a GPU (the HIP path has no CPU fallback)")
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    rank, world, _ = ss.init_from_env(backend="nccl", device=device)
    cfg = json.loads(args.config)
    if args.class_dropout is not None:
        if not cfg.get("num_classes", -1) > 0:
            raise SystemExit("tools/train.py: --class-dropout needs a class-conditional model (num_classes in --config)")
        cfg["class_dropout_prob"] = args.class_dropout
    torch.manual_seed(0)
    mdtype = torch.float32 if args.amp != "off" else torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model = ZigMa(device=device, dtype=mdtype, **cfg).train()
    cast = torch.autocast("cuda", dtype=torch.bfloat16 if args.amp == "bf16" else torch.float16, enabled=args.amp != "off")
    scaler = torch.amp.GradScaler("cuda", enabled=args.amp == "fp16")
    net = model
    if world > 1:
        net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local_rank], bucket_cap_mb=args.bucket_mb,
                                                        gradient_as_bucket_view=True)
    wd = {} if args.wd is None else dict(weight_decay=args.wd)
    ema = None
    if args.fused_step:
        import copy
        from zigma_amd import optim
        if mdtype == torch.bfloat16:
            opt = optim.FusedAdamW16(model.parameters(), lr=args.lr, max_grad_norm=args.max_grad_norm, ema=True, ema_decay=args.ema_decay, rounding=args.rounding,
                                     seed=args.opt_seed, **wd)         # (the fp32 EMA lives in the optimizer: opt.copy_ema_to(a copy of the model) for sampling)
        else:
            ema = copy.deepcopy(model).requires_grad_(False)
            opt = optim.FusedAdamW(model.parameters(), lr=args.lr, max_grad_norm=args.max_grad_norm, ema_params=ema, ema_decay=args.ema_decay,
                                   shadows=(model, torch.float16 if args.amp == "fp16" else torch.bfloat16) if args.amp != "off" else None, **wd)
    else:
        if args.max_grad_norm is not None or args.time_tail:
            raise SystemExit("tools/train.py: --max-grad-norm and --time-tail go with --fused-step")
        opt = torch.optim.AdamW(model.parameters(), lr=args.lr, fused=True, **wd)
    tr = create_transport()
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    frames = cfg.get("video_frames", 0)
    shape = ((frames,) if frames else ()) + (cfg["in_channels"], cfg["img_dim"], cfg["img_dim"])
    x1 = torch.randn((args.batch,) + shape, generator=g).to(device)
    kw = {}
    if cfg.get("has_text"):
        kw["y"] = torch.rand(args.batch, cfg["n_context_token"], cfg["d_context"], generator=g).to(device, model.x_embedder.proj.weight.dtype)
    elif cfg.get("num_classes", -1) > 0:
        kw["y"] = torch.randint(0, cfg["num_classes"], (args.batch,), generator=g).to(device)

    tail_events = []

    def step():
        opt.zero_grad(set_to_none=not args.fused_step)      # (FusedAdamW keeps its device table while the gradients stay where they are)
        with cast:
            loss = tr.training_losses(net, x1, kw)["loss"].mean()
        scaler.scale(loss).backward()          # (a disabled scaler passes the loss and the step through)
        if args.time_tail:
            tail_events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            tail_events[-1][0].record()
        scaler.step(opt)
        if args.time_tail:
            tail_events[-1][1].record()
        scaler.update()
        return loss

    losses = []
    for _ in range(args.warmup):
        step()
    ss.fence(device, world)
    del tail_events[:]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(step().detach())
    ss.fence(device, world)
    dt = (time.perf_counter() - t0) / args.steps
    tail = dict(optimizer=type(opt).__name__)
    if args.fused_step:
        from zigma_amd import optim
        if isinstance(opt, optim.FusedAdamW16):
            tail.update(rounding=args.rounding, opt_seed=args.opt_seed)
        tail.update(fused_step=True, step_tail_launches_per_step=optim.STATS["launches"] / max(optim.STATS["steps"], 1), step_tail_table_builds=optim.STATS["table_builds"],
                    last_step_skipped=int(opt.skipped), last_grad_norm=float(opt.grad_norm) if args.max_grad_norm is not None else None, max_grad_norm=args.max_grad_norm, ema_decay=args.ema_decay)
        if tail_events:
            tail["step_tail_ms"] = round(sum(a.elapsed_time(b) for a, b in tail_events) / len(tail_events), 4)
    if rank == 0:
        print(json.dumps(dict(world=world, per_gpu_batch=args.batch, ms_per_step=round(dt * 1e3, 2),
                              samples_per_s=round(world * args.batch / dt, 1), first_loss=round(float(losses[0]), 4),
                              last_loss=round(float(losses[-1]), 4), max_mem_GB=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                              amp=args.amp, amp_stats=dict(amp.STATS), use_shadows=amp.USE_SHADOWS, **tail)))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
