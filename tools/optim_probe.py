#!/usr/bin/env python
"""The tail of a training step alone: clip + AdamW + EMA + shadow refresh on the README model's parameter set (E = 640, depth 18,
has_text) with random gradients, HIP events around blocks of steps, one row appended to a .jsonl file (default profiles/optim_step_probe.jsonl).

    python tools/optim_probe.py [--out FILE] [--reps 7] [--steps 20]
    python tools/optim_probe.py --params bf16          # the pure bf16 model's tail, default profiles/optim16_probe.jsonl

own     zigma_amd.optim.FusedAdamW(max_grad_norm, ema_params, shadows): three launches
torch   clip_grad_norm_ + torch.optim.AdamW(fused=True) + _foreach EMA (mul_, add_) + amp refresh (one zigma_multi_cast_fwd launch) on tensors of the same
        sizes in the same process
--params bf16:
own     zigma_amd.optim.FusedAdamW16(max_grad_norm, ema=True): three launches, bf16 parameters written with stochastic rounding, fp32 moments and EMA
torch   clip_grad_norm_ + torch.optim.AdamW(fused=True) + _foreach EMA, all on bf16 tensors (bf16 moments, a bf16 EMA copy)
The two are timed alternately, `reps` blocks of `steps` steps each after a warm-up of both; min / median / max per step are reported, and the bytes each
path must move over its time beside the 1 GiB copy rate of bench.py's box_calib.  There is no threshold: the ratio is written down as it falls."""
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "optim_step_probe.jsonl")
OUT16 = os.path.join(ROOT, "profiles", "optim16_probe.jsonl")
CFG = dict(in_channels=3, img_dim=32, embed_dim=640, depth=18, patch_size=1, has_text=True, d_context=768, n_context_token=77, scan_type="zigzagN8", use_pe=2)


def main():
    import torch
    from zigma_amd import _lib, amp, optim
    from zigma_amd.model_zigma import ZigMa
    args = sys.argv[1:]
    opt_arg = lambda name, default: type(default)(args[args.index(name) + 1]) if name in args else default
    bf16 = opt_arg("--params", "fp32") == "bf16"
    out, reps, steps = os.path.abspath(opt_arg("--out", OUT16 if bf16 else OUT)), opt_arg("--reps", 7), opt_arg("--steps", 20)
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_probe.py needs a GPU (a time is measured on the device or not at all)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    kw = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    max_norm, decay, d16 = 2.0, 0.9999, torch.bfloat16

    def side():
        torch.manual_seed(0)
        m = ZigMa(device=dev, dtype=d16 if bf16 else torch.float32, **CFG)
        ema = copy.deepcopy(m)
        grp = None
        if not bf16:
            grp = amp.attach(m)
            grp.refresh(d16)
        g = torch.Generator(device=dev).manual_seed(1)
        for p in m.parameters():
            p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-2).to(p.dtype)
        return m, ema, grp

    m_own, ema_own, grp_own = side()
    m_ref, ema_ref, grp_ref = side()
    if bf16:
        del ema_own
        own = optim.FusedAdamW16(m_own.parameters(), max_grad_norm=max_norm, ema=True, ema_decay=decay, **kw)
    else:
        own = optim.FusedAdamW(m_own.parameters(), max_grad_norm=max_norm, ema_params=ema_own, ema_decay=decay, shadows=(m_own, d16), **kw)
    ref = torch.optim.AdamW(m_ref.parameters(), fused=True, **kw)
    ps_ref, es_ref = list(m_ref.parameters()), list(ema_ref.parameters())

    def step_own():
        own.step()

    def step_ref():
        torch.nn.utils.clip_grad_norm_(ps_ref, max_norm)
        ref.step()
        with torch.no_grad():
            torch._foreach_mul_(es_ref, decay)
            torch._foreach_add_(es_ref, ps_ref, alpha=1 - decay)
        if grp_ref is not None:
            grp_ref.refresh(d16)

    _lib.TRACE = []
    step_own()
    own_launches, _lib.TRACE = [t[1] for t in _lib.TRACE], None
    step_ref()
    for _ in range(5):
        step_own()
        step_ref()
    torch.cuda.synchronize()
    ms = {"own": [], "torch": []}
    for _ in range(reps):
        for name, fn in (("own", step_own), ("torch", step_ref)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / steps)
    # the copy rate of bench.py's box_calib (csrc/calib.hip, 1 GiB, read + write bytes over time)
    n = 1 << 30
    src, dst = torch.empty(n, device=dev, dtype=torch.uint8).fill_(1), torch.empty(n, device=dev, dtype=torch.uint8)
    P = _lib.CalibParams()
    P.mode, P.iters, P.bytes, P.src, P.dst = 0, 0, n, src.data_ptr(), dst.data_ptr()
    _lib.call("zigma_calib_launch", P, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        _lib.call("zigma_calib_launch", P, dev)
    e1.record()
    torch.cuda.synchronize()
    copy_gbps = 2 * n / (e0.elapsed_time(e1) * 1e-3 / 10) / 1e9
    n_all = sum(p.numel() for p in m_own.parameters())
    n_sh = 0 if bf16 else sum(grp_own.numels)
    # bytes each path must move: own = 4 (norm) + 36 per element + 2 per shadowed element; torch = 8 (clip: read, scale) + 28 (AdamW) + 12 (EMA: p read,
    # ema read and written; the two _foreach passes move 20) + 6 per shadowed element (cast)
    own_bytes, torch_bytes = 40 * n_all + 2 * n_sh, 48 * n_all + 6 * n_sh
    if bf16:
        # own = 2 (norm) + 16 read (p, g: 2 each; m, v, ema: 4 each) + 14 written (p: 2; m, v, ema: 4 each); torch, everything bf16 = 6 (clip: read, read and
        # scale) + 14 (AdamW: p, g, m, v read, p, m, v written) + 6 (EMA: p read, ema read and written)
        own_bytes, torch_bytes = 32 * n_all, 26 * n_all
    stat = lambda v: dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4))
    t_own, t_ref = statistics.median(ms["own"]), statistics.median(ms["torch"])
    row = dict(config="optim16_step_tail" if bf16 else "optim_step_tail", params="bf16" if bf16 else "fp32", model="README E=640 depth=18 has_text", tensors=len(ps_ref), elements=n_all, shadowed_elements=n_sh,
               own_launches=own_launches, steps_per_block=steps, blocks=reps, own_ms=stat(ms["own"]), torch_ms=stat(ms["torch"]),
               own_over_torch=round(t_own / t_ref, 4), own_bytes_MB=round(own_bytes / 1e6, 1), torch_min_bytes_MB=round(torch_bytes / 1e6, 1),
               copy_1GiB_GBps=round(copy_gbps, 1), own_GBps=round(own_bytes / (t_own * 1e-3) / 1e9, 1),
               own_fraction_of_copy_rate=round(own_bytes / (t_own * 1e-3) / 1e9 / copy_gbps, 4),
               torch_GBps_of_min_bytes=round(torch_bytes / (t_ref * 1e-3) / 1e9, 1), skipped=int(own.skipped), grad_norm=float(own.grad_norm),
               amp_stats=dict(amp.STATS), optim_stats=dict(optim.STATS))
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "a").write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
