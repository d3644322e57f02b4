#!/usr/bin/env python
"""Measurements of mixed-precision training, rows appended to a .jsonl file (default profiles/amp_train_step.jsonl):

    python tools/amp_probe.py [--out FILE]          all of the below, one after the other
    python tools/amp_probe.py train                 ms per training step of the README model at B = 64 through tools/train.py, as alternating child
                                                    processes on one box, two rounds: (a) the bf16 model, (c) the fp32 model under autocast(bf16), (d) as (c)
                                                    with amp.USE_SHADOWS=False; then once (b) the fp32 model without autocast
    python tools/amp_probe.py cast                  zigma_multi_cast_fwd on that model's registered weights against a device-to-device copy_ of the same
                                                    traffic and against one .to() per tensor (HIP events around 20 calls, 5 repeats)
    python tools/amp_probe.py nograd                the no-grad forward under autocast: which kernels serve it, ms per forward beside the bf16 model"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "amp_train_step.jsonl")
CFG = dict(in_channels=3, img_dim=32, embed_dim=640, depth=18, patch_size=1, has_text=True, d_context=768, n_context_token=77, scan_type="zigzagN8", use_pe=2)


def train(tag, extra, knobs="", steps=15):
    env = dict(os.environ, ZIGMA_KNOBS=knobs)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--config", json.dumps(CFG), "--batch", "64", "--steps", str(steps), "--warmup", "4"] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    if r.returncode != 0:
        print(tag, "FAILED", r.returncode, r.stderr[-1500:], flush=True)
        return r.returncode
    row = dict(config=tag, **json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(row), flush=True)
    open(OUT, "a").write(json.dumps(row) + "\n")
    return 0


def cast_bench():
    import torch
    from zigma_amd import amp
    from zigma_amd.model_zigma import ZigMa
    m = ZigMa(device="cuda", dtype=torch.float32, **CFG)
    grp = amp.attach(m)
    n = sum(grp.numels)
    grp.refresh(torch.bfloat16)
    a = torch.empty(3 * n, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    res = {}
    for name, fn in (("multi_cast_bf16", lambda: grp.refresh(torch.bfloat16)), ("copy_dtod_same_traffic", lambda: b.copy_(a)),
                     ("per_tensor_to", lambda: [p.detach().to(torch.bfloat16) for p in grp.params])):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(5):
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 20 * 1e3)
        res[name] = dict(us_min=round(min(ts), 1), us_max=round(max(ts), 1))
    row = dict(config="cast_kernel", tensors=len(grp.params), elements=n, chunks=len(grp.cmap_rows), traffic_MB=round(6 * n / 1e6, 1),
               GBps_cast=round(6 * n / (res["multi_cast_bf16"]["us_min"] * 1e-6) / 1e9, 1), **res)
    print(json.dumps(row), flush=True)
    open(OUT, "a").write(json.dumps(row) + "\n")


def nograd_bench():
    import torch
    from zigma_amd import _lib, amp
    from zigma_amd.model_zigma import ZigMa
    torch.manual_seed(0)
    m32 = ZigMa(device="cuda", dtype=torch.float32, **CFG).eval()
    with torch.no_grad():
        for blk in m32.blocks:
            blk.adaLN_modulation[-1].weight.normal_(std=0.02)
            blk.adaLN_modulation[-1].bias.normal_(std=0.3)
    m16 = ZigMa(device="cuda", dtype=torch.bfloat16, **CFG).eval()
    m16.load_state_dict(m32.state_dict())
    x, t, y = torch.randn(64, 3, 32, 32, device="cuda"), torch.rand(64, device="cuda"), torch.rand(64, 77, 768, device="cuda")

    def fwd(model, cast):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=cast):
            return model(x, t, y)

    def ms(model, cast):
        for _ in range(5):
            fwd(model, cast)
        torch.cuda.synchronize()
        out = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(20):
                fwd(model, cast)
            torch.cuda.synchronize()
            out.append(round((time.perf_counter() - t0) / 20 * 1e3, 3))
        return out

    _lib.TRACE = []
    o_amp = fwd(m32, True)
    trace, _lib.TRACE = _lib.TRACE, None
    kern = {}
    for fn, k, _ in trace:
        kern[k] = kern.get(k, 0) + 1
    o16 = fwd(m16, False)
    with torch.no_grad():
        o32 = m32(x, t, y)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    row = dict(config="no_grad_forward_b64", kernels_under_autocast=kern, err_autocast_vs_fp32=rel(o_amp, o32), err_bf16_model_vs_fp32=rel(o16, o32),
               ms_bf16_model=ms(m16, False), ms_fp32_autocast=ms(m32, True), ms_bf16_model_again=ms(m16, False), amp_stats=dict(amp.STATS))
    print(json.dumps(row))
    open(OUT, "a").write(json.dumps(row) + "\n")


def train_bench():
    runs = [("a_bf16_model", ["--dtype", "bf16"], ""), ("c_fp32_autocast_bf16", ["--amp", "bf16"], ""), ("d_fp32_autocast_bf16_no_shadows", ["--amp", "bf16"], "amp.USE_SHADOWS=False")]
    for rnd in range(2):
        for tag, extra, knobs in runs:
            if train(tag, extra, knobs):
                return 1
    return train("b_fp32_model", ["--dtype", "fp32"], "", steps=6)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        OUT = os.path.abspath(args[args.index("--out") + 1])
        del args[args.index("--out"):args.index("--out") + 2]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    what = args[0] if args else "all"
    if what == "train":
        sys.exit(train_bench())
    if what == "cast":
        sys.exit(cast_bench())
    if what == "nograd":
        sys.exit(nograd_bench())
    for part in ("train", "cast", "nograd"):          # each in a process of its own
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), part, "--out", OUT], timeout=900).returncode
        if rc:
            sys.exit(rc)
