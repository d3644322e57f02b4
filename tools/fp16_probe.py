"""fp16 against bf16 for every matrix-core kernel family at the headline shapes (65 536 tokens), and one fp16 forward of the README model at
B = 64 on the own kernels against the library-served fp16 forward (every fp16 gate closed: routing.POLICY = "off", the five predicates False).
One process, the two dtypes interleaved round by round (HIP events, medians), random operands.  One JSON line per kernel and one for the
forward into the file given with `--out` (default: fp16_probe.jsonl in the working directory).  `--no-forward` skips the model part."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from zigma_amd import _lib
from zigma_amd.attention import cross_attn
from zigma_amd.linear import linear
from zigma_amd.selective_scan_interface import conv_x_proj

DEV = "cuda"
DTS = {"bf16": torch.bfloat16, "f16": torch.float16}


def timeit(fs, rounds=7, reps=10):
    t = {k: [] for k in fs}
    for f in fs.values():
        f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) / reps * 1e3)
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in t.items()}, {k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()}


def kernels(out):
    torch.manual_seed(0)
    M, B, L = 65536, 64, 1024
    cases = []
    mk = lambda *s, sc=1.0: torch.randn(*s, device=DEV) * sc
    for name, K, N, kw, epi in (("in_proj 640->2560 ws", 640, 2560, dict(weight_stationary=True), None),
                                ("in_proj 640->2560 ws + silu", 640, 2560, dict(weight_stationary=True, silu_from_col=1280), None),
                                ("out_proj 1280->640 + add 4w", 1280, 640, {}, "res"), ("to_q 640->512 4w", 640, 512, {}, None),
                                ("to_out 512->640 + bias + add 4w", 512, 640, {}, "bias+res"),
                                ("out_proj 1280->640 8w", 1280, 640, dict(_probe_flags=0x2000), None)):
        x32, w32 = mk(B, L, K), mk(N, K, sc=K ** -0.5)
        b32, r32, g32 = mk(N, sc=0.3), mk(B, L, N), mk(B, N)
        fs, kern = {}, {}
        for tag, dt in DTS.items():
            x, w = x32.to(dt), w32.to(dt)
            b = b32.to(dt) if epi and "bias" in epi else None
            r, g = (r32.to(dt), g32.to(dt)) if epi and "res" in epi else (None, None)
            fs[tag] = (lambda x=x, w=w, b=b, r=r, g=g: linear(x, w, b, residual=r, gate=g, **kw))
            fs[tag]()
            kern[tag] = _lib.last_kernel()
        cases.append((name, fs, kern))
    Di, Nn = 1280, 72
    xz32, cw32, cb32, xw32 = mk(B, L, 2 * Di), mk(Di, 4, sc=0.4), mk(Di, sc=0.1), mk(Nn, Di, sc=Di ** -0.5)
    perm = torch.randperm(L, device=DEV).to(torch.int32)
    fs = {}
    for tag, dt in DTS.items():
        xz, cw, cb, xw = xz32.to(dt), cw32.to(dt), cb32.to(dt), xw32.to(dt)
        fs[tag] = (lambda xz=xz, cw=cw, cb=cb, xw=xw: conv_x_proj(xz[:, :, :Di], cw, cb, xw, perm))
    cases.append(("conv_x_proj Di=1280 n=72", fs, {k: "conv_x_proj_mfma" for k in DTS}))
    q32, kv32 = mk(B, L, 512), mk(B, 77, 2, 512)
    fs = {}
    for tag, dt in DTS.items():
        q, kv = q32.to(dt), kv32.to(dt)
        fs[tag] = (lambda q=q, kv=kv: cross_attn(q, kv[:, :, 0], kv[:, :, 1], 8))
    cases.append(("cross_attn 8 x 64, 77 keys", fs, {k: "cross_attn_mfma" for k in DTS}))
    for name, fs, kern in cases:
        us, spread = timeit(fs)
        rec = dict(kernel=name, served=kern, us=us, min_max_us=spread, f16_over_bf16=round(us["f16"] / us["bf16"], 3))
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")


def forward(out):
    import zigma_amd.linear as zl
    import zigma_amd.model_zigma as mz
    import zigma_amd.routing as zr
    import zigma_amd.selective_scan_interface as ssi
    wl = bench.WORKLOADS["readme_text_b64"]
    H = torch.float16
    m = bench.build_model(wl["model"], DEV, H)
    x, t, y = bench.make_inputs(wl, 64, DEV, 0)
    x, t, y = x.to(H), t.to(H), y.to(H)
    saved = (zr.POLICY, zl.linear_eligible, ssi.x_proj_eligible, ssi.conv_x_proj_eligible, ssi.dt_proj_eligible, mz.cross_attn_eligible)
    no = lambda *a, **k: False

    def gates(closed):
        if closed:
            zr.POLICY, zl.linear_eligible, ssi.x_proj_eligible, ssi.conv_x_proj_eligible, ssi.dt_proj_eligible, mz.cross_attn_eligible = "off", no, no, no, no, no
        else:
            zr.POLICY, zl.linear_eligible, ssi.x_proj_eligible, ssi.conv_x_proj_eligible, ssi.dt_proj_eligible, mz.cross_attn_eligible = saved

    def run(closed):
        gates(closed)
        try:
            with torch.no_grad():
                return m(x, t, y)
        finally:
            gates(False)

    o_own, o_lib = run(False), run(True)
    us, spread = timeit({"own": lambda: run(False), "library": lambda: run(True)}, rounds=5, reps=3)
    rec = dict(forward="README model fp16 B=64 (65 536 tokens)", ms={k: round(v / 1e3, 3) for k, v in us.items()},
               min_max_ms={k: [round(a / 1e3, 3), round(b / 1e3, 3)] for k, (a, b) in spread.items()},
               own_over_library=round(us["own"] / us["library"], 3), finite=[bool(torch.isfinite(o_own).all()), bool(torch.isfinite(o_lib).all())],
               own_vs_library=float((o_own.float() - o_lib.float()).norm() / o_lib.float().norm()))
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "fp16_probe.jsonl"
    with open(path, "w") as fh:
        kernels(fh)
        if "--no-forward" not in sys.argv:
            forward(fh)
