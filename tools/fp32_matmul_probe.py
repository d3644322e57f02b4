"""fp32 projections as split bf16 products (zigma_amd/fp32_matmul.py, csrc/linear_split.hip) against F.linear in the same process:
  1. the four block projections of E = 640 and E = 768 at 8192 / 16 384 / 65 536 tokens — "library" (F.linear, fp32), "high" (three
     products) and "medium" (one), interleaved round by round (HIP events, medians), random operands, with the norm-wise error of each
     against float64 on 256 sampled rows;
  2. one fp32 forward of the README model at B = 64 in the three modes, with the distance of "high" / "medium" from "highest".
One JSON line per shape and one for the forward into the file given with `--out` (default: fp32_matmul_probe.jsonl in the working
directory).  `--no-forward` skips the model part."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import zigma_amd
from zigma_amd import _lib
from zigma_amd.fp32_matmul import linear_split

DEV = "cuda"


def timeit(fs, rounds=5, reps=5):
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
    for E in (640, 768):
        for name, n, k, bias in (("in_proj", 4 * E, E, False), ("out_proj", E, 2 * E, False), ("to_q", 512, E, False), ("to_out", E, 512, True)):
            w = torch.randn(n, k, device=DEV) * k ** -0.5
            b = torch.randn(n, device=DEV) * 0.3 if bias else None
            for tokens in (8192, 16384, 65536):
                x = torch.randn(tokens, k, device=DEV)
                y = torch.empty(tokens, n, device=DEV)
                fs = {"library": lambda: F.linear(x, w, b), "high": lambda: linear_split(x, w, b, mode="high", out=y),
                      "medium": lambda: linear_split(x, w, b, mode="medium", out=y)}
                rows = torch.randint(0, tokens, (256,), device=DEV)
                ref = x[rows].double() @ w.double().t() + (0 if b is None else b.double())
                err = {m: float((f()[rows].double() - ref).norm() / ref.norm()) for m, f in fs.items()}
                served = {}
                for m in ("high", "medium"):
                    fs[m]()
                    served[m] = _lib.last_kernel()
                us, spread = timeit(fs)
                tf = {m: round(2.0 * tokens * n * k / (v * 1e-6) / 1e12, 1) for m, v in us.items()}
                rec = dict(projection=name, E=E, tokens=tokens, n=n, k=k, bias=bias, served=served, us=us, min_max_us=spread, tflops=tf,
                           high_over_library=round(us["high"] / us["library"], 3), medium_over_library=round(us["medium"] / us["library"], 3),
                           err_vs_float64={m: float(f"{v:.3e}") for m, v in err.items()})
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")


def forward(out):
    wl = bench.WORKLOADS["readme_text_b64"]
    m = bench.build_model(wl["model"], DEV, torch.float32)
    x, t, y = bench.make_inputs(wl, 64, DEV, 0)
    x, t, y = x.float(), t.float(), y.float()

    def run(mode):
        zigma_amd.set_float32_matmul_precision(mode)
        try:
            with torch.no_grad():
                return m(x, t, y)
        finally:
            zigma_amd.set_float32_matmul_precision("highest")

    modes = ("highest", "high", "medium")
    o = {md: run(md) for md in modes}
    us, spread = timeit({md: (lambda md=md: run(md)) for md in modes}, rounds=5, reps=2)
    ref = o["highest"].double()
    rec = dict(forward="README model fp32 B=64 (65 536 tokens)", ms={k: round(v / 1e3, 3) for k, v in us.items()},
               min_max_ms={k: [round(a / 1e3, 3), round(b / 1e3, 3)] for k, (a, b) in spread.items()},
               high_over_highest=round(us["high"] / us["highest"], 3), medium_over_highest=round(us["medium"] / us["highest"], 3),
               finite={md: bool(torch.isfinite(o[md]).all()) for md in modes},
               distance_from_highest={md: float(f"{float((o[md].double() - ref).norm() / ref.norm()):.3e}") for md in ("high", "medium")})
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "fp32_matmul_probe.jsonl"
    with open(path, "w") as fh:
        kernels(fh)
        if "--no-forward" not in sys.argv:
            forward(fh)
