"""Weight gradients dW = dY^T X of the block's projections at the headline training shape (M = B L = 65536 rows contracted): one library GEMM
against a batched GEMM over S row slabs (split-K by the library's batch dimension) + an fp32 sum of the S partial products.

`--own-ab [--out FILE]`: the own split-K kernel (zigma_linear_wgrad, wgrad.OWN_WGRAD="all") against the slab-bmm path (OWN_WGRAD=False) for the six
products at 65 536 and 16 384 tokens (and the two skinny ones at 4096 and 512), bf16: device events, warm-up, batches of 50 launches, the two
versions alternating in ONE process, 5 batches each (min / median / max = the spread of repeated identical runs); dt_proj's x is the 72-pitch
column view of x_dbl for the own kernel, and the bmm side is timed with the .contiguous() copy it needs.  Also sweeps forced slab counts for the
own kernel.  One JSON line per point (the rows of wgrad.PLAN_TABLE quote them)."""
import json, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def own_ab(out_path):
    import statistics
    from zigma_amd import _lib, wgrad as wg
    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    sink = open(out_path, "w") if out_path else None

    def batch_us(fn, n=50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    def stats(v):
        return dict(min=round(min(v), 2), med=round(statistics.median(v), 2), max=round(max(v), 2))

    shapes = (("in_proj", 2560, 640, 0), ("out_proj", 640, 1280, 0), ("to_q", 512, 640, 0), ("to_out", 640, 512, 0), ("x_proj", 72, 1280, 0), ("dt_proj", 1280, 40, 72))
    for M in (65536, 16384, 4096, 512):
        for name, N, K, pitch in shapes:
            if M < 16384 and name not in ("x_proj", "dt_proj"):
                continue
            dy = torch.randn(M, N, device=dev, dtype=dt)
            xw = torch.randn(M, pitch or K, device=dev, dtype=dt)
            x = xw[:, :K]

            def own(slabs=0):
                return wg.wgrad_own(dy, x, slabs=slabs)

            def bmm():
                wg.OWN_WGRAD = False
                r = wg.wgrad(dy, x if x.is_contiguous() else x.contiguous())
                wg.OWN_WGRAD = True
                return r

            a, b = own(), bmm()
            kern = _lib.last_kernel()
            for _ in range(5):
                own(), bmm()
            t_own, t_bmm = [], []
            for _ in range(5):
                t_own.append(batch_us(own))
                t_bmm.append(batch_us(bmm))
            ws = wg.wgrad_workspace_bytes(M, N, K, dt)
            rec = dict(product=name, tokens=M, n=N, k=K, dtype="bf16", x_pitch=pitch or K, own_us=stats(t_own), bmm_us=stats(t_bmm),
                       own_slabs=ws // (4 * N * K) if ws else 1, bmm_slabs=wg._slabs(M, N, K), launches_per_batch=50, batches=5,
                       relerr_own_vs_bmm=float((a.float() - b.float()).norm() / b.float().norm()))
            sweep = {}
            for S in (4, 8, 16, 32, 64, 128):
                if M // S < 64:
                    continue
                f = lambda S=S: own(S)
                f()
                sweep[S] = round(min(batch_us(f, 20) for _ in range(2)), 2)
            rec["own_forced_slabs_us"] = sweep
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
            del dy, xw, x


if "--own-ab" in sys.argv:
    own_ab(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
    sys.exit(0)
dev, dt = "cuda", torch.bfloat16
M = 65536
torch.manual_seed(0)
def timeit(fn, n=10):
    for _ in range(2): fn()
    torch.cuda.synchronize(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize(); return e0.elapsed_time(e1) / n * 1e3
for name, N, K in (("in_proj", 2560, 640), ("out_proj", 640, 1280), ("to_q", 512, 640), ("to_out", 640, 512), ("x_proj", 72, 1280), ("dt_proj", 1280, 40)):
    dy = torch.randn(M, N, device=dev, dtype=dt); x = torch.randn(M, K, device=dev, dtype=dt)
    ref = (dy.t() @ x)
    res = dict(shape=f"{name}: dW ({N} x {K}) = dY^T ({N} x {M}) X ({M} x {K})", GF=2.0 * M * N * K / 1e9, plain_us=timeit(lambda: dy.t() @ x))
    for S in (8, 16, 32, 64):
        f = lambda: torch.bmm(dy.view(S, M // S, N).transpose(1, 2), x.view(S, M // S, K)).sum(0, dtype=torch.float32).to(dt)
        out = f()
        res[f"split{S}_us"] = timeit(f)
        res[f"split{S}_relerr_vs_plain"] = float((out.float() - ref.float()).norm() / ref.float().norm())
    print(json.dumps(res), flush=True)
