#!/usr/bin/env python
"""Two builds of the library must run the training-step tail (zigma_optim_* and zigma_optim16_*, csrc/optim_step.hip) to the same bits.

    python tools/optim_tail_ab.py LIB_A LIB_B [--out FILE]

One fresh child process per library (ZIGMA_AMD_LIB) runs the same seeded launches through the ABI and prints a sha256 of every buffer it touched, whole
backing buffers with their margins, `partials`, the state block and the debug streams included.  The kernels are bit-identical from run to run, so LIB_A
against itself must give equal digests, and so must a refactored build against its parent.  One row is appended to FILE (default
profiles/optim_tail_merge_ab.jsonl); the exit status is 1 on any difference.

fp32: the 168 rows of tests/optim_cases.sweep_layout for every entry of CONFIGS (sizes 0 ... 3 x 4096 + 5, aligned and misaligned windows in NaN- and
      sentinel-filled buffers) x EMA on / off x shadows none / bf16 / f16, plus map rows outside the table.
bf16: the rows of tests/optim16_cases.sweep_layout for every entry of CONFIGS x EMA on / off x stochastic / nearest, both debug streams attached, plus a
      table row with a NULL stream, one above max_numel, a map row off the octet grid and map rows outside the table.
Each case: three steps in a row (the step counter reaches Philox), a step skipped by found_inf (fp32) or an inf gradient (bf16), a step with a NaN
gradient under the norm pass (skipped), and one without the norm pass, where the NaN goes through the update."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "optim_tail_merge_ab.jsonl")


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import optim16_cases as c16
    import optim_cases as oc
    from zigma_amd import _lib, amp
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)

    def digest(label, tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            raw = t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().tobytes()
            print(f"{label}/{k} {hashlib.sha256(raw).hexdigest()}", flush=True)

    def hyper(B, cfg, state, partials, n_entries, table, cmap, n_chunks):
        h = oc.HYPER
        B.table, B.chunk_map, B.n_entries, B.n_chunks = table.data_ptr(), cmap.data_ptr(), n_entries, n_chunks
        B.partials, B.state, B.chunk = _lib.ptr(partials), state.data_ptr(), oc.CHUNK
        B.lr, B.beta1, B.beta2, B.eps, B.weight_decay, B.max_grad_norm, B.ema_decay = h["lr"], h["beta1"], h["beta2"], h["eps"], cfg["wd"], cfg["max_norm"], h["ema_decay"]

    def run(label, bufs, state, partials, launch, poison, skip):
        """the case's launches; `launch(norm_pass)` is one step, `poison(value)` plants a non-finite gradient, `skip()` is a step something else skips"""
        everything = dict(bufs, state=state, partials=partials)
        step0, p0 = float(state[0]), bufs["p"].clone()
        counter = lambda: (float(state[0]) - step0, int(state.view(torch.int32)[1]))          # (steps taken, skipped)
        for i in (1, 2, 3):
            launch(True)
            digest(f"{label}/step{i}", everything)
        assert counter() == (3.0, 0) and not torch.equal(p0, bufs["p"]), label                 # (the launches ran and wrote)
        skip()
        digest(f"{label}/skipped", everything)
        assert counter() == (3.0, 1), label
        poison(float("nan"))
        launch(True)
        digest(f"{label}/nan_skipped", everything)
        assert counter() == (3.0, 1), label
        launch(False)
        digest(f"{label}/nan_taken", everything)
        assert counter() == (4.0, 0), label

    outside = [(-1, 0), (1 << 40, 0)]
    for name, cfg in oc.CONFIGS.items():
        rows = oc.sweep_values(1 + cfg["step0"], cfg["step0"] == 0)
        host, shadow_len, wins = oc.sweep_layout(rows)
        cm = amp.build_chunk_map([w["n"] for w in wins], oc.CHUNK)
        cmap = torch.tensor(cm[:40] + outside + cm[40:], dtype=torch.int64).to(dev)
        for with_ema in (True, False):
            for form, dt in (("none", None), ("bf16", torch.bfloat16), ("f16", torch.float16)):
                bufs = {k: up(host[k]) for k in oc.STREAMS}
                bufs["shadow"] = torch.full((shadow_len,), oc.SENTINEL, dtype=torch.int16, device=dev)
                addr = lambda w, k: 0 if w[k] is None or (k == "ema" and not with_ema) else bufs[k].data_ptr() + (2 if k == "shadow" else 4) * w[k]
                table = torch.tensor([[addr(w, k) for k in oc.STREAMS + ("shadow",)] + [w["n"], 0] for w in wins], dtype=torch.int64).to(dev)
                state = torch.zeros(8, device=dev)
                state[0] = float(cfg["step0"])
                partials = torch.full((len(cm) + 2,), float("nan"), device=dev)
                found = torch.zeros(1, device=dev)
                P = _lib.OptimParams()
                hyper(P, cfg, state, partials, len(wins), table, cmap, len(cm) + 2)
                P.found_inf, P.shadow_dtype, P.flags = found.data_ptr(), (-1 if dt is None else _lib._DT[dt]), 0

                def launch(norm_pass):
                    P.partials = partials.data_ptr() if norm_pass else None
                    for fn in ("zigma_optim_grad_sumsq", "zigma_optim_prepare", "zigma_optim_adamw")[0 if norm_pass else 1:]:
                        _lib.call(fn, P, dev)

                def skip():
                    found.fill_(1.0)
                    launch(True)
                    found.zero_()

                def poison(value):
                    bufs["g"][wins[-1]["g"] + wins[-1]["n"] - 3] = value

                run(f"fp32/{name}/{'ema' if with_ema else 'noema'}/{form}", bufs, state, partials, launch, poison, skip)

    for name, cfg in oc.CONFIGS.items():
        rows = c16.sweep_values(1 + cfg["step0"], cfg["step0"] == 0)
        host, wins = c16.sweep_layout(rows)
        numels = [w["n"] for w in wins]
        cm = amp.build_chunk_map(numels, oc.CHUNK)
        big = max(range(len(wins)), key=lambda i: numels[i])
        n = len(wins)
        # after the table's rows: row `big` again with a NULL v (row n) and with a numel above max_numel (row n + 1); a map row for each, one off the octet grid
        # of row `big`, and two outside the table
        extra = [(n, 0), (n + 1, 0), (big, 4)] + outside
        cmap = torch.tensor(cm[:40] + extra + cm[40:], dtype=torch.int64).to(dev)
        for with_ema in (True, False):
            for rounding, flags in (("sr", 0), ("nearest", _lib.OPTIM16_NEAREST)):
                bufs = {k: up(host[k]) for k in c16.STREAMS}
                bufs["dbg_x"] = torch.full((host["p"].size,), float("nan"), device=dev)
                bufs["dbg_b"] = torch.full((host["p"].size,), c16.SENTINEL, dtype=torch.int16, device=dev)
                addr = lambda w, k: 0 if w[k] is None or (k == "ema" and not with_ema) else bufs[k].data_ptr() + c16.WIDTH[k] * w[k]
                trows = [[addr(w, k) for k in c16.STREAMS] + [w["n"], 3 * i + 1, bufs["dbg_x"].data_ptr() + 4 * w["p"], bufs["dbg_b"].data_ptr() + 2 * w["p"], 0]
                         for i, w in enumerate(wins)]
                null_v, too_long = list(trows[big]), list(trows[big])
                null_v[3], too_long[5] = 0, numels[big] + 1
                table = torch.tensor(trows + [null_v, too_long], dtype=torch.int64).to(dev)
                state = torch.zeros(8, device=dev)
                state[0] = float(cfg["step0"])
                partials = torch.full((len(cm) + len(extra),), float("nan"), device=dev)
                P, Q = _lib.Optim16Params(), _lib.OptimParams()
                for B in (P, Q):
                    hyper(B, cfg, state, partials, n + 2, table, cmap, len(cm) + len(extra))
                P.max_numel, P.seed_lo, P.seed_hi, P.stream, P.flags = numels[big], 0x89abcdef, 0x01234567, 7, flags
                Q.shadow_dtype, Q.flags = -1, 0

                def launch(norm_pass):
                    Q.partials = partials.data_ptr() if norm_pass else None
                    if norm_pass:
                        _lib.call("zigma_optim16_grad_sumsq", P, dev)
                    _lib.call("zigma_optim_prepare", Q, dev)
                    _lib.call("zigma_optim16_adamw", P, dev)

                def poison(value):
                    bits = torch.tensor([value]).to(torch.bfloat16).view(torch.int16)[0]
                    bufs["g"][wins[-1]["g"] + wins[-1]["n"] - 3] = bits

                def skip():
                    poison(float("inf"))
                    launch(True)

                run(f"bf16/{name}/{'ema' if with_ema else 'noema'}/{rounding}", bufs, state, partials, launch, poison, skip)


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    out = os.path.abspath(argv[argv.index("--out") + 1]) if "--out" in argv else OUT
    if "--out" in argv:
        args.remove(argv[argv.index("--out") + 1])
    if len(args) != 2:
        sys.exit(__doc__)
    digests = []
    for lib in args:
        env = dict(os.environ, ZIGMA_AMD_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)      # a fresh process per library
        if r.returncode != 0:
            sys.exit(f"{lib}: the child ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        digests.append(dict(ln.split() for ln in r.stdout.strip().splitlines()))
    a, b = digests
    differing = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    whole = [hashlib.sha256("".join(f"{k} {d[k]}\n" for k in sorted(d)).encode()).hexdigest() for d in digests]
    row = dict(config="optim_tail_ab", lib_a=args[0], lib_b=args[1], buffers=len(a), cases=len({k.rsplit("/", 2)[0] for k in a}), differing=len(differing),
               first_differing=differing[:8], digest_a=whole[0], digest_b=whole[1], equal=not differing and len(a) > 0)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "a").write(json.dumps(row) + "\n")
    return 0 if row["equal"] else 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        sys.exit(main(sys.argv[1:]))
