"""TEST-ONLY stand-ins for the three HIP entry points, backed by the CPU oracle, so that the host-side logic
of zigma_amd (layouts, row tables, pending-residual flow, module plumbing) can be exercised without a GPU.
Installed by monkeypatching inside tests; never imported by the product."""
import numpy as np
import torch

from oracle import zigma_oracle as zo


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _split(a, period):
    """(B, D, n * period) -> (B * n, D, period): the independent sequences a reset_period concatenates along seqlen."""
    Bn, D, Lt = a.shape
    return a.reshape(Bn, D, Lt // period, period).transpose(0, 2, 1, 3).reshape(-1, D, period)


def _join(a, Bn, period):
    D = a.shape[1]
    return a.reshape(Bn, -1, D, period).transpose(0, 2, 1, 3).reshape(Bn, D, -1)


def conv_raw(x, weight, bias, silu, *, out=None, x_row_index=None, reset_period=0):
    xs = _np(x)
    if x_row_index is not None:
        xs = xs[:, :, x_row_index.long().cpu().numpy()]
    if reset_period:
        y = _join(zo.causal_conv1d(_split(xs, reset_period), _np(weight), _np(bias), "silu" if silu else None),
                  xs.shape[0], reset_period)
    else:
        y = zo.causal_conv1d(xs, _np(weight), _np(bias), "silu" if silu else None)
    y = torch.from_numpy(np.ascontiguousarray(y)).to(x.dtype)
    if out is None:
        out = torch.empty_like(x)
    out.copy_(y)
    return out


def scan_raw(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, *, out=None, out_z=None,
             x=None, z_row_index=None, out_row_index=None, want_out=True, checkpoints=None, reset_period=0,
             chunk_len=2048, z_preactivated=False, info=None, dt_x=None, dt_w=None, accumulate=False):
    assert checkpoints is None and not z_preactivated and not accumulate, "stand-in: GPU-only features"
    if delta is None or dt_x is not None:             # ABI 9 / 10: dt_proj inside the scan (delta absent, or the split's workspace); (B, L, >= R) rows x (D, R) -> (B, D, L)
        delta = torch.einsum("blr,dr->bdl", dt_x[:, :, :dt_w.shape[1]].float(), dt_w.float()).to(u.dtype)
    if info is not None:
        info[:] = [2, 0]
    zs = _np(z)
    if zs is not None and z_row_index is not None:
        zs = zs[:, :, z_row_index.long().cpu().numpy()]
    if reset_period:                                  # independent sequences of reset_period steps along seqlen
        Bn, P = u.shape[0], reset_period
        bc = lambda M: _split(_np(M)[:, 0], P)[:, None]                     # (B, 1, N, L) -> (B * n, 1, N, P)
        y, last = zo.selective_scan(_split(_np(u), P), _split(_np(delta), P), _np(A), bc(B), bc(C), _np(D), None,
                                    _np(delta_bias), delta_softplus, return_last_state=True)
        y = np.ascontiguousarray(_join(y, Bn, P))
        assert x is None
    else:
        y, last = zo.selective_scan(_np(u), _np(delta), _np(A), _np(B), _np(C), _np(D), None, _np(delta_bias), delta_softplus,
                                    return_last_state=True)
    yz = y * zo.silu(zs) if zs is not None else None

    def place(arr):
        if out_row_index is None:
            return arr
        o = np.empty_like(arr)
        o[:, :, out_row_index.long().cpu().numpy()] = arr
        return o
    if z is not None:
        if out_z is None:
            out_z = torch.empty_like(z)
        out_z.copy_(torch.from_numpy(place(yz)).to(u.dtype))
    if out is None and (want_out or z is None):
        out = torch.empty_like(delta)
    if out is not None:
        out.copy_(torch.from_numpy(place(y)).to(u.dtype))
    if x is not None:
        x.zero_()
        x[:, :, -1, 1::2] = torch.from_numpy(last)
    return out, out_z


def norm_call(x2, weight, bias, residual2, eps, is_rms, residual_dtype, *, rows_per_batch=None, branch=None,
              gate=None, x_out=None, shift=None, scale=None, want_y=True, want_res=None):
    rows, cols = x2.shape
    rpb = rows_per_batch or max(rows, 1)
    rep = lambda m: _np(m).repeat(rpb, axis=0)[:rows]
    xe = _np(x2)
    if branch is not None:
        xe = (xe + rep(gate) * _np(branch)).astype(np.float32)
        xe = _np(torch.from_numpy(xe).to(x2.dtype))
        if x_out is not None:
            x_out.copy_(torch.from_numpy(xe).to(x2.dtype))
    y, res = zo.fused_add_norm(xe, _np(weight), _np(bias), _np(residual2), eps, True, is_rms)
    if residual2 is not None:
        residual_dtype = residual2.dtype
    if want_res is None:
        want_res = residual2 is not None or (residual_dtype is not None and residual_dtype != x2.dtype)
    res_out = torch.from_numpy(res).to(residual_dtype or x2.dtype) if want_res else None
    yt = torch.from_numpy(y).to(x2.dtype)
    y_mod = None
    if shift is not None:
        y_mod = (yt.float() * (1 + torch.from_numpy(rep(scale))) + torch.from_numpy(rep(shift))).to(x2.dtype)
    return (yt if want_y else None), res_out, y_mod


def install(monkeypatch):
    from zigma_amd import causal_conv1d_interface as cci
    from zigma_amd import layernorm as ln
    from zigma_amd import selective_scan_interface as ssi
    monkeypatch.setattr(cci, "causal_conv1d_raw", conv_raw)
    monkeypatch.setattr(ssi, "causal_conv1d_raw", conv_raw)
    monkeypatch.setattr(ssi, "scan_raw", scan_raw)
    monkeypatch.setattr(ln, "_norm_call", norm_call)


# ---------------------------------------------------------------------------------------------------
# Stand-ins AT THE C ABI for the forward Mamba-inner entry points: _lib.call(name, parameter block, device) served on CPU tensors by float64
# torch restatements that read and write through the block's pointers and strides, so that tests/test_gpu_fwd_fuzz.py (views, row tables,
# NaN surroundings, staged checks) can be exercised without a GPU.  torch_scan_fwd is also the independent restatement the CPU test holds
# the numpy reference of tests/fwd_fuzz_cases.py against.
# ---------------------------------------------------------------------------------------------------
import ctypes

LAST_KERNEL = [""]


def torch_scan_fwd(u, step, A, Bm, Cm, D, gate, zi, oi, *, reset=0, chunk=0, out_z0=None, kernel_decay=False):
    """The token-major selective scan as an explicit float64 loop over (sequence, chunk, step) with restarts.  u, step (B, L, dim): scan order,
    step = the step sizes the recurrence runs on; Bm, Cm (B, L, N); gate (B, L, dim) multiplier in TOKEN rows (read at row zi[k]) or None;
    results are written at row oi[k].  kernel_decay: the decay taken the kernels' way, exp2(step * fl32(A * log2 e)) — the same number to 1e-7,
    and exactly 0.5 for the known-answer cases' A.  Returns y (ungated, placed), y_gated (placed, + out_z0), ckpt (B, tile, dim, N): the state before every
    16-step tile, x_prod / x_state (B, chunk, dim, N): running decay product and state at every chunk end."""
    f64 = torch.float64
    decay = (lambda d: torch.exp2(d * (A.float() * 1.4426950408889634).to(f64))) if kernel_decay else (lambda d: torch.exp(d * A.to(f64)))
    u, step, A, Bm, Cm = (t.to(f64) for t in (u, step, A, Bm, Cm))
    Bsz, L, dim = u.shape
    N = A.shape[1]
    y = torch.empty(Bsz, L, dim, dtype=f64)
    ckpt = torch.zeros(Bsz, -(-L // 16), dim, N, dtype=f64)
    n_chunks = -(-L // chunk) if chunk else 0
    x_prod, x_state = torch.zeros(Bsz, n_chunks, dim, N, dtype=f64), torch.zeros(Bsz, n_chunks, dim, N, dtype=f64)
    period = reset or L
    for a in range(0, L, period):                                  # independent sequences
        end = min(a + period, L)
        h, cum = torch.zeros(Bsz, dim, N, dtype=f64), torch.zeros(Bsz, dim, dtype=f64)
        for c0 in range(a, end, chunk or period):                  # chunks of one sequence: the state carries over
            c1 = min(c0 + (chunk or period), end)
            for l in range(c0, c1):
                if l % 16 == 0:
                    ckpt[:, l // 16] = h
                d = step[:, l]
                h = decay(d[..., None]) * h + (d * u[:, l])[..., None] * Bm[:, l, None, :]
                cum = cum + d
                y[:, l] = (h * Cm[:, l, None, :]).sum(-1)
            if chunk:
                x_prod[:, (c1 - 1) // chunk], x_state[:, (c1 - 1) // chunk] = decay(cum[..., None]), h
    if D is not None:
        y = y + u * D.to(f64)
    place = lambda t: t if oi is None else torch.empty_like(t).index_copy_(1, oi.long(), t)
    y_gated = None
    if gate is not None:
        g = gate.to(f64)
        y_gated = place(y * (g if zi is None else g.index_select(1, zi.long())))
        if out_z0 is not None:
            y_gated = out_z0.to(f64) + y_gated
    return dict(y=place(y), y_gated=y_gated, ckpt=ckpt, x_prod=x_prod, x_state=x_state)


def torch_scan_ref_layout(u, step, A, Bm, Cm, D, gate, zi, oi, *, chunk=0):
    """The selective scan of the reference's call surface as an explicit float64 loop over (chunk, step).  u, step (B, dim, L), step = the step
    sizes the recurrence runs on; Bm, Cm (B, G, N, L) — channel d reads group d // (dim // G) — or constant (dim, N); gate (B, dim, L) multiplier
    read at row zi[l] or None; results are written at row oi[l].  Returns y (ungated, placed), y_gated (placed) and, with chunk > 0, x_prod /
    x_state (B, dim, chunk, N): the decay product since the start of the sequence and the state at every chunk end."""
    f64 = torch.float64
    u, step, A = u.to(f64), step.to(f64), A.to(f64)
    Bsz, dim, L = u.shape
    N = A.shape[1]

    def per_channel(M):         # -> (B | 1, dim, N, L | 1)
        M = M.to(f64)
        return M[None, :, :, None] if M.dim() == 2 else M.repeat_interleave(dim // M.shape[1], dim=1)
    Bm, Cm = per_channel(Bm), per_channel(Cm)
    at = lambda M, l: M[..., 0] if M.shape[-1] == 1 else M[..., l]
    y = torch.empty(Bsz, dim, L, dtype=f64)
    n_chunks = -(-L // chunk) if chunk else 0
    x_prod, x_state = torch.zeros(Bsz, dim, n_chunks, N, dtype=f64), torch.zeros(Bsz, dim, n_chunks, N, dtype=f64)
    h, prod = torch.zeros(Bsz, dim, N, dtype=f64), torch.ones(Bsz, dim, N, dtype=f64)
    for l in range(L):
        d = step[:, :, l, None]
        a = torch.exp(d * A)
        h = a * h + d * u[:, :, l, None] * at(Bm, l)
        prod = prod * a
        y[:, :, l] = (h * at(Cm, l)).sum(-1)
        if chunk and ((l + 1) % chunk == 0 or l == L - 1):
            x_prod[:, :, l // chunk], x_state[:, :, l // chunk] = prod, h
    if D is not None:
        y = y + u * D.to(f64)[:, None]
    place = lambda t: t if oi is None else torch.empty_like(t).index_copy_(2, oi.long(), t)
    y_gated = None
    if gate is not None:
        g = gate.to(f64)
        y_gated = place(y * (g if zi is None else g.index_select(2, zi.long())))
    return dict(y=place(y), y_gated=y_gated, x_prod=x_prod, x_state=x_state)


def torch_conv1d(x, w, b, silu, rows=None, reset=0):
    """the depthwise causal conv of the call surface, float64, tap by tap: x (B, dim, L) read at row rows[l], w (dim, W), b (dim,) | None; with
    reset > 0 the window restarts every `reset` positions"""
    x, w = x.double(), w.double()
    if rows is not None:
        x = x.index_select(2, rows.long())
    L, W = x.shape[2], w.shape[1]
    pos = torch.arange(L)
    start = pos // reset * reset if reset else torch.zeros(L, dtype=torch.long)
    y = torch.zeros_like(x) + (0 if b is None else b.double()[:, None])
    for j in range(W):
        k = pos - (W - 1 - j)
        ok = (k >= start).double()
        y = y + w[:, j, None] * x[:, :, k.clamp(min=0)] * ok
    return y * torch.sigmoid(y) if silu else y


def _view(ptr, shape, strides, dtype):
    """the tensor a parameter block describes: base pointer, shape and strides in elements"""
    if not ptr:
        return None
    n = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
    es = torch.empty((), dtype=dtype).element_size()
    buf = (ctypes.c_char * (n * es)).from_address(ptr)
    return torch.frombuffer(buf, dtype=dtype, count=n).as_strided(tuple(shape), tuple(strides))


def _io_dtype(i):
    from zigma_amd import _lib
    return {v: k for k, v in _lib._DT.items()}[i]


def _scan_fwd(P, plan):
    from zigma_amd import _lib
    f32, dt = torch.float32, _io_dtype(P.io_dtype)
    got = plan(P)
    if got["status"] != 0:
        raise RuntimeError(f"zigma_selective_scan_fwd: refused (status {got['status']})")
    if got["family"] == _lib.SCAN_KERNEL_GENERIC:
        return _scan_generic_fwd(P, got)
    Bsz, dim, L, N = P.batch, P.dim, P.seqlen, P.dstate
    act = lambda name: _view(getattr(P, name), (Bsz, L, dim), [getattr(P, f"{name}_{s}_stride") for s in ("batch", "l", "d")], dt)
    bc = lambda name: _view(getattr(P, name), (Bsz, L, N), [getattr(P, f"{name}_{s}_stride") for s in ("batch", "l", "dstate")], dt)
    A = _view(P.A, (dim, N), (P.A_d_stride, P.A_dstate_stride), f32)
    D, bias = _view(P.D, (dim,), (1,), f32), _view(P.delta_bias, (dim,), (1,), f32)
    u, z, delta = act("u"), act("z"), act("delta")
    if P.dt_x:
        R = P.dt_rank
        x = _view(P.dt_x, (Bsz, L, R), (P.dt_x_batch_stride, P.dt_x_l_stride, 1), dt)
        w = _view(P.dt_w, (dim, R), (P.dt_w_row_stride, 1), dt)
        pre = x.double() @ w.double().T
    else:
        pre = delta.double()
    if bias is not None:
        pre = pre + bias.double()
    step = _softplus(pre) if P.delta_softplus else pre
    if P.dt_x and P.x:                      # the split's first pass writes the rounded step sizes; both passes run on them
        delta.copy_(step.to(dt))
        step = delta.double()
    gate = None
    if z is not None:
        gate = z.double() if P.flags & _lib.SCAN_Z_PREACTIVATED else z.double() * torch.sigmoid(z.double())
    zi, oi = _view(P.z_row_index, (L,), (1,), torch.int32), _view(P.out_row_index, (L,), (1,), torch.int32)
    out, out_z = act("out"), act("out_z")
    chunk = (P.chunk_len if P.chunk_len > 0 else 2048) if P.x else 0
    r = torch_scan_fwd(u, step, A, bc("B"), bc("C"), D, gate, zi, oi, reset=P.reset_period, chunk=chunk,
                       out_z0=out_z if P.flags & _lib.SCAN_ACCUMULATE else None, kernel_decay=True)
    if out_z is not None:
        out_z.copy_(r["y_gated"].to(dt))
    if out is not None:
        out.copy_(r["y"].to(dt))
    if P.x:
        xv = _view(P.x, (Bsz, dim, r["x_prod"].shape[1], 2 * N), _contig((Bsz, dim, r["x_prod"].shape[1], 2 * N)), f32)
        xv[..., 0::2], xv[..., 1::2] = r["x_prod"].transpose(1, 2).float(), r["x_state"].transpose(1, 2).float()
    if P.checkpoints and got["info1"]:
        nt = -(-L // 16)
        ck = _view(_addr(P.checkpoints), (Bsz, dim // 64, nt, N, 64), _contig((Bsz, dim // 64, nt, N, 64)), f32)
        ck.copy_(r["ckpt"].reshape(Bsz, nt, dim // 64, 64, N).permute(0, 2, 1, 4, 3).float())
    if P.info:
        P.info[0], P.info[1] = got["family"], got["info1"]
    return got["kernel"]


def _scan_generic_fwd(P, got):
    """what scan_generic_kernel serves: every operand through its own strides, B / C per group in bc_dtype or constant fp32 (dim, dstate), the
    row tables, the carries of every chunk end (tests/test_gpu_ref_layout.py on the CPU)"""
    f32, dt, bdt = torch.float32, _io_dtype(P.io_dtype), _io_dtype(P.bc_dtype)
    Bsz, dim, L, N, G = P.batch, P.dim, P.seqlen, P.dstate, P.n_groups
    act = lambda name: _view(getattr(P, name), (Bsz, dim, L), [getattr(P, f"{name}_{s}_stride") for s in ("batch", "d", "l")], dt)

    def bc(name, variable):
        if variable:
            return _view(getattr(P, name), (Bsz, G, N, L), [getattr(P, f"{name}_{s}_stride") for s in ("batch", "group", "dstate", "l")], bdt)
        return _view(getattr(P, name), (dim, N), [getattr(P, f"{name}_d_stride"), getattr(P, f"{name}_dstate_stride")], f32)
    A = _view(P.A, (dim, N), (P.A_d_stride, P.A_dstate_stride), f32)
    D, bias = _view(P.D, (dim,), (1,), f32), _view(P.delta_bias, (dim,), (1,), f32)
    u, z, delta = act("u"), act("z"), act("delta")
    pre = delta.double() if bias is None else delta.double() + bias.double()[:, None]
    step = _softplus(pre) if P.delta_softplus else pre
    gate = None if z is None else z.double() * torch.sigmoid(z.double())
    zi, oi = _view(P.z_row_index, (L,), (1,), torch.int32), _view(P.out_row_index, (L,), (1,), torch.int32)
    chunk = (P.chunk_len if P.chunk_len > 0 else 2048) if P.x else 0
    r = torch_scan_ref_layout(u, step, A, bc("B", P.is_variable_B), bc("C", P.is_variable_C), D, gate, zi, oi, chunk=chunk)
    out, out_z = act("out"), act("out_z")
    if out_z is not None and z is not None:
        out_z.copy_(r["y_gated"].to(dt))
    if out is not None:
        out.copy_(r["y"].to(dt))
    if P.x:
        nc = r["x_prod"].shape[2]
        xv = _view(P.x, (Bsz, dim, nc, 2 * N), _contig((Bsz, dim, nc, 2 * N)), f32)
        xv[..., 0::2], xv[..., 1::2] = r["x_prod"].float(), r["x_state"].float()
    if P.info:
        P.info[0], P.info[1] = got["family"], got["info1"]
    return got["kernel"]


def _conv1d_fwd(P, plan):
    kernel = _front_kernel("zigma_causal_conv1d_fwd", P, plan)
    dt, wdt = _io_dtype(P.io_dtype), _io_dtype(P.w_dtype)
    Bsz, dim, L, W = P.batch, P.dim, P.seqlen, P.width
    x = _view(P.x, (Bsz, dim, L), (P.x_batch_stride, P.x_c_stride, P.x_l_stride), dt)
    w, b = _view(P.weight, (dim, W), (P.weight_c_stride, P.weight_width_stride), wdt), _view(P.bias, (dim,), (1,), wdt)
    y = torch_conv1d(x, w, b, bool(P.silu_activation), _view(_addr(P.x_row_index), (L,), (1,), torch.int32), P.reset_period)
    _view(P.out, (Bsz, dim, L), (P.out_batch_stride, P.out_c_stride, P.out_l_stride), dt).copy_(y.to(dt))
    return kernel


def _addr(p):
    return p if isinstance(p, int) else ctypes.cast(p, ctypes.c_void_p).value


def _contig(shape):
    return [int(np.prod(shape[i + 1:])) for i in range(len(shape))]


def _softplus(x):
    return torch.nn.functional.softplus(x)          # beta 1, threshold 20: the reference's


def _front_kernel(fn_name, P, plan):
    """the kernel the compiled front plan (csrc/front_plan.h) names for the call; refuses what it refuses"""
    got = plan(P)
    if got["status"] != 0:
        raise RuntimeError(f"{fn_name}: refused (status {got['status']})")
    return got["kernel"]


def _conv_xproj_fwd(P, plan):
    kernel = _front_kernel("zigma_conv_x_proj_fwd", P, plan)
    dt = _io_dtype(P.dtype)
    Bsz, L, dim, n = P.batch, P.seqlen, P.dim, P.n
    x = _view(P.x, (Bsz, L, dim), (P.x_batch_stride, P.x_l_stride, 1), dt).double()
    cw, cb = _view(P.conv_weight, (dim, 4), (4, 1), dt).double(), _view(P.conv_bias, (dim,), (1,), dt).double()
    w = _view(P.w, (n, dim), (P.w_row_stride, 1), dt).double()
    idx = _view(_addr(P.x_row_index), (L,), (1,), torch.int32)
    if idx is not None:
        x = x.index_select(1, idx.long())
    xp = torch.nn.functional.pad(x, (0, 0, 3, 0))
    pre = cb + sum(cw[:, t] * xp[:, t:t + L] for t in range(4))
    u = _view(P.u, (Bsz, L, dim), (P.u_batch_stride, P.u_l_stride, 1), dt)
    u.copy_((pre * torch.sigmoid(pre)).to(dt))
    _view(P.out, (Bsz * L, n), (P.out_row_stride, 1), dt).copy_((u.double().reshape(Bsz * L, dim) @ w.T).to(dt))
    return kernel


def _x_proj_fwd(P, plan):
    kernel = _front_kernel("zigma_x_proj_fwd", P, plan)
    dt = _io_dtype(P.dtype)
    x, w = _view(P.x, (P.m, P.k), (P.x_row_stride, 1), dt), _view(P.w, (P.n, P.k), (P.w_row_stride, 1), dt)
    _view(P.out, (P.m, P.n), (P.out_row_stride, 1), dt).copy_((x.double() @ w.double().T).to(dt))
    return kernel


def _dt_proj_fwd(P, plan):
    kernel = _front_kernel("zigma_dt_proj_softplus_fwd", P, plan)
    dt = _io_dtype(P.dtype)
    x, w = _view(P.x, (P.m, P.k), (P.x_row_stride, 1), dt), _view(P.w, (P.n, P.k), (P.w_row_stride, 1), dt)
    pre = x.double() @ w.double().T
    if P.bias:
        pre = pre + _view(P.bias, (P.n,), (1,), torch.float32).double()
    _view(P.out, (P.m, P.n), (P.out_row_stride, 1), dt).copy_((_softplus(pre) if P.softplus else pre).to(dt))
    return kernel


def install_lib_call(monkeypatch, plan=None, front_plan=None, linear_plan=None, norm_linear_plan=None):
    """route _lib.call to the stand-ins above and below.  plan / front_plan / linear_plan / norm_linear_plan: plan_scan(), the plans of
    csrc/front_plan.h, plan_linear() and plan_norm_linear() compiled with g++ (the fixtures of tests/test_host_cpu.py and
    tests/test_linear_cases_cpu.py): they name the kernel, fill the scan's `info` and refuse what the library refuses (only the scan, the three
    front entry points and the two dense projections need them)"""
    from zigma_amd import _lib
    serve = {"zigma_selective_scan_fwd": lambda P: _scan_fwd(P, plan), "zigma_causal_conv1d_fwd": lambda P: _conv1d_fwd(P, front_plan), "zigma_conv_x_proj_fwd": lambda P: _conv_xproj_fwd(P, front_plan),
             "zigma_x_proj_fwd": lambda P: _x_proj_fwd(P, front_plan), "zigma_dt_proj_softplus_fwd": lambda P: _dt_proj_fwd(P, front_plan),
             "zigma_linear_fwd": lambda P: _linear_fwd(P, linear_plan), "zigma_norm_linear_fwd": lambda P: _norm_linear_fwd(P, norm_linear_plan), **OUTER_SERVE}

    def call(fn_name, params, device):
        LAST_KERNEL[0] = serve[fn_name](params)
        if _lib.TRACE is not None:
            _lib.TRACE.append((fn_name, LAST_KERNEL[0], params))
    plans = dict.fromkeys(("zigma_causal_conv1d_fwd", "zigma_conv_x_proj_fwd", "zigma_x_proj_fwd", "zigma_dt_proj_softplus_fwd"), front_plan)

    def ask(fn_name, params):            # _lib.plan: the host-only queries (zigma_*_fwd_plan), from the same compiled plans
        got = {"zigma_selective_scan_fwd": plan, **plans}[fn_name](params)
        return got["status"], got["kernel"]
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "plan", ask)
    monkeypatch.setattr(_lib, "require_device", lambda *t: torch.device("cpu"))
    monkeypatch.setattr(_lib, "last_kernel", lambda: LAST_KERNEL[0])


# ---------------------------------------------------------------------------------------------------
# Stand-ins AT THE C ABI for add-norm forward and the operators around the blocks (tests/test_gpu_outer_fwd.py on the CPU).  The torch_*
# functions are float64 torch restatements of the five operators (F.layer_norm, F.linear, unfold + matmul, TimestepEmbedder.timestep_embedding),
# UNROUNDED except at the 16-bit intermediates the ABI defines; the CPU test holds the numpy references of tests/outer_fwd_cases.py against
# them.  The _*_fwd functions read and write through the parameter block's pointers and strides, refuse what the library refuses and name the
# kernel the library would name (add_norm: launch_norm's selection restated on the block's pointers and pitches; LAST_INSTANTIATION).
# ---------------------------------------------------------------------------------------------------
LAST_INSTANTIATION = [None]
F = torch.nn.functional


def _r(t, dt):
    """a float64 tensor after being stored in dt (through fp32, as the kernels and the numpy references round)"""
    return t.float().to(dt).double()


def _refuse(rc):
    raise RuntimeError(f"stand-in: refused (status {rc})")


def torch_add_norm(x, branch, gate, residual, weight, bias, shift, scale, eps, is_rms, xdt):
    """everything (rows, cols) float64 or None (gate / shift / scale already expanded over the rows) -> dict(x_out, residual_out, y_out, y_mod)"""
    r = {}
    if branch is not None:
        r["x_out"] = x + gate * branch
        x = _r(r["x_out"], xdt)
    if residual is not None:
        x = x + residual
    r["residual_out"] = x
    cols = x.shape[-1]
    if is_rms:
        y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
        y = y if weight is None else y * weight
        y = y if bias is None else y + bias
    else:
        y = F.layer_norm(x, (cols,), weight, bias, eps)
    r["y_out"] = y
    if shift is not None:
        r["y_mod"] = _r(y, xdt) * (1.0 + scale) + shift
    return r


def _norm_instantiation(P, es):
    """launch_norm of csrc/add_norm.hip -> ((VEC, ITERS, LPR), kernel name); es: element sizes of (x, residual, weight, modulation)"""
    xs, rs, ws, ms = es
    strides = [P.x_row_stride, P.branch_row_stride, P.x_out_row_stride, P.res_row_stride, P.res_out_row_stride, P.y_row_stride, P.y_mod_row_stride,
               P.mod_batch_stride]
    ptrs = [(P.x, xs), (P.branch, xs), (P.x_out, xs), (P.y_out, xs), (P.y_mod, xs), (P.residual, rs), (P.residual_out, rs), (P.weight, ws), (P.bias, ws),
            (P.gate, ms), (P.shift, ms), (P.scale, ms)]
    al = lambda n: all(not p or p % (n * s) == 0 for p, s in ptrs)
    vec = P.cols % 4 == 0 and all(s % 4 == 0 for s in strides) and al(4)
    al8 = all(not p or p % (16 if (p in (P.residual, P.residual_out)) else 8 * s) == 0 for p, s in ptrs)
    vec8 = vec and P.cols % 8 == 0 and all(s % 8 == 0 for s in strides) and al8 and xs == 2
    light = (not P.residual and not P.residual_out) or rs == 2
    name = "add_norm_v4" if vec else "add_norm_v1"
    if vec8 and light and P.cols % 128 == 0 and P.cols <= 1024 and P.rows % 4 == 0 and not P.flags & 1:
        return (8, P.cols // 128, 16), "add_norm_v8x4"
    if vec8 and P.cols <= 1024:
        return (8, 2, 64), name
    if vec and P.cols <= 1024:
        return (4, 4, 64), name
    if vec and P.cols <= 4096:
        return (4, 16, 64), name
    if P.cols <= 1024:
        return (1, 16, 64), name
    if P.cols <= 4096:
        return (1, 64, 64), name
    _refuse(-2)


def _add_norm_fwd(P):
    if not P.x or bool(P.branch) != bool(P.gate) or bool(P.shift) != bool(P.scale) or (P.shift and not P.y_mod) or not (P.y_out or P.y_mod):
        _refuse(-1)
    if P.rows < 0 or P.cols < 1 or P.rows_per_batch < 1:
        _refuse(-2)
    if P.flags & ~1:
        _refuse(-6)
    xdt, rdt, wdt = _io_dtype(P.x_dtype), _io_dtype(P.res_dtype), _io_dtype(P.w_dtype)
    if (P.mod_dtype != P.x_dtype and (P.gate or P.shift)) or (P.res_dtype not in (0, P.x_dtype)) or (P.w_dtype not in (0, P.x_dtype)):
        _refuse(-3)
    es = [torch.empty((), dtype=d).element_size() for d in (xdt, rdt, wdt, xdt)]
    inst, name = _norm_instantiation(P, es)
    rows, cols, nb = P.rows, P.cols, -(-P.rows // P.rows_per_batch)
    row = lambda ptr, stride, dt: _view(ptr, (rows, cols), (stride, 1), dt)
    d = lambda t: None if t is None else t.double()
    mod = lambda ptr: None if not ptr else _view(ptr, (nb, cols), (P.mod_batch_stride, 1), xdt).double().repeat_interleave(P.rows_per_batch, 0)[:rows]
    r = torch_add_norm(d(row(P.x, P.x_row_stride, xdt)), d(row(P.branch, P.branch_row_stride, xdt)), mod(P.gate), d(row(P.residual, P.res_row_stride, rdt)),
                       d(_view(P.weight, (cols,), (1,), wdt)), d(_view(P.bias, (cols,), (1,), wdt)), mod(P.shift), mod(P.scale), float(P.eps), bool(P.is_rms), xdt)
    for key, ptr, stride, dt in (("x_out", P.x_out, P.x_out_row_stride, xdt), ("residual_out", P.residual_out, P.res_out_row_stride, rdt),
                                 ("y_out", P.y_out, P.y_row_stride, xdt), ("y_mod", P.y_mod, P.y_mod_row_stride, xdt)):
        if ptr and key in r:
            row(ptr, stride, dt).copy_(r[key].float().to(dt))
    LAST_INSTANTIATION[0] = inst
    return name


def torch_patch_embed(x, w, bias, pos):
    """x (B, C, H, W), w (E, C, p, p), bias (E) | None, pos (L, E) | None, float64 -> (B, L, E): unfold + matmul; conv + bias is a bf16 tensor
    before `+ pos`"""
    E, p = w.shape[0], w.shape[-1]
    cols = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2)            # (B, L, C p p), (channel, dy, dx) fastest
    conv = cols @ w.reshape(E, -1).T
    conv = conv if bias is None else conv + bias
    return conv if pos is None else _r(conv, torch.bfloat16) + pos


def _patch_embed_fwd(P):
    if P.batch < 0 or P.in_chans < 1 or P.patch < 1 or P.embed_dim < 8 or P.height < 1 or P.width < 1:
        _refuse(-2)
    if P.dtype != 2:
        _refuse(-3)
    B, C, p, E, H, W = P.batch, P.in_chans, P.patch, P.embed_dim, P.height, P.width
    if E % 8 or H % p or W % p or C * p * p * E * 4 > 65536:
        _refuse(-2)
    if P.out % 16 or P.out_row_stride % 8 or P.out_batch_stride % 8 or P.weight % 16 or (P.bias and P.bias % 16) or (P.pos and (P.pos % 16 or P.pos_row_stride % 8)):
        _refuse(-4)
    bf, L = torch.bfloat16, (H // p) * (W // p)
    d = lambda t: None if t is None else t.double()
    x = _view(P.x, (B, C, H, W), (P.x_batch_stride, P.x_chan_stride, P.x_row_stride, 1), bf)
    r = torch_patch_embed(d(x), d(_view(P.weight, (E, C, p, p), _contig((E, C, p, p)), bf)), d(_view(P.bias, (E,), (1,), bf)),
                          d(_view(P.pos, (L, E), (P.pos_row_stride, 1), bf)))
    _view(P.out, (B, L, E), (P.out_batch_stride, P.out_row_stride, 1), bf).copy_(r.float().to(bf))
    return "patch_embed"


def torch_timestep_embed(t, freqs, dim):
    """t (B,), freqs (dim // 2,) float64 -> (B, dim) float64 through the model's own timestep_embedding"""
    from zigma_amd.model_zigma import TimestepEmbedder
    return TimestepEmbedder.timestep_embedding(t.float(), dim, dtype=torch.float64, freqs=freqs)       # (t holds bf16 values: .float() is exact)


def _timestep_embed_fwd(P):
    if P.batch < 0 or P.dim < 2:
        _refuse(-2)
    if P.dtype != 2:
        _refuse(-3)
    bf = torch.bfloat16
    r = torch_timestep_embed(_view(P.t, (P.batch,), (1,), bf).double(), _view(P.freqs, (P.dim // 2,), (1,), bf).double(), P.dim)
    _view(P.out, (P.batch, P.dim), (P.out_row_stride, 1), bf).copy_(r.float().to(bf))
    return "timestep_embed"


def torch_skinny_linear(x, w, bias, silu):
    if silu:
        x = _r(F.silu(x), torch.bfloat16)
    return F.linear(x, w, bias)


def _skinny_linear_fwd(P):
    if P.m < 0 or P.n < 0 or P.k < 0:
        _refuse(-2)
    if P.dtype != 2:
        _refuse(-3)
    if P.m > 64 or P.n % 16 or P.k % 128 or P.k > 1024:
        _refuse(-2)
    if P.x % 16 or P.x_row_stride % 8 or P.w % 16 or P.w_row_stride % 8 or P.out % 8 or P.out_row_stride % 4 or (P.bias and P.bias % 8):
        _refuse(-4)
    bf = torch.bfloat16
    x, w = _view(P.x, (P.m, P.k), (P.x_row_stride, 1), bf), _view(P.w, (P.n, P.k), (P.w_row_stride, 1), bf)
    bias = _view(P.bias, (P.n,), (1,), bf)
    r = torch_skinny_linear(x.double(), w.double(), None if bias is None else bias.double(), bool(P.flags & 1))
    _view(P.out, (P.m, P.n), (P.out_row_stride, 1), bf).copy_(r.float().to(bf))
    return "skinny_linear_mfma"


def torch_final_layer(x, w, bias, eps):
    return F.linear(_r(F.layer_norm(x, (x.shape[-1],), eps=eps), torch.bfloat16), w, bias)


def _final_layer_fwd(P):
    if P.rows < 0 or P.cols < 8 or P.n_out < 1:
        _refuse(-2)
    if P.dtype != 2:
        _refuse(-3)
    if P.cols % 8 or P.cols > 2048 or P.n_out > 16:
        _refuse(-2)
    if P.x % 16 or P.x_row_stride % 8 or P.weight % 16:
        _refuse(-4)
    bf = torch.bfloat16
    x, w = _view(P.x, (P.rows, P.cols), (P.x_row_stride, 1), bf), _view(P.weight, (P.n_out, P.cols), (P.cols, 1), bf)
    bias = _view(P.bias, (P.n_out,), (1,), bf)
    r = torch_final_layer(x.double(), w.double(), None if bias is None else bias.double(), float(P.eps))
    _view(P.out, (P.rows, P.n_out), (P.out_row_stride, 1), bf).copy_(r.float().to(bf))
    return "final_layer"


OUTER_SERVE = {"zigma_add_norm_fwd": _add_norm_fwd, "zigma_patch_embed_fwd": _patch_embed_fwd, "zigma_timestep_embed_fwd": _timestep_embed_fwd,
               "zigma_skinny_linear_fwd": _skinny_linear_fwd, "zigma_final_layer_fwd": _final_layer_fwd}


# ---------------------------------------------------------------------------------------------------
# Stand-ins AT THE C ABI for the dense projections, zigma_linear_fwd and zigma_norm_linear_fwd (tests/test_gpu_linear_sweep.py on the CPU).  The
# torch_* functions are float64 torch restatements (F.linear, F.silu, F.layer_norm, torch.addcmul), UNROUNDED except at the 16-bit intermediates the
# ABI defines; the CPU test holds the numpy references of tests/linear_cases.py against them, and the GPU test forms them on the device, in row
# chunks, where a case is too large for the host.  The _*_fwd functions read and write through the parameter block; the compiled plan refuses
# what the library refuses, names the kernel and tells the family (the 4-wave kernel's gated epilogue does not round in the middle).
# ---------------------------------------------------------------------------------------------------
LIN_4W = 2              # enum LinearFamily


def torch_linear(x, w, bias, silu_from_col, res, gate_rows, dt, round_mid):
    """float64 operands (gate_rows already expanded over the rows) -> (out, (residual, gate * v) | None)"""
    v = F.linear(x, w, bias)
    if silu_from_col < w.shape[0]:
        v = torch.cat([v[:, :silu_from_col], F.silu(v[:, silu_from_col:])], 1)
    if res is None:
        return v, None
    return torch.addcmul(res, gate_rows, _r(v, dt) if round_mid else v), (res, gate_rows * v)


def torch_norm_linear(x, w, shift_rows, scale_rows, eps, dt):
    """-> dict(y_mod: the unrounded second stage on the rounded LayerNorm, xa, out, terms of y_mod)"""
    a = _r(F.layer_norm(x, (x.shape[-1],), eps=eps), dt) * (1.0 + scale_rows)
    xa = _r(a + shift_rows, dt)
    return dict(y_mod=a + shift_rows, xa=xa, out=F.linear(xa, w), terms=(a, shift_rows))


def _planned(fn_name, P, plan):
    got = plan(P)
    if got["status"] != 0:
        raise RuntimeError(f"{fn_name}: refused (status {got['status']})")
    return got


def _linear_fwd(P, plan):
    got = _planned("zigma_linear_fwd", P, plan)
    dt, m, n, k = _io_dtype(P.dtype), P.m, P.n, P.k
    d = lambda t: None if t is None else t.double()
    x, w = _view(P.x, (m, k), (P.x_row_stride, 1), dt), _view(P.w, (n, k), (P.w_row_stride, 1), dt)
    res, gate = _view(P.residual, (m, n), (P.res_row_stride, 1), dt), None
    if res is not None:
        gate = _view(P.gate, (m // P.rows_per_batch, n), (P.gate_batch_stride, 1), dt).double().repeat_interleave(P.rows_per_batch, 0)
    out, _ = torch_linear(d(x), d(w), d(_view(P.bias, (n,), (1,), dt)), P.silu_from_col, d(res), gate, dt, got["family"] != LIN_4W)
    _view(P.out, (m, n), (P.out_row_stride, 1), dt).copy_(out.float().to(dt))
    return got["kernel"]


def _norm_linear_fwd(P, plan):
    got = _planned("zigma_norm_linear_fwd", P, plan)
    dt, m, n, k = _io_dtype(P.dtype), P.m, P.n, P.k
    x, w = _view(P.x, (m, k), (P.x_row_stride, 1), dt), _view(P.w, (n, k), (P.w_row_stride, 1), dt)
    nb = m // P.rows_per_batch
    mod = lambda ptr: _view(ptr, (nb, k), (P.mod_batch_stride, 1), dt).double().repeat_interleave(P.rows_per_batch, 0)
    r = torch_norm_linear(x.double(), w.double(), mod(P.shift), mod(P.scale), float(P.eps), dt)
    _view(P.out, (m, n), (P.out_row_stride, 1), dt).copy_(r["out"].float().to(dt))
    return got["kernel"]


# ---------------------------------------------------------------------------------------------------
# Stand-ins AT THE C ABI for zigma_linear_f32_split and zigma_linear_wgrad (tests/test_gpu_matmul_sweep.py on the CPU).  torch_split_linear is
# fp32_matmul.reference on given weight planes (x is split by fp32_matmul.split, the definition), torch_wgrad the float64 dy^T x; the CPU test
# holds the numpy references of tests/matmul_sweep_cases.py against them.  The _* functions read and write through the parameter block, refuse
# what the entry points refuse and name the kernel from the host code's choice (the passes; wgrad_bk / wgrad_slabs of csrc/wgrad.hip).
# ---------------------------------------------------------------------------------------------------
def torch_split_linear(x, w_hi, w_lo, bias, passes):
    """x (m, k) fp32, w_hi / w_lo (n, k) bf16, bias (n) fp32 | None -> (m, n) float64: the bf16-plane products summed in float64"""
    from zigma_amd.fp32_matmul import split
    xh, xl = (t.double() for t in split(x))
    y = xh @ w_hi.double().T
    if passes == 3:
        y = y + (xl @ w_hi.double().T + xh @ w_lo.double().T)
    return y if bias is None else y + bias.double()


def torch_wgrad(dy, x):
    return dy.double().T @ x.double()


def _linear_f32_split(P):
    if not P.x or not P.w_hi or not P.out or (P.passes == 3 and not P.w_lo):
        _refuse(-1)
    if P.flags != 0 or P.passes not in (1, 3):
        _refuse(-6)
    lo, m, n, k = P.passes == 3, P.m, P.n, P.k
    if m < 0 or m % 8 or n < 128 or n % 128 or n > 65536 or k < 64 or k % 64 or k > 65536:
        _refuse(-2)
    if P.x_row_stride < k or P.w_hi_row_stride < k or (lo and P.w_lo_row_stride < k) or P.out_row_stride < n:
        _refuse(-2)
    if (any(p and p % 16 for p in (P.x, P.w_hi, P.w_lo if lo else 0, P.out, P.bias)) or P.x_row_stride % 4 or P.out_row_stride % 4 or P.w_hi_row_stride % 8
            or (lo and P.w_lo_row_stride % 8)):
        _refuse(-4)
    f32, bf = torch.float32, torch.bfloat16
    if m:
        y = torch_split_linear(_view(P.x, (m, k), (P.x_row_stride, 1), f32), _view(P.w_hi, (n, k), (P.w_hi_row_stride, 1), bf),
                               _view(P.w_lo, (n, k), (P.w_lo_row_stride, 1), bf) if lo else None, _view(P.bias, (n,), (1,), f32), P.passes)
        _view(P.out, (m, n), (P.out_row_stride, 1), f32).copy_(y.float() + 0.0)          # (the accumulators start at +0: no -0 result)
    return f"linear_split{P.passes}_128x128"


def _linear_wgrad(P):
    from zigma_amd import _lib
    if not P.dy or not P.x or not P.out:
        _refuse(-1)
    if P.dtype not in (_lib.BF16, _lib.F16) or P.out_dtype not in (P.dtype, _lib.F32):
        _refuse(-3)
    m, n, k = P.m, P.n, P.k
    if m < 1 or n < 8 or k < 8 or n % 8 or k % 8 or n > 8192 or k > 8192 or P.slabs < 0 or P.slabs > 4096:
        _refuse(-2)
    if P.flags != 0:
        _refuse(-6)
    bk = 64 if k <= 64 else 128
    tiles = -(-n // 128) * -(-k // bk)
    S = P.slabs if P.slabs > 0 else max(1, min(-(-512 // tiles), m // 512, 64))
    need = S * n * k * 4 if S > 1 else 0
    if need and not P.workspace:
        _refuse(-1)
    if P.workspace_bytes < need:
        _refuse(-2)
    dt, odt = _io_dtype(P.dtype), _io_dtype(P.out_dtype)
    es = torch.empty((), dtype=odt).element_size()
    if (P.dy_row_stride < n or P.x_row_stride < k or P.out_row_stride < k or P.dy_row_stride % 8 or P.x_row_stride % 8 or P.dy % 16 or P.x % 16 or P.out % 16
            or (P.out_row_stride * es) % 16 or (need and P.workspace % 16)):
        _refuse(-4)
    dy, x = _view(P.dy, (m, n), (P.dy_row_stride, 1), dt), _view(P.x, (m, k), (P.x_row_stride, 1), dt)
    if S > 1:                               # the fp32 partials of the slabs, [S][n][k]
        rows = -(-(-(-m // S)) // 64) * 64
        ws = _view(P.workspace, (S, n, k), (n * k, k, 1), torch.float32)
        for s in range(S):
            ws[s] = torch_wgrad(dy[s * rows:(s + 1) * rows], x[s * rows:(s + 1) * rows]).float()
    _view(P.out, (n, k), (P.out_row_stride, 1), odt).copy_((torch_wgrad(dy, x).float() + 0.0).to(odt))
    return f"wgrad_128x{bk}" + ("_splitk" if S > 1 else "")


OUTER_SERVE.update({"zigma_linear_f32_split": _linear_f32_split, "zigma_linear_wgrad": _linear_wgrad})
