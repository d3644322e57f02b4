"""The SDE samplers with every per-step value on the device: `Sampler.sample_sde(..., noise="device")`.

The reference's loop (integrators.py `sde`) draws each Wiener increment with the CPU generator, copies it to the device and composes a
step from about fifteen eager launches.  Here a step is the model evaluation(s), one to three launches of zigma_sde_step_fwd
(csrc/sde_step.hip: out = c0 a + c1 b + c2 c + cn xi, the noise a counter-based function of (seed, stream, step, element) drawn inside the
kernel) and one zigma_sde_advance, which moves the device step counter and writes the next model times.  Coefficients, times and counters are
read from device memory, so ONE captured graph replays for every step of a trajectory.

The algebra.  For every path, prediction and diffusion form, drift + w score is  p_t x + q_t m  at a fixed time (m: the model output) and
w_t a scalar, so with dt the grid spacing

    Euler-Maruyama   x' = (1 + dt p) x + dt q m + sqrt(2 w dt) xi                                        1 row per step
    Heun             xhat = x + sqrt(2 w dt) xi;  xp = (1 + dt p1) xhat + dt q1 m1;                      3 rows per step
                     x' = 1/2 xhat + (1/2 + 1/2 dt p2) xp + 1/2 dt q2 m2        (dt K1 = xp - xhat)
    last step        cx x + cm m                                                                         1 row

No formula of path.py is restated: p, q, w, cx, cm are obtained by PROBING the sampler's own closures in float64 on the CPU with one-element
tensors, (x, m) = (1, 0), (0, 1) and (0, 0); the last probe must give 0 (the closures are affine in (x, m) with no constant term).  The model
times are the float32 values the reference loop passes: linspace(t0, t1, num_steps)[k] and, for Heun's second evaluation, the float32 sum
t[k] + dt.  The model is always handed float32 times.
"""
import numpy as np
import torch as th

from .. import _lib

SOLVERS = {"Euler": (1, 1), "Heun": (3, 2)}             # sampling_method -> (coefficient rows per step, model times per step)
DTYPES = (th.float32, th.bfloat16, th.float16)


class SdePlan:
    """coef: float64 (rows_per_step * (num_steps - 1) + 1, 4), one row (c0, c1, c2, cn) per launch, the last step's row last;
    times: float32 (num_steps, n_t), row k the model times of step k, the last row the last step's time in every column."""

    def __init__(self, method, num_steps, coef, times, last_step):
        self.method, self.num_steps, self.coef, self.times, self.last_step = method, num_steps, coef, times, last_step
        self.rows_per_step, self.n_t = SOLVERS[method]
        self.last_row = coef.shape[0] - 1


def _probe(fn, t, t_dtype=th.float64):
    """fn(x, t, model) at (x, m) = (1, 0), (0, 1), (0, 0) in float64 -> (coefficient of x, coefficient of m); the third must be 0"""
    tt = th.tensor([float(t)], dtype=t_dtype)
    at = lambda xv, mv: float(th.as_tensor(fn(th.tensor([xv], dtype=th.float64), tt, lambda *_a, **_k: th.tensor([mv], dtype=th.float64))).reshape(-1)[0])
    cx, cm, c0 = at(1.0, 0.0), at(0.0, 1.0), at(0.0, 0.0)
    if c0 != 0.0 and np.isfinite(c0):
        raise ValueError(f"sde_device: the sampler's update is not linear in (x, model output) at t = {float(t)!r} (it maps (0, 0) to {c0!r})")
    return cx, cm


def make_plan(sampler, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=250,
              time_dtype=th.float32):
    """the two tables of one `sample_sde` configuration (module docstring).  Raises ValueError on a non-finite coefficient, naming the step and
    the diffusion form (a score or noise model asked to start at t = 0, say).  time_dtype: the type the reference loop forms Heun's second time in,
    its state's; the device path always runs on float32 times, float64 serves the check of the plan against the reference loop in float64."""
    if sampling_method not in SOLVERS:
        raise NotImplementedError("Sampler type not implemented.")
    if num_steps < 2:
        raise ValueError("sde_device: num_steps must be at least 2")
    if last_step is None:
        last_step_size = 0.0
    tr = sampler.transport
    sde_drift, diffusion = sampler._sde_drift_and_diffusion(diffusion_form=diffusion_form, diffusion_norm=diffusion_norm)
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=diffusion_form, sde=True, eval=True, reverse=False, last_step_size=last_step_size)
    assert t0 < t1, "SDE sampler has to be in forward time"
    t = th.linspace(t0, t1, num_steps)                                   # float32, as integrators.sde forms it
    dt32 = t[1] - t[0]
    dt = float(dt32)
    rows_per_step, n_t = SOLVERS[sampling_method]
    coef, times = [], []

    def w_at(tk):
        one, tt = th.ones(1, dtype=th.float64), th.tensor([float(tk)], dtype=th.float64)
        return float(th.as_tensor(diffusion(one, tt)).reshape(-1)[0])

    def checked(rows, k, what):
        for row in rows:
            if not all(np.isfinite(row)):
                raise ValueError(f"sde_device: non-finite coefficient {tuple(row)} at {what} {k} (t = {float(times[-1][0])!r}) of the {sampling_method} solver with "
                                 f"diffusion_form={diffusion_form!r}, path {type(tr.path_sampler).__name__}, {tr.model_type.name}: the interval starts or "
                                 "ends where this form is singular")
        coef.extend(rows)

    with th.no_grad(), np.errstate(all="ignore"):
        for k in range(num_steps - 1):
            tk = t[k]
            t2 = (th.ones(1, dtype=time_dtype) * tk + dt32.to(time_dtype))[0]         # Heun's second time: the sum as the reference loop forms it
            times.append((float(tk), float(t2))[:n_t])
            p, q = _probe(sde_drift, tk)
            w = w_at(tk)
            cn = float(np.sqrt(np.float64(2.0 * w * dt)))
            if sampling_method == "Euler":
                checked([(1.0 + dt * p, dt * q, 0.0, cn)], k, "step")
            else:
                p2, q2 = _probe(sde_drift, t2)
                checked([(1.0, 0.0, 0.0, cn), (1.0 + dt * p, dt * q, 0.0, 0.0), (0.5, 0.5 + 0.5 * dt * p2, 0.5 * dt * q2, 0.0)], k, "step")
        t_last = float(th.ones(1)[0] * t1)                               # float32(t1), the time Sampler.sample_sde hands the last step
        times.append((t_last,) * n_t)
        if last_step is None:
            checked([(1.0, 0.0, 0.0, 0.0)], num_steps - 1, "the last step")
        else:
            # (Sampler.sample_sde hands the last step a float32 time tensor whatever the state's type: a float64 reference loop forms this one
            # row's coefficients from float32 path functions, and the plan that is held against it does the same)
            cx, cm = _probe(sampler._last_step(sde_drift, last_step=last_step, last_step_size=last_step_size), t_last,
                            th.float64 if time_dtype == th.float32 else th.float32)
            checked([(cx, cm, 0.0, 0.0)], num_steps - 1, f"the last step ({last_step})")
    return SdePlan(sampling_method, num_steps, np.asarray(coef, np.float64), np.asarray(times, np.float32 if time_dtype == th.float32 else np.float64), last_step)


class DeviceNoise:
    """The 16-byte zigma_sde_state_t of a trajectory in device memory: Philox key (seed), stream, step counter.  The kernels read it when they
    run, so a captured graph follows reset()."""

    def __init__(self, seed=0, stream=0, device="cuda"):
        self.state = th.zeros(4, dtype=th.int32, device=device)
        self.reset(seed, stream)

    def reset(self, seed=None, stream=None):
        """new seed and / or stream (None: kept); the step counter returns to 0"""
        seed = self.seed if seed is None else int(seed)
        stream = self.stream if stream is None else int(stream)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("DeviceNoise: the seed is an integer in [0, 2^64)")
        if not 0 <= stream < 2 ** 32:
            raise ValueError("DeviceNoise: the stream is an integer in [0, 2^32)")
        self.seed, self.stream = seed, stream
        words = np.array([seed & 0xffffffff, seed >> 32, stream, 0], dtype=np.uint32)
        self.state.copy_(th.from_numpy(words.view(np.int32)))
        return self

    def rewind(self):
        """step counter to 0, on the device (no host copy)"""
        self.state[3:].zero_()
        return self


def sde_step(out, a=None, b=None, c=None, *, coef, row=0, rows_per_step=1, state=None, absolute=False, elem_offset=0, bits_out=None, n=None):
    """one zigma_sde_step_fwd launch on contiguous tensors (None: the operand is absent); coef: float32 (rows, 4) device tensor, state: DeviceNoise.state"""
    dev = _lib.require_device(out, a, b, c, coef, state, bits_out)
    for t in (a, b, c):
        if t is not None and (t.dtype != out.dtype or not t.is_contiguous()):
            raise ValueError("sde_step: the operands are contiguous tensors of the output's dtype")
    P = _lib.SdeStepParams(n=out.numel() if n is None else n, elem_offset=elem_offset, coef_rows=coef.shape[0], dtype=_lib.dtype_id(out),
                           flags=_lib.SDE_ROW_ABSOLUTE if absolute else 0, rows_per_step=rows_per_step, row=row, a=_lib.ptr(a), b=_lib.ptr(b), c=_lib.ptr(c),
                           out=_lib.ptr(out), coef=_lib.ptr(coef), state=_lib.ptr(state), bits_out=_lib.ptr(bits_out))
    _lib.call("zigma_sde_step_fwd", P, dev)


def sde_advance(state, times, t_out):
    """one zigma_sde_advance launch: times float32 (rows, n_t), t_out float32 (n_t, batch)"""
    dev = _lib.require_device(state, times, t_out)
    P = _lib.SdeAdvanceParams(state=_lib.ptr(state), times=_lib.ptr(times), t_out=_lib.ptr(t_out), n_rows=times.shape[0], n_t=times.shape[1], batch=t_out.shape[1], flags=0)
    _lib.call("zigma_sde_advance", P, dev)


def _check_init(z):
    if not th.is_tensor(z) or not z.is_cuda or z.dtype not in DTYPES:
        what = f"a {z.device.type} tensor of {z.dtype}" if th.is_tensor(z) else type(z).__name__
        raise ValueError(f"sample_sde(noise='device'): init_z must be a CUDA tensor in float32, bfloat16 or float16 (the noise is drawn by a HIP kernel); got {what}")


class _Trajectory:
    """the device tables and work buffers of one (plan, shape, dtype, model, keyword tensors): steps are launches only, so they can be captured"""

    def __init__(self, plan, z, model, kw, noise, graph):
        self.plan, self.model, self.noise = plan, model, noise
        dev = z.device
        self.coef = th.from_numpy(plan.coef.astype(np.float32)).to(dev)
        self.times = th.from_numpy(plan.times).to(dev)
        self.x = th.empty(z.shape, dtype=z.dtype, device=dev)
        self.xp = th.empty_like(self.x) if plan.method == "Heun" else None
        self.t = th.empty(plan.n_t, z.shape[0], dtype=th.float32, device=dev)
        self.kw = {k: (v.clone() if graph and th.is_tensor(v) else v) for k, v in kw.items()}
        self.step_graph = self.last_graph = None
        if graph:
            self._capture()

    def _m(self, m):
        if m.shape != self.x.shape:
            raise ValueError("sample_sde(noise='device'): the model output's shape differs from the state's")
        return m.to(self.x.dtype).contiguous()

    def _launch(self, out, a, b=None, c=None, *, row, absolute=False):
        sde_step(out, a, b, c, coef=self.coef, row=row, rows_per_step=self.plan.rows_per_step, state=self.noise.state, absolute=absolute)

    def _step(self):
        x, t = self.x, self.t
        if self.plan.method == "Euler":
            self._launch(x, x, self._m(self.model(x, t[0], **self.kw)), row=0)
        else:
            self._launch(x, x, row=0)                                                # xhat, in place
            self._launch(self.xp, x, self._m(self.model(x, t[0], **self.kw)), row=1)
            self._launch(x, x, self.xp, self._m(self.model(self.xp, t[1], **self.kw)), row=2)
        sde_advance(self.noise.state, self.times, t)

    def _last(self):
        if self.plan.last_step is not None:
            self._launch(self.x, self.x, self._m(self.model(self.x, self.t[0], **self.kw)), row=self.plan.last_row, absolute=True)

    def _begin(self, z):
        self.x.copy_(z)
        self.t.copy_(self.times[0].view(-1, 1).expand_as(self.t))
        self.noise.rewind()

    def _capture(self):
        self._begin(th.zeros_like(self.x))
        side = th.cuda.Stream()
        side.wait_stream(th.cuda.current_stream())
        with th.cuda.stream(side), th.no_grad():                     # library handles / lazy caches off the graph (as GraphedForward does)
            for _ in range(2):
                self._step()
            self._last()
        th.cuda.current_stream().wait_stream(side)
        self.step_graph = th.cuda.CUDAGraph()
        with th.cuda.graph(self.step_graph), th.no_grad():
            self._step()
        if self.plan.last_step is not None:
            self.last_graph = th.cuda.CUDAGraph()
            with th.cuda.graph(self.last_graph), th.no_grad():
                self._last()
        # (the warm-up advanced the counter and moved x: every trajectory starts with _begin, which puts both back)

    def run(self, z, kw):
        if self.step_graph is None:
            self.kw = kw
        else:                                                           # the capture reads its own copies of the keyword tensors
            for k, v in self.kw.items():
                if th.is_tensor(v):
                    v.copy_(kw[k])
        xs = []
        with th.no_grad():
            self._begin(z)
            for _ in range(self.plan.num_steps - 1):
                self.step_graph.replay() if self.step_graph is not None else self._step()
                xs.append(self.x.clone())
            self.last_graph.replay() if self.last_graph is not None else self._last()
            xs.append(self.x.clone())
        return xs


class DeviceSdeSampler:
    """what `Sampler.sample_sde(noise="device")` returns: fn(init_z, model, **model_kwargs) -> list of num_steps states, like the reference path.
    `fn.noise` is the DeviceNoise of the device last used (`fn.noise.reset(seed=...)` starts another trajectory on the same capture);
    `fn.captures` counts the graph captures made."""

    def __init__(self, plan, seed=0, stream=0, graph=False):
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("sample_sde: the seed is an integer in [0, 2^64)")
        if not 0 <= int(stream) < 2 ** 32:
            raise ValueError("sample_sde: the stream is an integer in [0, 2^32)")
        self.plan, self.seed, self.stream, self.graph = plan, int(seed), int(stream), graph
        self.noise, self.captures, self._traj = None, 0, {}

    def __call__(self, init_z, model, **model_kwargs):
        _check_init(init_z)
        if self.noise is None or self.noise.state.device != init_z.device:
            self.noise = DeviceNoise(self.seed, self.stream, init_z.device)
            self._traj = {}
        sig = lambda v: (tuple(v.shape), v.dtype) if th.is_tensor(v) else ("value", id(v))
        # (`model.forward` is a new bound-method object at every access: the key is the object and the function it is bound to)
        who = (id(model.__self__), id(model.__func__)) if hasattr(model, "__self__") and hasattr(model, "__func__") else id(model)
        key = (tuple(init_z.shape), init_z.dtype, who, tuple((k, sig(v)) for k, v in sorted(model_kwargs.items())))
        traj = self._traj.get(key)
        if traj is None:
            traj = self._traj[key] = _Trajectory(self.plan, init_z, model, model_kwargs, self.noise, self.graph)
            self.captures += bool(self.graph)
        return traj.run(init_z, model_kwargs)


def run_device(plan, init_z, model, graph=False, seed=0, stream=0, **model_kwargs):
    """one trajectory of `plan` (make_plan) from init_z -> list of num_steps states"""
    return DeviceSdeSampler(plan, seed=seed, stream=stream, graph=graph)(init_z, model, **model_kwargs)
