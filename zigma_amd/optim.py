"""The tail of a training step on the own kernels: global-norm gradient clipping, AdamW, the parameters' moving average (EMA) and the refresh of their
16-bit shadows in ONE pass over the parameters (csrc/optim_step.hip, zigma_optim_* in include/zigma_hip.h).

The reference's step is `opt.step()` -> `grad_clip(...)` -> `update_ema(ema_model, model)` (train_acc.py:443-448, utils/train_utils.py:103-133): a fused
AdamW, a norm pass plus a scaling pass, two small launches per parameter for the EMA, and — under autocast here — the cast of amp._Group.refresh.  Here a
device table names every parameter's (p, grad, exp_avg, exp_avg_sq, ema, shadow) and a chunk map names each workgroup's piece, as zigma_multi_cast_fwd
does, and a step is three launches: the gradients' sum of squares, one workgroup that turns it into the step's scalars ON THE DEVICE (norm, clip
coefficient, skip-on-overflow, the step counter, the bias corrections), and the update.  Nothing comes back to the host, so a step never waits for the
device and can be captured in a graph.

Two deliberate differences from the reference loop, both stated in DESIGN.md §6.3:
  * the clip comes BEFORE the update (the reference clips after `opt.step()`, which scales gradients that the next `zero_grad` throws away);
  * a non-finite gradient norm SKIPS the step — parameters, both moments, the EMA, the shadows and the step counter keep their bits — where
    `clip_grad_norm_` would multiply every gradient by NaN and poison the parameters.  `opt.skipped` reports it.

There is no fallback: parameters that are not contiguous fp32 tensors on one GPU are refused at construction.

FusedAdamW16 (below) is the same tail for a pure bf16 model: fp32 moments and EMA, the bf16 parameter written back with stochastic
rounding drawn inside the update kernel (zigma_optim16_*)."""
import torch

from . import _lib, amp

CHUNK = amp.CHUNK         # elements per workgroup (256 lanes x 8 elements x 2 rounds), the cast kernel's
STATS = {"steps": 0, "launches": 0, "table_builds": 0}


def _device_ok(t):
    return t.is_cuda


def _check_tensor(who, t, what, dtype, wrong_dtype, device=None, shape=None):
    """`wrong_dtype(dtype)` is the class's sentence about a tensor of another element type"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {what} is not a tensor")
    if t.layout != torch.strided:
        raise ValueError(f"{who}: {what} is sparse; the kernel takes dense tensors only")
    if t.dtype != dtype:
        raise ValueError(f"{who}: {what} is {wrong_dtype(t.dtype)}")
    if not _device_ok(t):
        raise ValueError(f"{who}: {what} is on {t.device}; the kernel needs a GPU (there is no CPU fallback)")
    if device is not None and t.device != device:
        raise ValueError(f"{who}: {what} is on {t.device}, the parameters are on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {what} is not contiguous")
    if shape is not None and t.shape != shape:
        raise ValueError(f"{who}: {what} has shape {tuple(t.shape)}, its parameter {tuple(shape)}")


def _check_hyper(who, lr, betas, eps, weight_decay, max_grad_norm, ema_decay):
    """the constructors' refusals of hyperparameters the launchers would refuse (or torch.optim.AdamW does)"""
    if isinstance(lr, torch.Tensor):
        raise ValueError(f"{who}: lr is a host value per launch, not a tensor")
    if not 0.0 <= lr < float("inf"):
        raise ValueError(f"{who}: invalid lr {lr}")
    if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
        raise ValueError(f"{who}: betas {betas} outside [0, 1)")
    if not 0.0 < eps < float("inf"):
        raise ValueError(f"{who}: eps must be positive, got {eps}")
    if not 0.0 <= weight_decay < float("inf"):
        raise ValueError(f"{who}: invalid weight_decay {weight_decay}")
    if max_grad_norm is not None and not 0.0 < max_grad_norm < float("inf"):
        raise ValueError(f"{who}: max_grad_norm must be positive or None, got {max_grad_norm}")
    if not 0.0 <= ema_decay <= 1.0:
        raise ValueError(f"{who}: ema_decay {ema_decay} outside [0, 1]")


def arena_views(like, device):
    """one zero-filled fp32 arena with a 256-byte slot per tensor of `like` (amp.arena_layout) -> (arena, [view shaped like each tensor])"""
    numels = [t.numel() for t in like]
    offsets, nbytes = amp.arena_layout(numels, itemsize=4)
    arena = torch.zeros(max(nbytes, amp.SLOT_ALIGN) + amp.SLOT_ALIGN, device=device, dtype=torch.uint8)
    arena = arena[(-arena.data_ptr()) % amp.SLOT_ALIGN:][:max(nbytes, amp.SLOT_ALIGN)]
    return arena, [arena[o:o + 4 * n].view(torch.float32).view(t.shape) for t, o, n in zip(like, offsets, numels)]


def step_rows(params, grads, ms, vs, emas, shadows):
    """the table's rows, one per parameter that has a gradient (torch's optimizers skip the others too): eight int64 each, zigma_optim_row_t.
    Anything with data_ptr() and numel() will do."""
    rows = []
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            continue
        ema, sh = (emas[i] if emas else None), (shadows[i] if shadows else None)
        rows.append((p.data_ptr(), g.data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(), 0 if ema is None else ema.data_ptr(), 0 if sh is None else sh.data_ptr(),
                     p.numel(), 0))
    return rows


class StepTables:
    """the device table, chunk map and partial-sum buffer of a step, rebuilt and uploaded only when the host list of rows has moved (compared every
    step; `zero_grad(set_to_none=False)` keeps the gradients' addresses, so in a steady loop nothing is uploaded or allocated)"""

    def __init__(self, chunk=CHUNK, width=8, numel_col=6):
        self.chunk, self.rows, self.numels = chunk, None, None
        self.width, self.numel_col = width, numel_col                     # int64 words per row, and which of them is numel (zigma_optim16_row_t: 10, 5)
        self.table = self.cmap = self.partials = None
        self.n_chunks = self.builds = 0

    def update(self, rows, device):
        """-> True if anything was uploaded"""
        if rows == self.rows:
            return False
        numels = [r[self.numel_col] for r in rows]
        if numels != self.numels:
            cmap = amp.build_chunk_map(numels, self.chunk)
            self.cmap = torch.tensor(cmap or [(0, 0)], dtype=torch.int64).to(device)
            self.partials = torch.zeros(max(len(cmap), 1), dtype=torch.float32, device=device)
            self.n_chunks, self.numels = len(cmap), numels
        self.table = torch.tensor(rows or [(0,) * self.width], dtype=torch.int64).to(device)     # (the old table stays alive until here, past its last launch)
        self.rows = rows
        self.builds += 1
        return True


class _StepTail(torch.optim.Optimizer):
    """what the two optimizers of this module share: ONE parameter group of torch.optim.AdamW's keys, fp32 moment arenas, the device state block
    (zigma_optim_state_t in `_block`) behind `step_count`, `skipped` and `grad_norm`, state_dict() as copies, zero_grad() in place, and the step:
    checks, rows, tables, three launches.  A subclass names its element type (`_dtype`, `_wrong_dtype`), and supplies `_rows(ps, grads)`,
    `_launch(group, tables, n_rows)` and, if its group carries more keys, `_check_group_extra(group)`."""

    def __init__(self, params, lr, betas, eps, weight_decay, max_grad_norm, ema_decay, amsgrad, maximize, **more_keys):
        _check_hyper(type(self).__name__, lr, betas, eps, weight_decay, max_grad_norm, ema_decay)
        # (the keys torch.optim.AdamW's groups carry, so that a state_dict travels both ways)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None, capturable=False,
                        differentiable=False, fused=True, decoupled_weight_decay=True, **more_keys)
        super().__init__(params, defaults)
        self._check_group()
        ps = self.param_groups[0]["params"]
        for i, p in enumerate(ps):
            self._check_tensor(p, f"parameter {i}", ps[0].device)
        self.device = ps[0].device
        self.max_grad_norm, self.ema_decay = max_grad_norm, ema_decay

    def _allocate(self, tables):
        """the end of a constructor, past its refusals: the fp32 moment arenas, the state block, the step's tables, state[p]"""
        ps = self.param_groups[0]["params"]
        self._m_arena, self._m = arena_views(ps, self.device)
        self._v_arena, self._v = arena_views(ps, self.device)
        self._block = torch.zeros(8, dtype=torch.float32, device=self.device)             # zigma_optim_state_t
        self._tables = tables
        self._install_state()

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError(f"{type(self).__name__}: one parameter group only (the gradient norm is global; the reference trains with one group)")
        super().add_param_group(param_group)

    def _check_tensor(self, t, what, device=None, shape=None):
        _check_tensor(type(self).__name__, t, what, self._dtype, self._wrong_dtype, device, shape)

    def _check_group(self):
        g, who = self.param_groups[0], type(self).__name__
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError(f"{who}: amsgrad and maximize are not implemented by the kernel")
        if g.get("decoupled_weight_decay") is False:
            raise ValueError(f"{who}: the kernel's weight decay is decoupled (AdamW); this group asks for Adam's L2 form")
        if isinstance(g["lr"], torch.Tensor):
            raise ValueError(f"{who}: lr is a host value per launch, not a tensor")
        self._check_group_extra(g)

    def _check_group_extra(self, g):
        pass

    @property
    def step_count(self):
        """the shared device step counter (fp32 scalar, like the steps of torch's fused / capturable optimizers)"""
        return self._block[0]

    @property
    def skipped(self):
        """device int32 scalar: 1 if the last step changed nothing (non-finite norm or GradScaler's found_inf)"""
        return self._block.view(torch.int32)[1]

    @property
    def grad_norm(self):
        """device fp32 scalar: the last step's global gradient norm before clipping, unscaled (NaN when max_grad_norm is None)"""
        return self._block[2]

    def _install_state(self):
        for p, m, v in zip(self.param_groups[0]["params"], self._m, self._v):
            self.state[p] = {"step": self._block[0], "exp_avg": m, "exp_avg_sq": v}

    def state_dict(self):
        """torch's layout.  Every tensor is a COPY (the live ones are views of the arenas and one shared step, which another optimizer must not
        alias), and each parameter gets a step of its own, as torch.optim.AdamW keeps them."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in st.items()} for k, st in sd["state"].items()}
        return sd

    def _loaded_step(self, loaded):
        """the ONE step of the loaded per-parameter states (None: a parameter without state); raises if they disagree"""
        n = len(self.param_groups[0]["params"])
        steps = [torch.as_tensor(st["step"]).detach().to(device="cpu", dtype=torch.float32).reshape(()) for st in loaded if st is not None]
        steps = torch.stack(steps).tolist() if steps else []
        if len(set(steps)) > 1 or (steps and steps[0] != 0 and len(steps) != n):
            raise ValueError(f"{type(self).__name__}: the loaded per-parameter steps disagree (or some parameters have none); this optimizer keeps ONE step counter: "
                             f"{sorted(set(steps))}, {len(steps)} of {n} parameters")
        return steps[0] if steps else 0.0

    def _restart_at(self, step):
        """the end of a load: a fresh state block at `step`, state[p] on the live tensors again"""
        self._block.zero_()
        self._block[0] = step
        self.state.clear()
        self._install_state()

    def zero_grad(self, set_to_none=False):
        """zeroes the gradients in place by default, so that their addresses — and with them the device table — stay put"""
        super().zero_grad(set_to_none=set_to_none)

    def _fill(self, P, g, T, n_rows):
        """what both parameter blocks carry: table, map, counts, state, partials (when there is a norm pass), the seven hyperparameters, chunk"""
        P.table, P.chunk_map, P.n_entries, P.n_chunks = T.table.data_ptr(), T.cmap.data_ptr(), n_rows, T.n_chunks
        P.state, P.chunk = self._block.data_ptr(), T.chunk
        P.lr, (P.beta1, P.beta2), P.eps, P.weight_decay = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        P.max_grad_norm, P.ema_decay = self.max_grad_norm or 0.0, self.ema_decay
        if self.max_grad_norm is not None:
            P.partials = T.partials.data_ptr()
        return P

    def _launches(self, sumsq, P, prepare_block, adamw):
        if self.max_grad_norm is not None:
            _lib.call(sumsq, P, self.device)
        _lib.call("zigma_optim_prepare", prepare_block, self.device)
        _lib.call(adamw, P, self.device)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        self._check_group()
        ps, dt = g["params"], self._dtype
        grads = [p.grad for p in ps]
        for i, (p, gr) in enumerate(zip(ps, grads)):
            if gr is not None and (gr.dtype != dt or gr.layout != torch.strided or gr.device != p.device or gr.shape != p.shape or not gr.is_contiguous()
                                   or not p.is_contiguous() or p.dtype != dt):
                raise RuntimeError(f"{type(self).__name__}: parameter {i} or its gradient is not a dense contiguous {str(dt).replace('torch.', '')} tensor on {self.device}")
        rows = self._rows(ps, grads)
        if not rows:
            return loss
        STATS["table_builds"] += self._tables.update(rows, self.device)
        self._launch(g, self._tables, len(rows))
        STATS["steps"] += 1
        STATS["launches"] += 3 if self.max_grad_norm is not None else 2
        return loss


class FusedAdamW(_StepTail):
    """AdamW (decoupled weight decay, torch.optim.AdamW's formulas) with global-norm clipping, an EMA of the parameters and the 16-bit shadows of
    zigma_amd.amp in one pass, three launches per step (two without clipping), no host synchronisation.

      max_grad_norm  None: no norm pass, no clipping.  Else the gradients are scaled by min(1, max_grad_norm / (norm + 1e-6)), the formula of
                     `clip_grad_norm_`, BEFORE the update (the reference clips after its step); the gradients themselves are never written.
      ema_params     tensors parallel to `params`, or a module whose parameters() are (`copy.deepcopy(model)`): ema += (p_new - ema) * (1 - ema_decay),
                     in place where they live.
      shadows        a module that carries (or can carry) a zigma_amd.amp group, or (module, torch.bfloat16 / torch.float16); a bare module means
                     bf16.  The step writes the registered parameters' shadows itself, and the next autocast forward casts nothing.

    A step whose gradient norm is not finite, or for which a GradScaler found an inf, is SKIPPED on the device: nothing is written and the step counter
    stays (where `clip_grad_norm_` would have poisoned the parameters).  `opt.grad_norm` and `opt.skipped` are device tensors of the last step
    (`grad_norm` is NaN without clipping); reading them is the caller's synchronisation, the step has none.

    One parameter group; contiguous fp32 parameters on one GPU; no amsgrad, no maximize, no sparse gradients — anything else raises.  `lr` and the other
    hyperparameters are host values handed to each launch: a captured graph (torch.cuda.graph) bakes them in, and a schedule needs a re-capture.
    Capture after one eager step, with `zero_grad(set_to_none=False)` (this class's default), so that the tables exist and the addresses stay.

    state[p] has torch's keys: "exp_avg" / "exp_avg_sq" are views of two fp32 arenas, "step" is ONE device scalar shared by all parameters.
    state_dict() hands out copies with a step per parameter and loads into torch.optim.AdamW(fused=True); load_state_dict() takes that one's, and
    raises if its per-parameter steps disagree."""

    _step_supports_amp_scaling = True
    _dtype = torch.float32

    @staticmethod
    def _wrong_dtype(dtype):
        return f"{dtype}; the kernel takes float32 only (keep fp32 master parameters and train under torch.autocast)"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, ema_params=None, ema_decay=0.9999,
                 shadows=None, *, amsgrad=False, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, ema_decay, amsgrad, maximize)
        ps = self.param_groups[0]["params"]
        self._ema = None
        if ema_params is not None:
            ema = list(ema_params.parameters()) if isinstance(ema_params, torch.nn.Module) else list(ema_params)
            if len(ema) != len(ps):
                raise ValueError(f"FusedAdamW: {len(ema)} ema tensors for {len(ps)} parameters")
            for i, (e, p) in enumerate(zip(ema, ps)):
                self._check_tensor(e, f"ema tensor {i}", self.device, p.shape)
                if e.data_ptr() == p.data_ptr() and p.numel():
                    raise ValueError(f"FusedAdamW: ema tensor {i} IS parameter {i}; pass a copy (copy.deepcopy(model))")
            self._ema = ema
        self._shadow_module, self._shadow_dtype, self._grp, self._shadow_list = None, None, None, None
        if shadows is not None:
            mod, dt = shadows if isinstance(shadows, (tuple, list)) else (shadows, torch.bfloat16)
            if not isinstance(mod, torch.nn.Module) or dt not in (torch.bfloat16, torch.float16):
                raise ValueError("FusedAdamW: shadows is a module or (module, torch.bfloat16 / torch.float16)")
            self._shadow_module, self._shadow_dtype = mod, dt
        self._allocate(StepTables())

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdamW: one parameter group only")
        self._check_group()
        loaded = [self.state[p] if p in self.state and len(self.state[p]) else None for p in self.param_groups[0]["params"]]
        step = self._loaded_step(loaded)
        for st, m, v in zip(loaded, self._m, self._v):
            if st is None:
                m.zero_()
                v.zero_()
            else:
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
        self._restart_at(step)

    # ---- the step ---------------------------------------------------------------------------------------------------------------------------------
    def _shadows_now(self):
        """per parameter, its slot in the module's shadow arena (or None), and that arena's group"""
        mod = self._shadow_module
        if mod is None:
            return None, None
        if not amp.attached(mod):
            amp.attach(mod)
        grp = mod.__dict__["_amp_group"]
        if grp is not self._grp:
            slot = {id(q): s for q, s in zip(grp.params, grp._arena(self._shadow_dtype)["shadows"])}
            self._grp, self._shadow_list = grp, [slot.get(id(p)) for p in self.param_groups[0]["params"]]
        return self._shadow_list, grp

    def _scaler_scalar(self, name):
        t = getattr(self, name, None)               # (set by torch.amp.GradScaler.step around the call, grad_scaler.py: `optimizer.grad_scale = ...`)
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() == 1 and t.device == self.device):
            raise RuntimeError(f"FusedAdamW: {name} must be a one-element float32 tensor on {self.device}")
        return t

    def _rows(self, ps, grads):
        return step_rows(ps, grads, self._m, self._v, self._ema, self._shadows_now()[0])

    def _launch(self, g, T, n_rows):
        shadows, grp = self._shadows_now()
        P = self._fill(_lib.OptimParams(), g, T, n_rows)
        P.grad_scale, P.found_inf = _lib.ptr(self._scaler_scalar("grad_scale")), _lib.ptr(self._scaler_scalar("found_inf"))
        P.shadow_dtype = _lib._DT[self._shadow_dtype] if shadows else -1
        # were the shadows current before this step?  Then they are current after it: written by the kernel, or — a skipped step — as unchanged as the
        # parameters.  If they were stale, a skipped step would leave them stale, so nothing is recorded and the next forward refreshes as ever.
        fresh = grp is not None and grp.fresh(self._shadow_dtype)
        self._launches("zigma_optim_grad_sumsq", P, P, "zigma_optim_adamw")
        if fresh:
            grp.written_by_step(self._shadow_dtype)


# ---- the same tail for a pure bf16 model ----------------------------------------------------------------------------------------------------------------
MAX_NUMEL16 = 1 << 35     # an element's random bits are addressed by a 32-bit octet index (include/zigma_hip.h)
_ROUNDINGS = ("stochastic", "nearest")


def step_rows16(params, grads, ms, vs, emas):
    """the 16-bit table's rows, one per parameter that has a gradient: ten int64 each, zigma_optim16_row_t.  `pid` is the parameter's index in
    `params`, NOT the row's index: a parameter's random bits do not depend on which others got a gradient."""
    rows = []
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            continue
        rows.append((p.data_ptr(), g.data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(), emas[i].data_ptr() if emas else 0, p.numel(), i, 0, 0, 0))
    return rows


class FusedAdamW16(_StepTail):
    """FusedAdamW for a pure bfloat16 model: bf16 parameters and gradients, fp32 moments, an optional fp32 EMA, and the parameter written back with
    STOCHASTIC ROUNDING drawn inside the update kernel (zigma_optim16_* of include/zigma_hip.h).  Three launches per step (two
    without clipping), no host synchronisation; clip-before-update and skip-on-a-non-finite-norm as in FusedAdamW.

    Why: in bf16 an update below half an ulp is rounded away.  At lr = 1e-4 a weight of 1.0 (a norm weight) never moves under round-to-nearest, and
    an EMA with decay 0.9999 kept in bf16 is a frozen copy.  Here the update and the EMA are formed in fp32 from the bf16 parameter, the EMA stays
    fp32, and the parameter is rounded up or down with probability proportional to the distance: the expectation of what is stored is the fp32 value.

      ema            True: a third fp32 arena, initialised from the parameters (exact widening); ema += (x - ema) * (1 - ema_decay) with the fp32 x
                     of the step, not its rounding.  `ema_tensors()` hands out the views, `copy_ema_to(module)` writes them, rounded to nearest,
                     into a module's bf16 parameters (a sampling copy).
      rounding       "stochastic", or "nearest": round to nearest even, no random bits (what torch.optim.AdamW does on bf16 tensors).
      seed, stream   the random bits are a function of (seed, stream, the parameter's index in the group, the step counter, the element's index):
                     Philox4x32-10, nothing else.  EVERY RANK of a DistributedDataParallel run must pass the same seed and stream: the replicas
                     then round alike and stay bit-identical.

    Under graph replay (torch.cuda.graph) seed, stream and the hyperparameters are baked into the graph, but the step counter is read ON THE DEVICE:
    every replay draws fresh bits.  The counter is an fp32 scalar, exact below 2^24 steps.  Capture after one eager step, with
    `zero_grad(set_to_none=False)` (this class's default).

    One parameter group; contiguous bf16 parameters on one GPU with dense contiguous bf16 gradients; anything else raises: fp32 parameters belong to
    FusedAdamW, fp16 ones have no loss scaling to train with.  state[p] has torch's keys "step" (ONE device scalar shared by all), "exp_avg",
    "exp_avg_sq" (fp32 views of two arenas) plus "ema".  state_dict() hands out copies and records rounding, seed and stream in the group;
    load_state_dict() takes its own dicts and those of torch.optim.AdamW on the same bf16 model (bf16 moments are widened), and raises if the
    per-parameter steps disagree.  `skipped`, `grad_norm` and `step_count` are device scalars, as in FusedAdamW."""

    _dtype = torch.bfloat16

    @staticmethod
    def _wrong_dtype(dtype):
        if dtype == torch.float16:
            return ("float16; the kernel takes bfloat16 only.  A pure fp16 model has no loss scaling to train with: torch.amp.GradScaler will not unscale "
                    "16-bit gradients.  Keep fp32 master parameters under torch.autocast(float16) and use FusedAdamW")
        if dtype == torch.float32:
            return "float32; the kernel takes bfloat16 only (fp32 parameters go to zigma_amd.optim.FusedAdamW)"
        return f"{dtype}; the kernel takes bfloat16 only"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, ema=False, ema_decay=0.9999,
                 rounding="stochastic", seed=0, stream=0, *, amsgrad=False, maximize=False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, ema_decay, amsgrad, maximize, rounding=rounding, seed=seed, stream=stream)
        ps = self.param_groups[0]["params"]
        for i, p in enumerate(ps):
            if p.numel() >= MAX_NUMEL16:
                raise ValueError(f"FusedAdamW16: parameter {i} has {p.numel()} elements; the kernel addresses its random bits below 2^35 elements per tensor")
        self._ema_arena, self._ema = None, None
        if ema:
            self._ema_arena, self._ema = arena_views(ps, self.device)
            with torch.no_grad():
                for e, p in zip(self._ema, ps):
                    e.copy_(p)                                                         # bf16 -> fp32: exact
        self._cast_tables = None
        self._allocate(StepTables(width=10, numel_col=5))

    def _check_group_extra(self, g):
        if g["rounding"] not in _ROUNDINGS:
            raise ValueError(f"FusedAdamW16: rounding is one of {_ROUNDINGS}, got {g['rounding']!r}")
        if isinstance(g["seed"], bool) or not isinstance(g["seed"], int) or not 0 <= g["seed"] < 1 << 64:
            raise ValueError(f"FusedAdamW16: seed is an integer in [0, 2^64), got {g['seed']!r}")
        if isinstance(g["stream"], bool) or not isinstance(g["stream"], int) or not 0 <= g["stream"] < 1 << 32:
            raise ValueError(f"FusedAdamW16: stream is an integer in [0, 2^32), got {g['stream']!r}")

    def ema_tensors(self):
        """the fp32 EMA views, parallel to the parameters (live: the step writes them)"""
        if self._ema is None:
            raise RuntimeError("FusedAdamW16: built with ema=False")
        return list(self._ema)

    def copy_ema_to(self, module):
        """writes the EMA, rounded to nearest even, into the bf16 parameters of `module` (a copy of the model: the same parameters in the same order) in
        one zigma_multi_cast_fwd launch"""
        dst = [q.detach() for q in module.parameters()]
        src = self.ema_tensors()
        if len(dst) != len(src):
            raise ValueError(f"FusedAdamW16: the module has {len(dst)} parameters, the optimizer {len(src)}")
        for i, (d, s) in enumerate(zip(dst, src)):
            if d.dtype != torch.bfloat16 or d.shape != s.shape or d.device != s.device or not d.is_contiguous():
                raise ValueError(f"FusedAdamW16: parameter {i} of the module is not a contiguous bfloat16 tensor of shape {tuple(s.shape)} on {s.device}")
        self._cast_tables = amp.cast_tensors(src, dst)                                    # (kept alive past the launch)
        amp._on_optimizer_step(self, (), {})                # the parameters of `module` were written behind their version counters: what is cached of them is stale

    def _install_state(self):
        super()._install_state()
        if self._ema is not None:
            for p, e in zip(self.param_groups[0]["params"], self._ema):
                self.state[p]["ema"] = e

    def load_state_dict(self, state_dict):
        """its own dicts, or torch.optim.AdamW's on the same bf16 model.  Written out here and not left to torch.optim.Optimizer.load_state_dict, which
        casts every floating state tensor to its parameter's dtype: the fp32 moments and EMA would come back rounded to bf16.  A dict without "ema"
        leaves the EMA as it is."""
        import copy
        groups = state_dict["param_groups"]
        ps = self.param_groups[0]["params"]
        if len(groups) != 1:
            raise ValueError("FusedAdamW16: one parameter group only")
        ids = list(groups[0]["params"])
        if len(ids) != len(ps):
            raise ValueError(f"FusedAdamW16: the loaded group has {len(ids)} parameters, this optimizer {len(ps)}")
        old = dict(self.param_groups[0])
        self.param_groups[0].update({k: copy.deepcopy(v) for k, v in groups[0].items() if k != "params"})
        try:
            self._check_group()
        except ValueError:
            self.param_groups[0].clear()
            self.param_groups[0].update(old)
            raise
        state = state_dict["state"]
        loaded = [state.get(i) or None for i in ids]
        step = self._loaded_step(loaded)
        with torch.no_grad():
            for i, st in enumerate(loaded):
                if st is None:
                    self._m[i].zero_()
                    self._v[i].zero_()
                    continue
                self._m[i].copy_(st["exp_avg"])                                           # (a bf16 moment of torch's is widened: exact)
                self._v[i].copy_(st["exp_avg_sq"])
                if self._ema is not None and "ema" in st:
                    self._ema[i].copy_(st["ema"])
            self._restart_at(step)

    # ---- the step ---------------------------------------------------------------------------------------------------------------------------------
    def _rows(self, ps, grads):
        return step_rows16(ps, grads, self._m, self._v, self._ema)

    def _launch(self, g, T, n_rows):
        P = self._fill(_lib.Optim16Params(), g, T, n_rows)
        P.max_numel, P.flags = max(T.numels), _lib.OPTIM16_NEAREST if g["rounding"] == "nearest" else 0
        P.seed_lo, P.seed_hi, P.stream = g["seed"] & 0xffffffff, g["seed"] >> 32, g["stream"]
        Q = self._fill(_lib.OptimParams(), g, T, n_rows)    # the prepare launch is the fp32 path's, on its own block
        Q.shadow_dtype = -1
        self._launches("zigma_optim16_grad_sumsq", P, Q, "zigma_optim16_adamw")


