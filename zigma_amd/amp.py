"""Mixed precision under torch.autocast: fp32 parameters, 16-bit compute on the own kernels.

The reference trains this way (train_acc.py:122 hands `mixed_precision` to accelerate, which wraps the forward in torch.autocast; MambaInnerFn and
the Triton norm carry custom_fwd / custom_bwd for it, selective_scan_interface.py:295-312,368).  The own projection, x_proj, dt_proj and scan kernels
read matrix operands of ONE 16-bit type, so an fp32 model under autocast needs 16-bit copies ("shadows") of its matrix weights.  This module keeps them:

  attach(module)     registers the module's matrix weights (and the biases those products add) and lays their shadows out in one arena per 16-bit
                     type: every slot on a 256-byte boundary, every shadow with the parameter's shape and contiguous strides
  shadow(p, dtype)   the 16-bit copy of p.  A registered parameter's copy lives in the arena, and the WHOLE arena is refreshed by one
                     zigma_multi_cast_fwd launch when a registered parameter's (_version, data_ptr()) has moved since the last refresh, or an
                     optimizer has stepped since (torch's fused optimizers update parameters WITHOUT moving _version, so the package installs
                     a global optimizer-step hook at import that counts steps: step_count()) — once per optimizer step; two forwards without a step in between, or a
                     step that a GradScaler skipped, cast nothing; nor does a forward after a step of zigma_amd.optim.FusedAdamW, which writes the
                     shadows in its own pass (written_by_step).  An unregistered fp32 parameter gets a one-entry launch of
                     the same kernel; what the kernel does not take (non-contiguous, not fp32, not on a GPU) takes `.to()`
  operands(x, w, b)  what a projection under autocast reads: the shadows of (w, b) if x is already in the autocast type and w is fp32, else (w, b)

USE_SHADOWS = False is the A/B partner: a `.to()` per use, the same numbers (ZIGMA_KNOBS="amp.USE_SHADOWS=False").  STATS counts the launches."""
import weakref

import torch

from . import _knobs, _lib

USE_SHADOWS = True
CHUNK = 4096              # elements per workgroup of zigma_multi_cast_fwd: 256 lanes x 8 elements x 2 rounds
SLOT_ALIGN = 256          # bytes; the projection kernels ask for 16
STATS = {"refresh_launches": 0, "single_casts": 0}
_knobs.apply(globals(), "amp")

_DTYPES = (torch.bfloat16, torch.float16)
_REG = {}                 # id(parameter) -> (weakref to its _Group, index in it)
_EPOCH = [0]              # optimizer steps seen by the hook below
_HOOK = []


def _on_optimizer_step(optimizer, args, kwargs):
    _EPOCH[0] += 1


def step_count():
    """optimizer steps of this process (a cache key beside `_version` for everything this package derives from parameters and caches: the shadows,
    Mamba._scan_consts, ZigMa._batched_conditioning, fp32_matmul's weight planes)"""
    return _EPOCH[0]


def _watch_optimizers():
    """count every torch.optim step of the process: `fused=True` optimizers write the parameters without moving their version counters.  Installed when
    the package is imported, so that the caches of a model that never runs under autocast see the steps too."""
    if not _HOOK:
        from torch.optim.optimizer import register_optimizer_step_post_hook
        _HOOK.append(register_optimizer_step_post_hook(_on_optimizer_step))


_watch_optimizers()


def Like(p, dtype, k=2):
    """What a shadow of parameter p WILL look like, as the planning predicates read a tensor (device, dtype, shape, contiguous strides, an aligned address,
    no grad): arena slots start on 256-byte boundaries and a fresh `.to()` is an aligned allocation, so a plan needs no cast.  The k-th placeholder of its block."""
    return _lib.Desc.fresh(p, tuple(p.shape), k, dtype)


def autocast_dtype():
    return torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()


def build_chunk_map(numels, chunk=CHUNK):
    """[(entry, offset)] — one row per workgroup: tensor `entry`, elements [offset, min(offset + chunk, numel)).  Empty tensors get no row."""
    rows = []
    for e, n in enumerate(numels):
        rows.extend((e, o) for o in range(0, int(n), chunk))
    return rows


def arena_layout(numels, itemsize=2, align=SLOT_ALIGN):
    """byte offset of every slot (each on an `align`-byte boundary, in order, nothing overlapping) and the arena's size in bytes"""
    offsets, at = [], 0
    for n in numels:
        offsets.append(at)
        at += -(-int(n) * itemsize // align) * align
    return offsets, at


def multi_cast(table, chunk_map, n_entries, n_chunks, dtype, device, chunk=CHUNK):
    """one zigma_multi_cast_fwd launch; table (n_entries, 3) and chunk_map (n_chunks, 2) are int64 DEVICE tensors (include/zigma_hip.h)"""
    P = _lib.MultiCastParams()
    P.table, P.chunk_map, P.n_entries, P.n_chunks = _lib.ptr(table), _lib.ptr(chunk_map), n_entries, n_chunks
    P.out_dtype, P.chunk, P.flags = _lib._DT.get(dtype, -1), chunk, 0
    _lib.call("zigma_multi_cast_fwd", P, device)


def cast_tensors(srcs, dsts, chunk=CHUNK):
    """dsts[i] = srcs[i] rounded to dsts' 16-bit type, all in one launch (contiguous fp32 sources / 16-bit destinations on one device).
    Returns the (table, chunk_map) device tensors, which must outlive the launch."""
    dev = _lib.require_device(*srcs, *dsts)
    rows = [(s.data_ptr(), d.data_ptr(), s.numel()) for s, d in zip(srcs, dsts)]
    cmap = build_chunk_map([r[2] for r in rows], chunk)
    table = torch.tensor(rows or [(0, 0, 0)], dtype=torch.int64).to(dev)
    cm = torch.tensor(cmap or [(0, 0)], dtype=torch.int64).to(dev)
    multi_cast(table, cm, len(rows), len(cmap), dsts[0].dtype if dsts else torch.bfloat16, dev, chunk)
    return table, cm


def _takes_kernel(p):
    return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()


class _Group:
    """the registered parameters of one attach() and, per 16-bit type, their arena"""

    def __init__(self, params):
        self.params = params
        self.numels = [p.numel() for p in params]
        self.offsets, self.nbytes = arena_layout(self.numels)
        self.cmap_rows = build_chunk_map(self.numels)
        self.arenas = {}          # dtype -> dict(arena, shadows, table, cmap, ptrs, keys)

    def _arena(self, dtype):
        a = self.arenas.get(dtype)
        if a is None:
            dev = self.params[0].device
            arena = torch.empty(max(self.nbytes, SLOT_ALIGN) + SLOT_ALIGN, device=dev, dtype=torch.uint8)
            arena = arena[(-arena.data_ptr()) % SLOT_ALIGN:][:max(self.nbytes, SLOT_ALIGN)]
            shadows = [arena[o:o + 2 * n].view(dtype).view(p.shape) for p, o, n in zip(self.params, self.offsets, self.numels)]
            cmap = torch.tensor(self.cmap_rows or [(0, 0)], dtype=torch.int64).to(dev)
            a = dict(arena=arena, shadows=shadows, table=None, cmap=cmap, ptrs=None, keys=[None] * len(self.params))
            self.arenas[dtype] = a
        return a

    def get(self, i, dtype):
        a = self._arena(dtype)
        p = self.params[i]
        if a["keys"][i] != (_EPOCH[0], p._version, p.data_ptr()):
            self.refresh(dtype)
        return a["shadows"][i]

    def refresh(self, dtype):
        """the whole arena in one launch (the table of source addresses is rebuilt only when a parameter's storage has moved)"""
        a = self._arena(dtype)
        ptrs = [p.data_ptr() for p in self.params]
        if a["ptrs"] != ptrs:
            rows = [(s, d.data_ptr(), n) for s, d, n in zip(ptrs, a["shadows"], self.numels)]
            a["table"], a["ptrs"] = torch.tensor(rows, dtype=torch.int64).to(a["arena"].device), ptrs
        multi_cast(a["table"], a["cmap"], len(self.params), len(self.cmap_rows), dtype, a["arena"].device)
        a["keys"] = [(_EPOCH[0], p._version, q) for p, q in zip(self.params, ptrs)]
        STATS["refresh_launches"] += 1

    def fresh(self, dtype):
        """does the `dtype` arena hold the parameters as they are now — would get() hand out every shadow without a refresh?"""
        a = self.arenas.get(dtype)
        return a is not None and all(k == (_EPOCH[0], p._version, p.data_ptr()) for k, p in zip(a["keys"], self.params))

    def written_by_step(self, dtype):
        """an optimizer that writes the shadows itself (zigma_amd.optim.FusedAdamW) records, inside its step(), that the arena holds the parameters
        as of the step BEING taken: the keys carry the count the optimizer-step hook is about to reach, so the next forward refreshes nothing.
        Only for an arena that was fresh() before the step: a step the device skipped then leaves parameters and arena alike untouched."""
        a = self._arena(dtype)
        a["keys"] = [(_EPOCH[0] + 1, p._version, p.data_ptr()) for p in self.params]


def matrix_parameters(module):
    """the parameters attach() registers: every weight a projection or a GEMM inside an autograd Function of this package consumes — in_proj, out_proj,
    x_proj, dt_proj and their `_b` twins, to_q / to_k / to_v, to_out, the y_embedder of text models — and the biases those products add (dt_proj's bias
    is the scan's fp32 delta_bias, not a GEMM's)"""
    from .mamba_simple import Mamba
    from .model_zigma import CrossAttention, ZigMa
    out = []
    for m in module.modules():
        lins = []
        if isinstance(m, Mamba):
            lins = [(getattr(m, n + sfx, None), n != "dt_proj") for sfx in ("", "_b") for n in ("in_proj", "x_proj", "dt_proj")] + [(m.out_proj, True)]
        elif isinstance(m, CrossAttention):
            lins = [(m.to_q, True), (m.to_k, True), (m.to_v, True), (m.to_out[0], True)]
        elif isinstance(m, ZigMa) and m.has_text:
            lins = [(m.y_embedder, True)]
        for lin, with_bias in lins:
            if isinstance(lin, torch.nn.Linear):
                out.append(lin.weight)
                if with_bias and lin.bias is not None:
                    out.append(lin.bias)
    seen, uniq = set(), []
    for p in out:
        if id(p) not in seen and p.is_floating_point():
            seen.add(id(p))
            uniq.append(p)
    return uniq


def attach(module):
    """register `module`'s matrix weights; returns the group (kept alive by the module).  Parameters the cast kernel does not take stay unregistered."""
    params = [p for p in matrix_parameters(module) if _takes_kernel(p)]
    if params:
        params = [p for p in params if p.device == params[0].device]
    grp = _Group(params)
    ref = weakref.ref(grp)
    for i, p in enumerate(params):
        _REG[id(p)] = (ref, i)
    module.__dict__["_amp_group"] = grp           # (not a submodule, not in the state_dict)
    for k in [k for k, (r, _) in _REG.items() if r() is None]:
        del _REG[k]
    return grp


def attached(module):
    """does `module` carry a group of ITS OWN parameters?  A copy.deepcopy / unpickled copy of an attached model carries a copy of the group whose
    parameters are registered nowhere: the caller attaches the copy again."""
    grp = module.__dict__.get("_amp_group")
    if grp is None:
        return False
    if not grp.params:
        return True
    hit = _REG.get(id(grp.params[0]))
    return hit is not None and hit[0]() is grp


def shadow(p, dtype):
    """the `dtype` copy of parameter p (a detached tensor that requires no grad)"""
    if dtype not in _DTYPES:
        raise RuntimeError(f"amp.shadow: {dtype} is not a 16-bit autocast type")
    if not USE_SHADOWS or not _takes_kernel(p):
        return p.detach().to(dtype)
    hit = _REG.get(id(p))
    if hit is not None:
        grp = hit[0]()
        if grp is not None and grp.params[hit[1]] is p:
            return grp.get(hit[1], dtype)
    out = torch.empty(p.shape, device=p.device, dtype=dtype)
    keep = cast_tensors([p.detach()], [out])
    STATS["single_casts"] += 1
    del keep                                       # (the caching allocator hands the table's block out again in stream order only)
    return out


def operands(x, weight, bias=None):
    """(weight, bias) as a product with x reads them under autocast: their shadows when x already is in the autocast type and weight is fp32"""
    d = autocast_dtype()
    if d not in _DTYPES or x.dtype != d or weight.dtype != torch.float32 or not weight.is_cuda:
        return weight, bias
    return shadow(weight, d), (shadow(bias, d) if bias is not None and bias.dtype == torch.float32 else bias)


def planned(x, weight, bias=None):
    """operands() for a PLAN: stand-ins (Like) instead of the shadows — no cast, no launch; same dtype, shape, strides and alignment"""
    d = autocast_dtype()
    if d not in _DTYPES or x.dtype != d or weight.dtype != torch.float32 or not weight.is_cuda:
        return weight, bias
    return Like(weight, d), (Like(bias, d, 3) if bias is not None and bias.dtype == torch.float32 else bias)


def mixed(x, weight):
    """is (x, weight) the mixed-precision case: autocast on, x in the autocast type, an fp32 weight on the device"""
    return torch.is_autocast_enabled() and weight.dtype == torch.float32 and weight.is_cuda and x.dtype == autocast_dtype() and x.dtype in _DTYPES
