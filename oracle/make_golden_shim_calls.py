"""The extension calls the reference's OWN `mamba_inner_fn` (MambaInnerFn.forward) makes, recorded as data, so that the call surface of
zigma_amd.extension_shims can be checked without the reference checkout (tests/test_host_cpu.py::test_extension_shims_under_the_reference_python).

The reference's selective_scan_interface.py runs on CPU with `selective_scan_cuda` / `causal_conv1d_cuda` = the shim modules (kernels replaced by the
oracle stand-ins of tests/kernel_standins.py).  Every call into them is recorded: module and entry-point name, argument order, each tensor argument
as a view (shape, strides, storage offset) into a stored copy of its storage — so views that alias one buffer (x and z of one xz) alias again on
replay — and the arity of the result.  Next to each call: what the reference's own pure-torch functions (causal_conv1d_ref, selective_scan_ref)
return for the same operands.  Inputs and the final output are those of tests/golden/mamba_inner.npz.

TEST INFRASTRUCTURE ONLY (needs the reference checkout that oracle/ref_shim.py mounts).
    python -m oracle.make_golden_shim_calls   ->  tests/golden/shim_calls_mamba_inner.npz
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)                                   # repo root: `python -m oracle.make_golden_shim_calls` or `python oracle/make_golden_shim_calls.py`
sys.path.insert(0, os.path.join(ROOT, "tests"))            # kernel_standins
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


class Recorder:
    def __init__(self):
        self.storages = []                                 # (data_ptr, flat float32 copy)
        self.arrs = {}
        self.names = []

    def storage_index(self, t):
        st = t.untyped_storage()
        for i, (ptr, _) in enumerate(self.storages):
            if ptr == st.data_ptr():
                return i
        flat = torch.empty(0, dtype=t.dtype).set_(st, 0, (st.nbytes() // t.element_size(),), (1,))
        self.storages.append((st.data_ptr(), flat.detach().clone().numpy()))
        return len(self.storages) - 1

    def wrap(self, module, name, fn):
        def rec(*args):
            i = len(self.names)
            self.names.append(f"{module}.{name}")
            kinds = []
            for j, a in enumerate(args):
                key = f"c{i}_a{j}"
                if a is None:
                    kinds.append("none")
                elif isinstance(a, torch.Tensor):
                    assert a.dtype == torch.float32, a.dtype
                    kinds.append("tensor")
                    self.arrs[key + "_storage"] = np.int64(self.storage_index(a))
                    self.arrs[key + "_view"] = np.array([a.storage_offset(), a.dim(), *a.shape, *a.stride()], np.int64)
                elif isinstance(a, bool):
                    kinds.append("bool")
                    self.arrs[key + "_value"] = np.bool_(a)
                else:
                    raise TypeError(f"{module}.{name}: argument {j} of type {type(a)}")
            self.arrs[f"c{i}_kinds"] = np.array(kinds)
            res = fn(*args)
            self.arrs[f"c{i}_nret"] = np.int64(len(res) if isinstance(res, (list, tuple)) else -1)
            return res
        return rec


def main():
    import kernel_standins
    with contextlib.redirect_stdout(io.StringIO()):
        _, ref_ssi, ref_cci, _ = ref_shim.reference_modules()          # the reference's pure-torch causal_conv1d_ref / selective_scan_ref
    conv_ref, scan_ref = ref_cci.causal_conv1d_ref, ref_ssi.selective_scan_ref
    rec = Recorder()
    with pytest.MonkeyPatch.context() as mp:
        kernel_standins.install(mp)
        from zigma_amd import _lib, extension_shims
        mp.setattr(_lib, "require_device", lambda *a: torch.device("cpu"))
        ss, cc = types.ModuleType("selective_scan_cuda"), types.ModuleType("causal_conv1d_cuda")
        ss.fwd = rec.wrap("selective_scan_cuda", "fwd", extension_shims.selective_scan_cuda.fwd)
        cc.causal_conv1d_fwd = rec.wrap("causal_conv1d_cuda", "causal_conv1d_fwd", extension_shims.causal_conv1d_cuda.causal_conv1d_fwd)
        mp.setitem(sys.modules, "selective_scan_cuda", ss)
        mp.setitem(sys.modules, "causal_conv1d_cuda", cc)
        mp.syspath_prepend(os.path.join(ref_shim.REF, "dis_causal_conv1d"))
        for pkg, sub in (("dis_mamba", "dis_mamba"), ("dis_mamba.mamba_ssm", "dis_mamba/mamba_ssm"), ("dis_mamba.mamba_ssm.ops", "dis_mamba/mamba_ssm/ops")):
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(ref_shim.REF, sub)]
            mp.setitem(sys.modules, pkg, m)
        for name in ("causal_conv1d", "causal_conv1d.causal_conv1d_interface", "dis_mamba.mamba_ssm.ops.selective_scan_interface"):
            mp.delitem(sys.modules, name, raising=False)
        ssi = importlib.import_module("dis_mamba.mamba_ssm.ops.selective_scan_interface")
        assert ssi.selective_scan_cuda is ss and ssi.causal_conv1d_cuda is cc
        with np.load(os.path.join(OUT, "mamba_inner.npz")) as f:
            g = {k: f[k] for k in f.files}
        T = lambda k: torch.from_numpy(g[k])
        with torch.no_grad():
            out = ssi.mamba_inner_fn(T("xz"), T("conv_w"), T("conv_b"), T("x_proj_w"), T("dt_proj_w"), T("out_proj_w"),
                                     T("out_proj_b"), T("A"), None, None, T("D"), delta_bias=T("delta_bias"), delta_softplus=True)
    assert rec.names == ["causal_conv1d_cuda.causal_conv1d_fwd", "selective_scan_cuda.fwd"], rec.names
    err = float(np.linalg.norm(out.numpy() - g["out"]) / np.linalg.norm(g["out"]))
    assert err < 5e-6, err

    def arg(i, j):
        off, nd, *rest = rec.arrs[f"c{i}_a{j}_view"].tolist()
        flat = torch.from_numpy(rec.storages[int(rec.arrs[f"c{i}_a{j}_storage"])][1])
        return torch.as_strided(flat, rest[:nd], rest[nd:], off)
    with torch.no_grad():
        x, w, b = arg(0, 0), arg(0, 1), arg(0, 2)
        rec.arrs["c0_expect"] = conv_ref(x, w, b, activation="silu").numpy()
        u, delta, A, B, C, D, z, db = (arg(1, j) for j in range(8))
        rec.arrs["c1_expect_out"] = scan_ref(u, delta, A, B, C, D, None, db, True).numpy()
        rec.arrs["c1_expect_out_z"] = scan_ref(u, delta, A, B, C, D, z, db, True).numpy()
    rec.arrs["calls"] = np.array(rec.names)
    for k, (_, flat) in enumerate(rec.storages):
        rec.arrs[f"s{k}"] = flat
    np.savez_compressed(os.path.join(OUT, "shim_calls_mamba_inner.npz"), **rec.arrs)
    print("shim_calls_mamba_inner.npz", rec.names, {f"s{k}": s.shape for k, (_, s) in enumerate(rec.storages)}, f"out vs golden {err:.2e}")


if __name__ == "__main__":
    main()
