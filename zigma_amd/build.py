"""Build libzigma_hip.so (gfx950) in-tree with hipcc.  `python -m zigma_amd.build [--force]`."""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "lib", "libzigma_hip.so")
SOURCES = ["api.hip", "selective_scan.hip", "scan_tok_bf16.hip", "scan_tok_f16.hip", "scan_tok_f32.hip",
           "causal_conv1d.hip", "add_norm.hip", "dt_proj.hip", "scan_bwd.hip", "conv_bwd.hip", "norm_bwd.hip", "cross_attn.hip", "cross_attn_bwd.hip", "x_proj.hip", "linear.hip", "linear4w.hip", "linear_ws.hip", "linear_sm.hip", "conv_x_proj.hip", "glue_bwd.hip", "embed.hip", "skinny_linear.hip", "calib.hip", "wgrad.hip", "linear_split.hip", "norm_linear.hip", "multi_cast.hip", "optim_step.hip", "sde_step.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-fno-slp-vectorize",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


# per-source flags.  cross_attn.hip: MFMA results in VGPRs — its accumulators are consumed by VALU code right away (softmax, normalisation);
# left to the default (AGPR destinations in a kernel with registers to spare) every result costs a v_accvgpr_read_b32
# (the same switch on conv_x_proj.hip and cross_attn_bwd.hip removes their AGPR moves too and changes nothing measurable: 17.21-17.28 vs
# 17.23-17.26 ms per forward, 97.5-98.2 vs 96.8-98.0 ms per training step, tools/fwd_vgpr_mfma_ab.sh)
_VGPR_MFMA = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
# scan_tok2_kernel loads its bf16 rows with inline-asm `buffer_load_short_d16_hi` (csrc/scan_tok2.inc): the compiler does not see those writes, so a spill or
# a live-range split of the destination registers between the load and the tile's fence would silently lose a row.  The two TUs that instantiate
# the kernel are compiled with the resource-usage remarks on, and the build FAILS if any instantiation uses scratch memory or spills a register.
_RES = ["-Rpass-analysis=kernel-resource-usage"]
# wgrad_kernel (csrc/wgrad.hip) holds its accumulators and one prefetched step in registers at 3 - 4 workgroups per CU: scratch would cost it the stream rate, so
# the same check guards its instantiations.
# linear_split_kernel (csrc/linear_split.hip) keeps up to 128 accumulator registers and one prefetched k-step (64 registers) per lane: the same check.
# norm_linear_kernel (csrc/norm_linear.hip) holds its 32 rows as MFMA fragments (up to 192 registers) next to the accumulators of a pass at two waves per SIMD:
# a silent spill would decide its speed, so the same check.
# multi_cast_kernel (csrc/multi_cast.hip) is a pure stream of 16-byte accesses: scratch traffic would come straight off its copy rate, so the same check.
# final_layer_cfg_kernel (csrc/embed.hip) keeps a row of up to 2048 features (128 registers per lane) through two statistics passes and the dot products, twice per
# output: the same check.
# multi_sumsq_kernel and multi_adamw_kernel (csrc/optim_step.hip; 2 + 5 instantiations, fp32 and bf16 parameters) stream up to ten 16-byte accesses per lane and
# iteration and hold 40 values between them, the stochastically rounding store adds a Philox call per lane and iteration: the same check.
# sde_step_kernel (csrc/sde_step.hip) calls the library's logf and sincospif, whose results come back through pointers: a pointer left in scratch would put memory
# traffic into a kernel that has none to spare, so the same check.
SOURCE_FLAGS = {"cross_attn.hip": _VGPR_MFMA, "scan_tok_bf16.hip": _RES, "scan_tok_f16.hip": _RES, "wgrad.hip": _RES, "linear_split.hip": _RES, "norm_linear.hip": _RES, "multi_cast.hip": _RES, "optim_step.hip": _RES, "embed.hip": _RES, "sde_step.hip": _RES}
NO_SCRATCH_KERNELS = ("scan_tok2_kernel", "wgrad_kernel", "wgrad_reduce_kernel", "linear_split_kernel", "norm_linear_kernel", "multi_cast_kernel", "multi_sumsq_kernel",
                      "multi_adamw_kernel", "final_layer_cfg_kernel", "sde_step_kernel")


def check_no_scratch(remarks, src):
    """parse -Rpass-analysis=kernel-resource-usage output: every NO_SCRATCH_KERNELS instantiation must report ScratchSize 0 and no spills"""
    import re
    bad, seen, name = [], 0, None
    for ln in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = m.group(1) if any(k in m.group(1) for k in NO_SCRATCH_KERNELS) else None
            seen += name is not None
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and name and int(m.group(2)) != 0:
            bad.append((name, m.group(1), int(m.group(2))))
    if bad or not seen:
        raise RuntimeError(f"{src}: {' / '.join(NO_SCRATCH_KERNELS)} must not spill or use scratch (scan_tok2_kernel: inline-asm d16_hi row loads are invisible to the register allocator): "
                           f"{bad if bad else 'no instantiation found in the remarks'}")
    return seen


GENERATED_F16_INC = os.path.join(CSRC, "linear4w_body_f16.inc")


def ensure_generated(verbose=True):
    """csrc/linear4w_body_f16.inc — the fp16 bodies of linear4w_kernel's generated main loop (csrc/gen/linear4w_gen.py, cfg f16=True) — is a build
    product, not a committed file: its 19 400 lines are the committed bf16 text of linear4w_body.inc with four mnemonics substituted one for one
    (tests/test_linear4w_gen_f16.py checks exactly that).  (Re)written here when missing or not what the generator emits; takes about a second."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("zigma_linear4w_gen", os.path.join(CSRC, "gen", "linear4w_gen.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    tmp = GENERATED_F16_INC + ".tmp"
    gen.emit_inc_f16(tmp)
    if os.path.exists(GENERATED_F16_INC) and open(GENERATED_F16_INC).read() == open(tmp).read():
        os.remove(tmp)
        return GENERATED_F16_INC
    os.replace(tmp, GENERATED_F16_INC)
    if verbose:
        print(f"generated {GENERATED_F16_INC}", flush=True)
    return GENERATED_F16_INC


def _digest(paths, extra=()):
    h = hashlib.sha256()
    for pth in sorted(paths):
        h.update(os.path.basename(pth).encode())
        h.update(open(pth, "rb").read())
    for e in extra:
        h.update(str(e).encode())
    return h.hexdigest()


def build(force=False, verbose=True, sources=None, lib=None, extra_flags=()):
    """Compile every .hip of csrc/ and link the shared library.  Staleness is decided by a CONTENT hash of the
    sources + flags stored next to the library (mtimes do not survive the snapshot copy to the GPU box, and a
    library that already matches its sources must not be rebuilt there)."""
    sources = sources or SOURCES
    lib = lib or LIB
    obj_dir = OBJ if lib == LIB else OBJ + "_" + os.path.splitext(os.path.basename(lib))[0]      # (A/B libraries of tools/ keep their own objects)
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    ensure_generated(verbose)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    headers.append(os.path.join(ROOT, "include", "zigma_hip.h"))
    stamp = lib + ".srchash"
    want = _digest([os.path.join(CSRC, s) for s in sources] + headers, extra=list(FLAGS) + list(extra_flags) + [str(sorted(SOURCE_FLAGS.items()))])
    if not force and os.path.exists(lib) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        if verbose:
            print(f"{lib} is up to date (source hash {want[:12]})")
        return lib

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    objs, jobs = [], []
    for src in sources:
        s_path = os.path.join(CSRC, src)
        o_path = os.path.join(obj_dir, src.replace(".hip", ".o"))
        o_stamp = o_path + ".srchash"
        src_flags = SOURCE_FLAGS.get(src, [])
        o_want = _digest([s_path] + headers, extra=list(FLAGS) + list(extra_flags) + src_flags)
        objs.append(o_path)
        if force or not os.path.exists(o_path) or not os.path.exists(o_stamp) or open(o_stamp).read().strip() != o_want:
            jobs.append(([HIPCC, *FLAGS, *extra_flags, *src_flags, "-c", s_path, "-o", o_path], o_stamp, o_want))

    def compile_one(job):
        cmd, o_stamp, o_want = job
        if _RES[0] in cmd:
            if verbose:
                print(" ".join(cmd), flush=True)
            r = subprocess.run(cmd, check=True, capture_output=True, text=True)
            n = check_no_scratch(r.stderr, cmd[-3])
            if verbose:
                print(f"  {os.path.basename(cmd[-3])}: {n} checked kernel instantiations, no scratch, no spills", flush=True)
        else:
            run(cmd)
        open(o_stamp, "w").write(o_want)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(compile_one, jobs))
    run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib])
    open(stamp, "w").write(want)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv)
