"""Host side of mixed precision (zigma_amd/amp.py, zigma_multi_cast_fwd): the parameter block's ctypes mirror, the chunk map, the arena layout.  No GPU."""
import ctypes
import os
import random
import subprocess
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_cast_struct_matches_the_header():
    """sizeof / offsetof of the new parameter block and its two table rows as gcc sees include/zigma_hip.h (the recipe of
    test_ctypes_structs_match_the_header); the rows are what amp.py writes as int64 triples / pairs"""
    from zigma_amd import _lib
    st = _lib.MultiCastParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(zigma_multi_cast_params_t));']
    for f, _ in st._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(zigma_multi_cast_params_t, {f}));')
    lines.append('printf("row_entry %zu %zu %zu %zu\\n", sizeof(zigma_multi_cast_entry_t), offsetof(zigma_multi_cast_entry_t, src), '
                 'offsetof(zigma_multi_cast_entry_t, dst), offsetof(zigma_multi_cast_entry_t, numel));')
    lines.append('printf("row_chunk %zu %zu %zu\\n", sizeof(zigma_multi_cast_chunk_t), offsetof(zigma_multi_cast_chunk_t, entry), '
                 'offsetof(zigma_multi_cast_chunk_t, offset));')
    lines.append('printf("abi %d\\n", ZIGMA_ABI_VERSION);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in out.strip().splitlines()}
    assert got["size"] == [ctypes.sizeof(st)]
    for f, _ in st._fields_:
        assert got[f] == [getattr(st, f).offset], f
    assert got["row_entry"] == [24, 0, 8, 16] and got["row_chunk"] == [16, 0, 8]
    assert got["abi"] == [11]
    assert "zigma_multi_cast_fwd" in _lib.EXPORTS
    from zigma_amd import build
    assert "multi_cast.hip" in build.SOURCES and build.SOURCE_FLAGS["multi_cast.hip"] == build._RES and "multi_cast_kernel" in build.NO_SCRATCH_KERNELS


def test_chunk_map_covers_every_element_exactly_once():
    from zigma_amd import amp
    rnd = random.Random(7)
    for chunk in (8, 64, 4096):
        edge = [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
        for trial in range(6):
            sizes = edge + [rnd.randrange(0, 5 * chunk) for _ in range(rnd.randrange(0, 12))]
            rnd.shuffle(sizes)
            rows = amp.build_chunk_map(sizes, chunk)
            hits = [[0] * n for n in sizes]
            for e, o in rows:
                assert 0 <= e < len(sizes) and 0 <= o < sizes[e] and o % chunk == 0
                for i in range(o, min(o + chunk, sizes[e])):
                    hits[e][i] += 1
            assert all(h == 1 for t in hits for h in t)
            assert len(rows) == sum(-(-n // chunk) for n in sizes)
    assert amp.build_chunk_map([], 4096) == [] and amp.build_chunk_map([0, 0], 4096) == []


def test_arena_layout_slots_are_aligned_shaped_like_the_parameters_and_disjoint():
    from zigma_amd import amp
    shapes = [(72, 128), (128, 8), (3,), (0,), (1,), (257,), (640, 2560), (5, 7, 3)]
    params = [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    offsets, total = amp.arena_layout([p.numel() for p in params])
    assert all(o % 256 == 0 for o in offsets) and total % 256 == 0
    spans = sorted((o, o + 2 * p.numel()) for o, p in zip(offsets, params) if p.numel())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    grp = amp._Group(params)
    for dtype in (torch.bfloat16, torch.float16):
        a = grp._arena(dtype)
        ends = []
        for p, sh in zip(params, a["shadows"]):
            assert sh.dtype == dtype and sh.shape == p.shape and sh.stride() == p.stride() and sh.is_contiguous()
            assert sh.data_ptr() % 256 == 0
            if p.numel():
                ends.append((sh.data_ptr(), sh.data_ptr() + 2 * p.numel()))
        ends.sort()
        assert all(x[1] <= y[0] for x, y in zip(ends, ends[1:]))
        lo, hi = a["arena"].data_ptr(), a["arena"].data_ptr() + a["arena"].numel()
        assert lo <= ends[0][0] and ends[-1][1] <= hi
    assert grp._arena(torch.bfloat16)["arena"].data_ptr() != grp._arena(torch.float16)["arena"].data_ptr()


def test_matrix_parameters_of_a_text_model_and_cpu_shadow():
    """which parameters attach() registers (every projection weight and the biases those products add; not the conv taps, norms, adaLN, embedders),
    and the `.to()` path of shadow() for tensors the kernel does not take"""
    from zigma_amd import amp
    from zigma_amd.model_zigma import ZigMa
    m = ZigMa(in_channels=4, embed_dim=64, depth=2, img_dim=8, patch_size=1, has_text=True, d_context=32, n_context_token=7, scan_type="zigzagN8",
              use_pe=2, device="cpu")
    names = {id(p): n for n, p in m.named_parameters()}
    got = sorted(names[id(p)] for p in amp.matrix_parameters(m))
    want = ["y_embedder.weight", "y_embedder.bias"]
    for i in range(2):
        want += [f"blocks.{i}.mixer.{n}.weight" for n in ("in_proj", "x_proj", "dt_proj", "out_proj")]
        want += [f"blocks.{i}.msa.{n}.weight" for n in ("to_q", "to_k", "to_v", "to_out.0")] + [f"blocks.{i}.msa.to_out.0.bias"]
    assert got == sorted(want)
    grp = amp.attach(m)
    assert grp.params == [] and m._amp_group is grp and "_amp_group" not in m.state_dict()      # CPU parameters are not the kernel's
    before = dict(amp.STATS)
    p = m.blocks[0].mixer.x_proj.weight
    s = amp.shadow(p, torch.bfloat16)
    assert torch.equal(s, p.detach().to(torch.bfloat16)) and not s.requires_grad and amp.STATS == before


def test_optimizer_steps_are_counted_from_import_and_key_the_caches():
    """torch's fused optimizers write parameters without moving `_version`: the package counts optimizer steps from import on (no attach needed) and
    every cache derived from parameters carries the count — here Mamba._scan_consts, on the CPU"""
    from zigma_amd import amp
    from zigma_amd.mamba_simple import Mamba
    mx = Mamba(32, device="cpu")
    with torch.no_grad():
        a0 = mx._scan_consts("")[0].clone()
        assert mx._scan_consts("")[0] is mx._scan_consts("")[0]                     # cached
    opt = torch.optim.AdamW([mx.A_log], lr=0.1, fused=True)
    mx.A_log.grad = torch.ones_like(mx.A_log)
    before = amp.step_count()
    opt.step()
    assert amp.step_count() == before + 1
    with torch.no_grad():
        a1 = mx._scan_consts("")[0]
    assert torch.equal(a1, -torch.exp(mx.A_log.detach())) and not torch.equal(a1, a0)


def test_plan_stand_in_reads_like_the_shadow():
    from zigma_amd import amp
    p = torch.nn.Parameter(torch.randn(640, 1280))
    like = amp.Like(p, torch.bfloat16)
    sh = p.detach().to(torch.bfloat16)
    assert like.dtype == sh.dtype and like.shape == sh.shape and like.stride() == sh.stride() and like.stride(0) == 1280 and like.stride(1) == 1
    assert like.dim() == 2 and like.numel() == sh.numel() and like.is_contiguous() and like.data_ptr() % 256 == 0 and not like.requires_grad
    b = amp.Like(torch.nn.Parameter(torch.randn(640)), torch.float16)
    assert b.stride(0) == 1 and b.shape == (640,)
