"""CPU checks of the fp16 form of the generated main loop of linear4w_kernel (zigma_amd/csrc/gen, generator cfg f16=True): the
linear4w_body_f16.inc the build compiles is what the generator emits (the file is a build product of zigma_amd/build.py — the committed text is
linear4w_body.inc, from which it differs in four mnemonics); the generated TEXT, executed by the simulator on fp16 operands (fp16 rounding = numpy
float16, round to nearest even), computes x @ W^T (+ bias, + gated residual) and keeps the synchronisation discipline; the switch changes
nothing but the four substituted instructions, and with it off the generator returns the bf16 text of linear4w_body.inc.

Bound: the bf16 suite's 3e-3 (tests/test_linear4w_gen.py) divided by 8 — fp16 carries three more mantissa bits; the rounding floor of one
fp16 rounding on these operands is 2.1e-4 norm-wise (2.5e-4 with the gated add), as 1.7e-3 / 2.0e-3 is for bf16."""
import os
import re
import sys

import pytest

from conftest import ROOT

GEN = os.path.join(ROOT, "zigma_amd", "csrc", "gen")
if GEN not in sys.path:
    sys.path.insert(0, GEN)
CSRC = os.path.join(ROOT, "zigma_amd", "csrc")
F16_BOUND = 3e-3 / 8


def _macro_bodies(path):
    """{macro name: [asm lines]} of a generated .inc"""
    out, name = {}, None
    for ln in open(path):
        m = re.match(r"#define (ZIGMA_LINEAR4W\w*BODY\w*) \\", ln)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and ln.startswith('    "') and ln.rstrip().endswith('\\n" \\'):
            out[name].append(ln[5:ln.rindex('\\n" \\')])
        elif name and ln.strip() == '""':
            name = None
    return out


def test_built_f16_inc_is_current(tmp_path):
    """the file the build compiles is the generator's output: the one in the tree if a build left one (a stale one fails here), and in any case
    what zigma_amd.build.ensure_generated writes"""
    import linear4w_gen as G
    from zigma_amd import build as zb
    out = tmp_path / "body_f16.inc"
    G.emit_inc_f16(str(out))
    in_tree = os.path.join(CSRC, "linear4w_body_f16.inc")
    assert zb.GENERATED_F16_INC == in_tree
    if os.path.exists(in_tree):
        assert out.read_text() == open(in_tree).read(), "stale linear4w_body_f16.inc: run `python -m zigma_amd.build`"
    assert zb.ensure_generated(verbose=False) == in_tree and out.read_text() == open(in_tree).read()
    bodies = _macro_bodies(str(out))
    assert sorted(bodies) == ["ZIGMA_LINEAR4W_F16_BODY", "ZIGMA_LINEAR4W_F16_BODY_N", "ZIGMA_LINEAR4W_F16_BODY_NR", "ZIGMA_LINEAR4W_F16_BODY_NRB"]
    for name, cfg in G.VARIANTS.items():
        assert bodies["ZIGMA_LINEAR4W_F16_BODY" + name] == G.generate(dict(cfg, f16=True))[0]


@pytest.mark.parametrize("case", range(12))
def test_generated_f16_loop_in_the_simulator(case):
    """all 12 simulator cases (every kernel variant, width changes, wraps, odd and even k-step counts, all wave orders) on fp16 operands"""
    import linear4w_sim as S
    M, N, K, n_wg, wg, order, cfg, rpb = S.CASES[case]
    r = S.check(M, N, K, n_wg, wg, order, cfg=dict(cfg, f16=True), rows_per_batch=rpb)
    print(f"case {case}: rel err {r and r[0]:.3e}")
    assert r is not None and r[0] < F16_BOUND


def test_switch_off_returns_todays_text():
    """generate() without the switch (and with f16=False) is, line for line, the bf16 body committed in linear4w_body.inc"""
    import linear4w_gen as G
    committed = _macro_bodies(os.path.join(CSRC, "linear4w_body.inc"))
    for name, cfg in G.VARIANTS.items():
        lines, T = G.generate(cfg)
        assert lines == committed["ZIGMA_LINEAR4W_BODY" + name], name
        assert G.generate(dict(cfg, f16=False)) == (lines, T)
        assert not any("f16" in ln.replace("bf16", "") for ln in lines), name


def test_f16_substitution_is_one_for_one():
    """same instruction count, same placement: the f16 text differs from the bf16 text only in the four substituted instructions (MFMA,
    packed conversion, the two halves of the 16-bit unpack), so no other instruction — no store of any other kind, no wait — came or went"""
    import linear4w_gen as G
    subst = [(r"^v_mfma_f32_32x32x16_bf16 (.*)$", r"^v_mfma_f32_32x32x16_f16 (.*)$"),
             (r"^v_cvt_pk_bf16_f32 (.*)$", r"^v_cvt_pk_f16_f32 (.*)$"),
             (r"^v_lshlrev_b32 (v\d+), 16, (v\d+)$", r"^v_cvt_f32_f16 (v\d+), (v\d+)$"),
             (r"^v_and_b32 (v\d+), 0xffff0000, (v\d+)$", r"^v_cvt_f32_f16_sdwa (v\d+), (v\d+) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1$")]
    for name, cfg in G.VARIANTS.items():
        b, Tb = G.generate(cfg)
        h, Th = G.generate(dict(cfg, f16=True))
        assert len(b) == len(h) and Tb == Th, name
        n_diff = 0
        for lb, lh in zip(b, h):
            if lb == lh:
                assert "bf16" not in lb, lb
                continue
            n_diff += 1
            assert any((mb := re.match(pb, lb)) and (mh := re.match(ph, lh)) and mb.groups() == mh.groups() for pb, ph in subst), (lb, lh)
        assert n_diff > 0


def test_f16_simulation_catches_a_missing_wait():
    """the f16 run of the checker is not vacuous either"""
    import linear4w_gen as G
    import linear4w_sim as S
    lines, T = G.generate(dict(f16=True))
    start = lines.index("L_first0_w_0_%=:")
    j = next(k for k in range(start, len(lines)) if lines[k].startswith("s_waitcnt lgkmcnt(0)"))
    with pytest.raises(S.SimError):
        S.check(256, 256, 192, 8, 0, gen=(lines[:j] + lines[j + 1:], T), cfg=dict(f16=True))
