"""The dispatch tables of the nine entry points whose limits Python asks the library about outside the Mamba inner and the dense projections:
plan_patch_embed(), plan_timestep_embed(), plan_final_layer(), plan_final_layer_cfg(), plan_skinny_linear() (zigma_amd/csrc/outer_plan.h),
plan_cross_attn(), plan_cross_attn_bwd(), plan_scale_reduce_bwd() (csrc/attn_plan.h) and plan_wgrad() (csrc/wgrad_plan.h) — one case per leaf of the
plans: every refusal clause, the empty calls, every serving leaf at the smallest shape that tells it from its neighbour.

Each case is a small call of the product's own block builder (embed.*_block, attention.cross_attn*_block, layernorm.glue_bwd_block, wgrad.wgrad_block) on
real operands and outputs, and what the library reports for it: status and zigma_last_kernel().  A refusal case breaks its check AND a later one where it
can, so that two checks in the wrong order change its status.  test_host_cpu.py checks the table against the plans compiled with g++ and the built
library's queries, test_gpu_outer_plan_query.py against the launches on the GPU.
"""
import ctypes
from collections import namedtuple

import torch

from zigma_amd import _lib

Expect = namedtuple("Expect", "status kernel")      # kernel None: nothing launched, nothing reported
OK, NULL, SHAPE, DTYPE, STRIDE, UNSUPPORTED = 0, -1, -2, -3, -4, -6
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _ok(kernel):
    return Expect(OK, kernel)


def _no(status):
    return Expect(status, None)


def _plus(field, nbytes):
    """patch value: the pointer the builder wrote, moved by nbytes"""
    return lambda P: getattr(P, field) + nbytes


PE, TE, FL, CFG, SK = "patch_embed", "timestep_embed", "final_layer", "final_layer_cfg", "skinny_linear_mfma"
XA, XB, GB = "cross_attn_mfma", "cross_attn_bwd_mfma", "scale_reduce_bwd"
# name: (entry, case, expected).  patch: parameter-block fields set after the builder has filled the block; only refused and empty cases carry one, so
# nothing is ever launched on a block that does not describe its tensors.  Defaults of the entries: see their builders below.
CASES = {
    # -- zigma_patch_embed_fwd: bf16, B=2, C=4, 8 x 8 pixels, patch 2 (K = 16), E=64, bias, position table
    "pe_shape_negative_batch": ("patch_embed", dict(patch=dict(batch=-1, flags=1)), _no(SHAPE)),
    "pe_shape_embed_dim_4": ("patch_embed", dict(patch=dict(embed_dim=4, flags=1)), _no(SHAPE)),
    "pe_shape_patch_0": ("patch_embed", dict(patch=dict(patch=0, dtype=_lib.F16)), _no(SHAPE)),
    "pe_unsupported_flag_on_empty": ("patch_embed", dict(B=0, patch=dict(flags=1, dtype=_lib.F16)), _no(UNSUPPORTED)),
    "pe_dtype_f16": ("patch_embed", dict(patch=dict(dtype=_lib.F16, embed_dim=12)), _no(DTYPE)),
    "pe_dtype_f32": ("patch_embed", dict(patch=dict(dtype=_lib.F32, height=9)), _no(DTYPE)),
    "pe_shape_embed_dim_12": ("patch_embed", dict(patch=dict(embed_dim=12, x=None)), _no(SHAPE)),
    "pe_shape_height_9": ("patch_embed", dict(patch=dict(height=9, x=None)), _no(SHAPE)),
    "pe_shape_width_9": ("patch_embed", dict(patch=dict(width=9, x=None)), _no(SHAPE)),
    "pe_shape_weight_above_64KB": ("patch_embed", dict(patch=dict(in_chans=16, embed_dim=264, x=None)), _no(SHAPE)),          # 64 x 264 x 4 bytes
    "pe_empty": ("patch_embed", dict(B=0, patch=dict(x=None)), Expect(OK, None)),
    "pe_null_x": ("patch_embed", dict(patch=dict(x=None, out=_plus("out", 8))), _no(NULL)),
    "pe_null_weight": ("patch_embed", dict(patch=dict(weight=None, out_row_stride=68)), _no(NULL)),
    "pe_null_out": ("patch_embed", dict(patch=dict(out=None, batch=65536)), _no(NULL)),
    "pe_stride_out_plus_8_bytes": ("patch_embed", dict(patch=dict(out=_plus("out", 8), batch=65536)), _no(STRIDE)),
    "pe_stride_out_pitch_68": ("patch_embed", dict(patch=dict(out_row_stride=68, batch=65536)), _no(STRIDE)),
    "pe_stride_out_batch_stride": ("patch_embed", dict(patch=dict(out_batch_stride=16 * 64 + 4)), _no(STRIDE)),
    "pe_stride_weight_plus_8_bytes": ("patch_embed", dict(patch=dict(weight=_plus("weight", 8), batch=65536)), _no(STRIDE)),
    "pe_stride_bias_plus_8_bytes": ("patch_embed", dict(patch=dict(bias=_plus("bias", 8), batch=65536)), _no(STRIDE)),
    "pe_stride_pos_plus_8_bytes": ("patch_embed", dict(patch=dict(pos=_plus("pos", 8), batch=65536)), _no(STRIDE)),
    "pe_stride_pos_pitch_68": ("patch_embed", dict(patch=dict(pos_row_stride=68, batch=65536)), _no(STRIDE)),
    "pe_shape_batch_65536": ("patch_embed", dict(patch=dict(batch=65536)), _no(SHAPE)),
    "pe_served_K16": ("patch_embed", dict(), _ok(PE)),
    "pe_served_K3": ("patch_embed", dict(C=3, p=1), _ok(PE)),
    "pe_served_K4_no_bias_no_pos": ("patch_embed", dict(C=4, p=1, bias=False, pos=False), _ok(PE)),
    "pe_served_K12": ("patch_embed", dict(C=3, p=2), _ok(PE)),
    "pe_served_K8_any": ("patch_embed", dict(C=2, p=2), _ok(PE)),
    "pe_served_weight_64KB": ("patch_embed", dict(C=16, p=2, E=256), _ok(PE)),
    "pe_served_batch_7": ("patch_embed", dict(B=7, C=3, p=1, H=64, W=64, E=8), _ok(PE)),
    "pe_served_batch_8": ("patch_embed", dict(B=8, C=3, p=1, H=64, W=64, E=8), _ok(PE)),
    "pe_served_batch_63": ("patch_embed", dict(B=63, C=3, p=1, H=64, W=64, E=8), _ok(PE)),
    "pe_served_batch_64": ("patch_embed", dict(B=64, C=3, p=1, H=64, W=64, E=8), _ok(PE)),
    # -- zigma_timestep_embed_fwd: bf16, B=3, dim=8
    "te_shape_negative_batch": ("timestep_embed", dict(patch=dict(batch=-1, flags=1)), _no(SHAPE)),
    "te_shape_dim_1": ("timestep_embed", dict(patch=dict(dim=1, flags=1)), _no(SHAPE)),
    "te_unsupported_flag_on_empty": ("timestep_embed", dict(B=0, patch=dict(flags=1, dtype=_lib.F16)), _no(UNSUPPORTED)),
    "te_dtype_f16": ("timestep_embed", dict(patch=dict(dtype=_lib.F16, t=None)), _no(DTYPE)),
    "te_empty": ("timestep_embed", dict(B=0, patch=dict(t=None)), Expect(OK, None)),
    "te_null_t": ("timestep_embed", dict(patch=dict(t=None)), _no(NULL)),
    "te_null_freqs": ("timestep_embed", dict(patch=dict(freqs=None)), _no(NULL)),
    "te_null_out": ("timestep_embed", dict(patch=dict(out=None)), _no(NULL)),
    "te_served": ("timestep_embed", dict(), _ok(TE)),
    "te_served_257_pairs": ("timestep_embed", dict(B=257, dim=2), _ok(TE)),
    # -- zigma_skinny_linear_fwd: bf16, m=2, n=16, k=128, bias
    "sk_shape_negative_m": ("skinny_linear", dict(patch=dict(m=-1, flags=2)), _no(SHAPE)),
    "sk_unsupported_flag_2_on_empty": ("skinny_linear", dict(m=0, patch=dict(flags=2, dtype=_lib.F16)), _no(UNSUPPORTED)),
    "sk_dtype_f16": ("skinny_linear", dict(patch=dict(dtype=_lib.F16, m=65)), _no(DTYPE)),
    "sk_shape_m_65": ("skinny_linear", dict(patch=dict(m=65, x=None)), _no(SHAPE)),
    "sk_shape_n_24": ("skinny_linear", dict(patch=dict(n=24, x=None)), _no(SHAPE)),
    "sk_shape_k_192": ("skinny_linear", dict(patch=dict(k=192, x=None)), _no(SHAPE)),
    "sk_shape_k_1152": ("skinny_linear", dict(patch=dict(k=1152, x=None)), _no(SHAPE)),
    "sk_empty_no_rows": ("skinny_linear", dict(m=0, patch=dict(x=None)), Expect(OK, None)),
    "sk_empty_no_features": ("skinny_linear", dict(patch=dict(n=0, w=None)), Expect(OK, None)),
    "sk_null_k_0": ("skinny_linear", dict(patch=dict(k=0, x_row_stride=4)), _no(NULL)),
    "sk_null_x": ("skinny_linear", dict(patch=dict(x=None, w_row_stride=132)), _no(NULL)),
    "sk_null_w": ("skinny_linear", dict(patch=dict(w=None)), _no(NULL)),
    "sk_null_out": ("skinny_linear", dict(patch=dict(out=None)), _no(NULL)),
    "sk_stride_x_plus_8_bytes": ("skinny_linear", dict(patch=dict(x=_plus("x", 8))), _no(STRIDE)),
    "sk_stride_x_pitch_132": ("skinny_linear", dict(patch=dict(x_row_stride=132)), _no(STRIDE)),
    "sk_stride_w_plus_8_bytes": ("skinny_linear", dict(patch=dict(w=_plus("w", 8))), _no(STRIDE)),
    "sk_stride_w_pitch_132": ("skinny_linear", dict(patch=dict(w_row_stride=132)), _no(STRIDE)),
    "sk_stride_out_plus_4_bytes": ("skinny_linear", dict(patch=dict(out=_plus("out", 4))), _no(STRIDE)),
    "sk_stride_out_pitch_18": ("skinny_linear", dict(patch=dict(out_row_stride=18)), _no(STRIDE)),
    "sk_stride_bias_plus_4_bytes": ("skinny_linear", dict(patch=dict(bias=_plus("bias", 4))), _no(STRIDE)),
    "sk_served_k128_m1": ("skinny_linear", dict(m=1), _ok(SK)),
    "sk_served_k128_m64_silu": ("skinny_linear", dict(m=64, silu=True), _ok(SK)),
    "sk_served_k1024_m1_silu_no_bias": ("skinny_linear", dict(m=1, k=1024, silu=True, bias=False), _ok(SK)),
    "sk_served_k1024_m64": ("skinny_linear", dict(m=64, k=1024), _ok(SK)),
    "sk_served_out_plus_8_bytes_n_4112": ("skinny_linear", dict(m=3, n=4112, out_off=4), _ok(SK)),             # 257 strips: 33 workgroups
    # -- zigma_final_layer_fwd: bf16, rows=5, cols=64, n_out=3, bias
    "fl_shape_negative_rows": ("final_layer", dict(patch=dict(rows=-1, flags=1)), _no(SHAPE)),
    "fl_shape_cols_4": ("final_layer", dict(patch=dict(cols=4, flags=1)), _no(SHAPE)),
    "fl_shape_n_out_0": ("final_layer", dict(patch=dict(n_out=0, flags=1)), _no(SHAPE)),
    "fl_unsupported_flag_on_empty": ("final_layer", dict(rows=0, patch=dict(flags=1, dtype=_lib.F16)), _no(UNSUPPORTED)),
    "fl_dtype_f16": ("final_layer", dict(patch=dict(dtype=_lib.F16, n_out=17)), _no(DTYPE)),
    "fl_shape_cols_68": ("final_layer", dict(patch=dict(cols=68, x=None)), _no(SHAPE)),
    "fl_shape_cols_2056": ("final_layer", dict(patch=dict(cols=2056, x=None)), _no(SHAPE)),
    "fl_shape_n_out_17": ("final_layer", dict(patch=dict(n_out=17, x=None)), _no(SHAPE)),
    "fl_empty": ("final_layer", dict(rows=0, patch=dict(x=None)), Expect(OK, None)),
    "fl_null_x": ("final_layer", dict(patch=dict(x=None, x_row_stride=68)), _no(NULL)),
    "fl_null_weight": ("final_layer", dict(patch=dict(weight=None)), _no(NULL)),
    "fl_null_out": ("final_layer", dict(patch=dict(out=None)), _no(NULL)),
    "fl_stride_x_plus_8_bytes": ("final_layer", dict(patch=dict(x=_plus("x", 8))), _no(STRIDE)),
    "fl_stride_x_pitch_68": ("final_layer", dict(patch=dict(x_row_stride=68)), _no(STRIDE)),
    "fl_stride_weight_plus_8_bytes": ("final_layer", dict(patch=dict(weight=_plus("weight", 8))), _no(STRIDE)),
    **{f"fl_served_cols_{c}_n_out_{n}": ("final_layer", dict(cols=c, n_out=n), _ok(FL))
       for c, n in ((8, 1), (640, 16), (648, 3), (1024, 1), (1032, 16), (2048, 16))},
    "fl_served_no_bias_17_rows": ("final_layer", dict(rows=17, bias=False), _ok(FL)),
    # -- zigma_final_layer_cfg_fwd: bf16 pair of B=2 samples, grid 2 (4 tokens per sample), patch 1, 3 channels (n_out = 3), cols=64, fp32 out
    "cfg_shape_negative_rows": ("final_layer_cfg", dict(patch=dict(rows=-4, flags=1)), _no(SHAPE)),
    "cfg_shape_cols_4": ("final_layer_cfg", dict(patch=dict(cols=4, flags=1)), _no(SHAPE)),
    "cfg_unsupported_flag_on_empty": ("final_layer_cfg", dict(B=0, patch=dict(flags=1, dtype=_lib.F16)), _no(UNSUPPORTED)),
    "cfg_dtype_f16": ("final_layer_cfg", dict(patch=dict(dtype=_lib.F16, n_out=17)), _no(DTYPE)),
    "cfg_dtype_out_f16": ("final_layer_cfg", dict(out_dtype=F16, patch=dict(n_out=17)), _no(DTYPE)),
    "cfg_shape_cols_2056": ("final_layer_cfg", dict(patch=dict(cols=2056, grid_w=0)), _no(SHAPE)),
    "cfg_shape_n_out_17": ("final_layer_cfg", dict(patch=dict(n_out=17, x_cond=None)), _no(SHAPE)),
    "cfg_shape_grid_w_0": ("final_layer_cfg", dict(patch=dict(grid_w=0, x_cond=None)), _no(SHAPE)),
    "cfg_shape_chans_4": ("final_layer_cfg", dict(patch=dict(chans=4, x_cond=None)), _no(SHAPE)),
    "cfg_shape_rows_per_sample_3": ("final_layer_cfg", dict(patch=dict(rows_per_sample=3, x_cond=None)), _no(SHAPE)),
    "cfg_shape_tokens_per_frame_3": ("final_layer_cfg", dict(patch=dict(tokens_per_frame=3, x_cond=None)), _no(SHAPE)),
    "cfg_shape_grid_w_3": ("final_layer_cfg", dict(patch=dict(grid_w=3, x_cond=None)), _no(SHAPE)),
    "cfg_empty": ("final_layer_cfg", dict(B=0, patch=dict(x_cond=None)), Expect(OK, None)),
    "cfg_null_x_uncond": ("final_layer_cfg", dict(patch=dict(x_uncond=None, x_row_stride=68)), _no(NULL)),
    "cfg_null_scale": ("final_layer_cfg", dict(patch=dict(scale=None, x_row_stride=68)), _no(NULL)),
    "cfg_null_out": ("final_layer_cfg", dict(patch=dict(out=None)), _no(NULL)),
    "cfg_stride_x_cond_plus_8_bytes": ("final_layer_cfg", dict(patch=dict(x_cond=_plus("x_cond", 8))), _no(STRIDE)),
    "cfg_stride_x_pitch_68": ("final_layer_cfg", dict(patch=dict(x_row_stride=68)), _no(STRIDE)),
    "cfg_stride_weight_plus_8_bytes": ("final_layer_cfg", dict(patch=dict(weight=_plus("weight", 8))), _no(STRIDE)),
    "cfg_stride_scale_plus_2_bytes": ("final_layer_cfg", dict(patch=dict(scale=_plus("scale", 2))), _no(STRIDE)),
    "cfg_stride_out_plus_2_bytes": ("final_layer_cfg", dict(patch=dict(out=_plus("out", 2))), _no(STRIDE)),
    "cfg_stride_bf16_out_plus_1_byte": ("final_layer_cfg", dict(out_dtype=BF, patch=dict(out=_plus("out", 1))), _no(STRIDE)),
    **{f"cfg_served_cols_{c}_n_out_{n}": ("final_layer_cfg", dict(cols=c, patch_size=p, chans=ch), _ok(CFG))
       for c, n, p, ch in ((8, 1, 1, 1), (640, 16, 2, 4), (648, 3, 1, 3), (1024, 1, 1, 1), (1032, 16, 4, 1), (2048, 16, 2, 4))},
    "cfg_served_bf16_out_two_frames": ("final_layer_cfg", dict(out_dtype=BF, frames=2), _ok(CFG)),
    # -- zigma_cross_attn_fwd: bf16, B=2, L=33, 2 heads of 64, n_ctx=77
    "xa_shape_negative_batch": ("cross_attn", dict(patch=dict(batch=-1, flags=1)), _no(SHAPE)),
    "xa_shape_heads_0": ("cross_attn", dict(patch=dict(heads=0, flags=1)), _no(SHAPE)),
    "xa_shape_n_ctx_0": ("cross_attn", dict(patch=dict(n_ctx=0, scale=0.0)), _no(SHAPE)),
    "xa_unsupported_flag": ("cross_attn", dict(B=0, patch=dict(flags=1)), _no(UNSUPPORTED)),
    "xa_unsupported_scale_0_on_empty": ("cross_attn", dict(B=0, scale=0.0), _no(UNSUPPORTED)),
    "xa_unsupported_scale_inf": ("cross_attn", dict(scale=float("inf"), patch=dict(q=None)), _no(UNSUPPORTED)),
    "xa_unsupported_scale_nan": ("cross_attn", dict(scale=float("nan"), patch=dict(q=None)), _no(UNSUPPORTED)),
    "xa_empty_no_samples": ("cross_attn", dict(B=0, patch=dict(q=None)), Expect(OK, None)),
    "xa_empty_no_tokens": ("cross_attn", dict(L=0, patch=dict(q=None, dtype=_lib.F32)), Expect(OK, None)),
    "xa_null_q": ("cross_attn", dict(patch=dict(q=None, dtype=_lib.F32)), _no(NULL)),
    "xa_null_out": ("cross_attn", dict(patch=dict(out=None, dtype=_lib.F32)), _no(NULL)),
    "xa_dtype_f32": ("cross_attn", dict(patch=dict(dtype=_lib.F32, head_dim=32)), _no(DTYPE)),
    "xa_shape_head_dim_32": ("cross_attn", dict(patch=dict(head_dim=32, q_row_stride=132)), _no(SHAPE)),
    "xa_shape_n_ctx_129": ("cross_attn", dict(patch=dict(n_ctx=129, q_row_stride=132)), _no(SHAPE)),
    "xa_shape_batch_65536": ("cross_attn", dict(patch=dict(batch=65536, q_row_stride=132)), _no(SHAPE)),
    "xa_shape_heads_65536": ("cross_attn", dict(patch=dict(heads=65536, q_row_stride=132)), _no(SHAPE)),
    "xa_stride_q_pitch_132": ("cross_attn", dict(patch=dict(q_row_stride=132)), _no(STRIDE)),
    "xa_stride_k_batch_stride": ("cross_attn", dict(patch=dict(k_batch_stride=77 * 128 + 4)), _no(STRIDE)),
    "xa_stride_v_plus_8_bytes": ("cross_attn", dict(patch=dict(v=_plus("v", 8))), _no(STRIDE)),
    "xa_stride_out_plus_8_bytes": ("cross_attn", dict(patch=dict(out=_plus("out", 8))), _no(STRIDE)),
    "xa_stride_out_pitch_132": ("cross_attn", dict(patch=dict(o_row_stride=132)), _no(STRIDE)),
    **{f"xa_served_n_ctx_{n}": ("cross_attn", dict(n_ctx=n), _ok(XA)) for n in (1, 64, 65, 80, 81, 112, 113, 128)},
    "xa_served_f16_511_tokens": ("cross_attn", dict(dtype=F16, L=511, B=1), _ok(XA)),
    "xa_served_512_tokens_kv_halves": ("cross_attn", dict(L=512, B=1, kv="halves"), _ok(XA)),
    # -- zigma_cross_attn_bwd: the same operands, bf16 only
    "xb_shape_negative_seqlen": ("cross_attn_bwd", dict(patch=dict(seqlen=-1, flags=1)), _no(SHAPE)),
    "xb_unsupported_flag": ("cross_attn_bwd", dict(B=0, patch=dict(flags=1)), _no(UNSUPPORTED)),
    "xb_unsupported_scale_negative": ("cross_attn_bwd", dict(scale=-0.125, patch=dict(q=None)), _no(UNSUPPORTED)),
    "xb_empty_no_tokens": ("cross_attn_bwd", dict(L=0, patch=dict(q=None)), Expect(OK, None)),
    "xb_null_dout": ("cross_attn_bwd", dict(patch=dict(dout=None, dtype=_lib.F16)), _no(NULL)),
    "xb_null_dv_part": ("cross_attn_bwd", dict(patch=dict(dv_part=None, dtype=_lib.F16)), _no(NULL)),
    "xb_dtype_f16": ("cross_attn_bwd", dict(dtype=F16, patch=dict(head_dim=32)), _no(DTYPE)),
    "xb_shape_head_dim_32": ("cross_attn_bwd", dict(patch=dict(head_dim=32, chunks=2)), _no(SHAPE)),
    "xb_shape_n_ctx_129": ("cross_attn_bwd", dict(patch=dict(n_ctx=129, dq_row_stride=132)), _no(SHAPE)),
    "xb_shape_chunks_2_for_33_tokens": ("cross_attn_bwd", dict(patch=dict(chunks=2, dq_row_stride=132)), _no(SHAPE)),
    "xb_shape_chunks_1_for_513_tokens": ("cross_attn_bwd", dict(L=513, B=1, patch=dict(chunks=1, dq_row_stride=132)), _no(SHAPE)),
    "xb_stride_do_pitch_132": ("cross_attn_bwd", dict(patch=dict(do_row_stride=132)), _no(STRIDE)),
    "xb_stride_dq_plus_8_bytes": ("cross_attn_bwd", dict(patch=dict(dq=_plus("dq", 8))), _no(STRIDE)),
    "xb_stride_dk_part_plus_8_bytes": ("cross_attn_bwd", dict(patch=dict(dk_part=_plus("dk_part", 8))), _no(STRIDE)),
    "xb_stride_dv_part_plus_8_bytes": ("cross_attn_bwd", dict(patch=dict(dv_part=_plus("dv_part", 8))), _no(STRIDE)),
    **{f"xb_served_n_ctx_{n}": ("cross_attn_bwd", dict(n_ctx=n), _ok(XB)) for n in (1, 80, 81, 128)},
    "xb_served_511_tokens": ("cross_attn_bwd", dict(L=511, B=1), _ok(XB)),
    "xb_served_513_tokens_kv_halves": ("cross_attn_bwd", dict(L=513, B=1, kv="halves"), _ok(XB)),
    # -- zigma_scale_reduce_bwd: bf16, B=2, L=64, cols=128, out and both sums
    "gb_shape_negative_rows": ("scale_reduce_bwd", dict(patch=dict(rows=-64, flags=1)), _no(SHAPE)),
    "gb_shape_cols_0": ("scale_reduce_bwd", dict(patch=dict(cols=0, flags=1)), _no(SHAPE)),
    "gb_shape_rows_per_batch_0": ("scale_reduce_bwd", dict(patch=dict(rows_per_batch=0, flags=1)), _no(SHAPE)),
    "gb_unsupported_flag_on_empty": ("scale_reduce_bwd", dict(B=0, patch=dict(flags=1)), _no(UNSUPPORTED)),
    "gb_empty": ("scale_reduce_bwd", dict(B=0, patch=dict(dy=None, dtype=_lib.F16)), Expect(OK, None)),
    "gb_null_dy": ("scale_reduce_bwd", dict(patch=dict(dy=None, dtype=_lib.F16)), _no(NULL)),
    "gb_null_r1": ("scale_reduce_bwd", dict(patch=dict(r1=None, dtype=_lib.F16)), _no(NULL)),
    "gb_dtype_f16": ("scale_reduce_bwd", dict(dtype=F16, patch=dict(cols=192)), _no(DTYPE)),
    "gb_shape_cols_192": ("scale_reduce_bwd", dict(patch=dict(cols=192, dy_row_stride=132)), _no(SHAPE)),
    "gb_shape_cols_8320": ("scale_reduce_bwd", dict(patch=dict(cols=8320, dy_row_stride=132)), _no(SHAPE)),
    "gb_shape_rows_per_batch_100": ("scale_reduce_bwd", dict(patch=dict(rows_per_batch=100, dy_row_stride=132)), _no(SHAPE)),
    "gb_shape_rows_not_whole_samples": ("scale_reduce_bwd", dict(patch=dict(rows=64 * 3, rows_per_batch=128, dy_row_stride=132)), _no(SHAPE)),
    "gb_stride_dy_pitch_132": ("scale_reduce_bwd", dict(patch=dict(dy_row_stride=132)), _no(STRIDE)),
    "gb_stride_a_plus_8_bytes": ("scale_reduce_bwd", dict(patch=dict(a=_plus("a", 8))), _no(STRIDE)),
    "gb_stride_out_plus_8_bytes": ("scale_reduce_bwd", dict(patch=dict(out=_plus("out", 8))), _no(STRIDE)),
    "gb_stride_s_pitch_132": ("scale_reduce_bwd", dict(patch=dict(s_batch_stride=132)), _no(STRIDE)),
    "gb_served_cols_128_both_sums": ("scale_reduce_bwd", dict(), _ok(GB)),
    "gb_served_cols_128_one_sum_no_out": ("scale_reduce_bwd", dict(want_out=False, want_sum=False), _ok(GB)),
    "gb_served_cols_8192_both_sums": ("scale_reduce_bwd", dict(B=1, cols=8192), _ok(GB)),
    "gb_served_cols_8192_one_sum_s_a_third_of_its_rows": ("scale_reduce_bwd", dict(B=1, cols=8192, want_sum=False, s_wide=True), _ok(GB)),
    # -- zigma_linear_wgrad: bf16, m=64, n=16, k=64, slabs 0
    "wg_null_dy": ("linear_wgrad", dict(patch=dict(dy=None, dtype=_lib.F32)), _no(NULL)),
    "wg_null_out": ("linear_wgrad", dict(patch=dict(out=None, dtype=_lib.F32)), _no(NULL)),
    "wg_dtype_f32": ("linear_wgrad", dict(patch=dict(dtype=_lib.F32, m=0)), _no(DTYPE)),
    "wg_dtype_out_f16_of_bf16": ("linear_wgrad", dict(patch=dict(out_dtype=_lib.F16, m=0)), _no(DTYPE)),
    "wg_shape_m_0": ("linear_wgrad", dict(patch=dict(m=0, flags=1)), _no(SHAPE)),
    "wg_shape_n_12": ("linear_wgrad", dict(patch=dict(n=12, flags=1)), _no(SHAPE)),
    "wg_shape_k_8200": ("linear_wgrad", dict(patch=dict(k=8200, flags=1)), _no(SHAPE)),
    "wg_shape_slabs_4097": ("linear_wgrad", dict(patch=dict(slabs=4097, flags=1)), _no(SHAPE)),
    "wg_unsupported_flag": ("linear_wgrad", dict(patch=dict(flags=1, slabs=2)), _no(UNSUPPORTED)),
    "wg_null_workspace_forced_slabs": ("linear_wgrad", dict(patch=dict(slabs=2, workspace=None)), _no(NULL)),
    "wg_shape_workspace_too_small": ("linear_wgrad", dict(slabs=2, patch=dict(workspace_bytes=2 * 16 * 64 * 4 - 4, dy_row_stride=20)), _no(SHAPE)),
    "wg_stride_dy_pitch_below_n": ("linear_wgrad", dict(patch=dict(dy_row_stride=8)), _no(STRIDE)),
    "wg_stride_dy_pitch_20": ("linear_wgrad", dict(patch=dict(dy_row_stride=20)), _no(STRIDE)),
    "wg_stride_x_plus_8_bytes": ("linear_wgrad", dict(patch=dict(x=_plus("x", 8))), _no(STRIDE)),
    "wg_stride_out_pitch_68": ("linear_wgrad", dict(patch=dict(out_row_stride=68)), _no(STRIDE)),
    "wg_stride_workspace_plus_8_bytes": ("linear_wgrad", dict(slabs=2, patch=dict(workspace=_plus("workspace", 8))), _no(STRIDE)),
    "wg_served_k64_m511": ("linear_wgrad", dict(m=511), _ok("wgrad_128x64")),
    "wg_served_k72_m512": ("linear_wgrad", dict(m=512, k=72), _ok("wgrad_128x128")),
    "wg_served_k64_m1024_two_slabs": ("linear_wgrad", dict(m=1024), _ok("wgrad_128x64_splitk")),
    "wg_served_k72_m1024_f16": ("linear_wgrad", dict(m=1024, k=72, dtype=F16), _ok("wgrad_128x128_splitk")),
    "wg_served_forced_3_slabs_fp32_out": ("linear_wgrad", dict(m=100, slabs=3, out_dtype=F32), _ok("wgrad_128x64_splitk")),
    "wg_served_fp32_out_pitch_68_x_a_column_view": ("linear_wgrad", dict(k=72, out_dtype=F32, out_pitch=76, x_pitch=80), _ok("wgrad_128x128")),
}
ENTRY = {e: "zigma_" + e + ("" if e.endswith(("bwd", "wgrad")) else "_fwd") for e in {c[0] for c in CASES.values()}}
# the fields of each block that hold the addresses of tensors the wrapper allocates itself: what a block asked about on placeholders may differ in
ALLOCATED = {"patch_embed": ("out",), "timestep_embed": ("out",), "skinny_linear": ("out",), "final_layer": ("out",), "final_layer_cfg": ("out",),
             "cross_attn": ("out",), "cross_attn_bwd": ("dq", "dk_part", "dv_part"), "scale_reduce_bwd": ("out", "r1", "r2"),
             "linear_wgrad": ("out", "workspace")}


def _rand(g, device, dtype, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(device=device, dtype=dtype)


def _pitched(g, device, dtype, rows, cols, pitch=0, off=0):
    """(rows, cols) random rows `pitch` elements apart, `off` elements into their allocation"""
    wide = _rand(g, device, dtype, rows * (pitch or cols) + off)
    return wide[off:].view(rows, pitch or cols)[:, :cols]


# Every builder below returns (args, kwargs, outs): the operands of the product's predicate / wrapper / block builder in their order, the keywords all
# three take, and the outputs the block points to as keywords of the block builder.
def _patch_embed(c, dev, g):
    c = {**dict(B=2, C=4, H=8, W=8, p=2, E=64, bias=True, pos=True), **c}
    B, C, H, W, p, E = (c[k] for k in "B C H W p E".split())
    L = (H // p) * (W // p)
    args = (_rand(g, dev, BF, B, C, H, W), _rand(g, dev, BF, E, C, p, p, scale=0.25), _rand(g, dev, BF, E) if c["bias"] else None,
            _rand(g, dev, BF, 1, L, E) if c["pos"] else None)
    return args, {}, dict(out=torch.empty(B, L, E, device=dev, dtype=BF))


def _timestep_embed(c, dev, g):
    c = {**dict(B=3, dim=8), **c}
    args = (_rand(g, dev, BF, c["B"]), _rand(g, dev, BF, c["dim"] // 2), c["dim"])
    return args, {}, dict(out=torch.empty(c["B"], c["dim"], device=dev, dtype=BF))


def _skinny_linear(c, dev, g):
    c = {**dict(m=2, n=16, k=128, bias=True, silu=False, out_off=0), **c}
    m, n, k = c["m"], c["n"], c["k"]
    args = (_rand(g, dev, BF, m, k), _rand(g, dev, BF, n, k, scale=k ** -0.5), _rand(g, dev, BF, n) if c["bias"] else None)
    return args, dict(silu=c["silu"]), dict(out=_pitched(g, dev, BF, m, n, off=c["out_off"]))


def _final_layer(c, dev, g):
    c = {**dict(rows=5, cols=64, n_out=3, bias=True), **c}
    rows, cols, n = c["rows"], c["cols"], c["n_out"]
    args = (_rand(g, dev, BF, rows, cols), _rand(g, dev, BF, n, cols, scale=cols ** -0.5), _rand(g, dev, BF, n) if c["bias"] else None, 1e-6)
    return args, {}, dict(out=torch.empty(rows, n, device=dev, dtype=BF))


def _final_layer_cfg(c, dev, g):
    c = {**dict(B=2, cols=64, grid=2, patch_size=1, chans=3, frames=0, out_dtype=F32), **c}
    B, cols, grid, p, ch, T = c["B"], c["cols"], c["grid"], c["patch_size"], c["chans"], c["frames"]
    L, n = max(T, 1) * grid * grid, p * p * ch
    args = (_rand(g, dev, BF, 2 * B, L, cols), _rand(g, dev, BF, n, cols, scale=cols ** -0.5), _rand(g, dev, BF, n), 1e-6,
            torch.full((B,), 4.0, device=dev, dtype=F32))
    out = torch.empty((B,) + ((T,) if T else ()) + (ch, grid * p, grid * p), device=dev, dtype=c["out_dtype"])
    return args, dict(patch=p, chans=ch, grid=grid, frames=T, out_dtype=c["out_dtype"]), dict(out=out)


def _xattn_operands(c, dev, g):
    c = {**dict(dtype=BF, B=2, L=33, H=2, n_ctx=77, scale=None, kv="own"), **c}
    dt, B, L, n, C = c["dtype"], c["B"], c["L"], c["n_ctx"], c["H"] * 64
    q = _rand(g, dev, dt, B, L, C)
    if c["kv"] == "halves":            # the column halves of one batched projection, as the block produces them
        kv = _rand(g, dev, dt, B, n, 2 * C)
        k, v = kv[..., :C], kv[..., C:]
    else:
        k, v = _rand(g, dev, dt, B, n, C), _rand(g, dev, dt, B, n, C)
    return c, q, k, v


def _cross_attn(c, dev, g):
    c, q, k, v = _xattn_operands(c, dev, g)
    return (q, k, v, c["H"], c["scale"]), {}, dict(out=torch.empty_like(q))


def _cross_attn_bwd(c, dev, g):
    c, q, k, v = _xattn_operands(c, dev, g)
    chunks = max(_lib.lib().zigma_cross_attn_bwd_chunks(q.shape[1]), 1)
    outs = dict(dq=torch.empty_like(q), part=torch.empty(2, chunks, *k.shape, device=dev, dtype=F32))
    return (q, k, v, _rand(g, dev, c["dtype"], *q.shape), c["H"], c["scale"]), {}, outs


def _scale_reduce_bwd(c, dev, g):
    c = {**dict(dtype=BF, B=2, L=64, cols=128, want_out=True, want_sum=True, s_wide=False), **c}
    dt, B, L, E = c["dtype"], c["B"], c["L"], c["cols"]
    s = _rand(g, dev, dt, B, 3 * E)[:, E:2 * E] if c["s_wide"] else _rand(g, dev, dt, B, E)
    sums = lambda: torch.empty(B, L // 64, E, device=dev, dtype=F32)
    outs = dict(out=torch.empty(B, L, E, device=dev, dtype=dt) if c["want_out"] else None, r1=sums(), r2=sums() if c["want_sum"] else None)
    return (_rand(g, dev, dt, B, L, E), _rand(g, dev, dt, B, L, E), s, 1.0), dict(want_out=c["want_out"], want_sum=c["want_sum"]), outs


def _linear_wgrad(c, dev, g):
    c = {**dict(dtype=BF, m=64, n=16, k=64, slabs=0, out_dtype=None, out_pitch=0, x_pitch=0), **c}
    dt, m, n, k = c["dtype"], c["m"], c["n"], c["k"]
    args = (_rand(g, dev, dt, m, n), _pitched(g, dev, dt, m, k, c["x_pitch"]), c["out_dtype"], c["slabs"])
    P = _lib.LinearWgradParams()
    P.m, P.n, P.k, P.slabs, P.dtype, P.out_dtype = m, n, k, c["slabs"], _lib._DT[dt], _lib._DT[c["out_dtype"] or dt]
    ws = torch.empty(max(int(_lib.lib().zigma_linear_wgrad_workspace_bytes(ctypes.byref(P))), 16), device=dev, dtype=torch.uint8)
    return args, {}, dict(out=_pitched(g, dev, c["out_dtype"] or dt, n, k, c["out_pitch"]), workspace=ws)


_BUILD = {"patch_embed": _patch_embed, "timestep_embed": _timestep_embed, "skinny_linear": _skinny_linear, "final_layer": _final_layer,
          "final_layer_cfg": _final_layer_cfg, "cross_attn": _cross_attn, "cross_attn_bwd": _cross_attn_bwd, "scale_reduce_bwd": _scale_reduce_bwd,
          "linear_wgrad": _linear_wgrad}


def product(entry):
    """(block builder, predicate or None, wrapper) of the entry point.  The predicate is named where it takes the wrapper's operands and returns the block
    it accepted (the wrapper's `block=`)."""
    from zigma_amd import attention, embed, layernorm, wgrad
    return {"patch_embed": (embed.patch_embed_block, embed.patch_embed_eligible, embed.patch_embed),
            "timestep_embed": (embed.timestep_embed_block, None, embed.timestep_embed),
            "skinny_linear": (embed.skinny_linear_block, embed.skinny_linear_eligible, embed.skinny_linear),
            "final_layer": (embed.final_layer_block, None, embed.final_layer),
            "final_layer_cfg": (embed.final_layer_cfg_block, None, embed.final_layer_guided),
            "cross_attn": (attention.cross_attn_block, attention.cross_attn_eligible, attention.cross_attn),
            "cross_attn_bwd": (attention.cross_attn_bwd_block, None, attention.cross_attn_bwd),
            "scale_reduce_bwd": (layernorm.glue_bwd_block, None, layernorm.scale_reduce_bwd),
            "linear_wgrad": (wgrad.wgrad_block, None, wgrad.wgrad_own)}[entry]


def operands(name, device):
    entry, case, _ = CASES[name]
    case = {k: v for k, v in case.items() if k != "patch"}
    return _BUILD[entry](case, device, torch.Generator().manual_seed(len(name)))


def block(name, device):
    """Build the case's operands and outputs on `device`, let the product's block builder fill the parameter block on them, fill every output with NaN and
    apply the case's patch -> (entry point, block, outputs)"""
    entry, case, _ = CASES[name]
    args, kwargs, outs = operands(name, device)
    P = product(entry)[0](*args, **kwargs, **outs)
    for t in outs.values():
        if t is not None and t.dtype != torch.uint8:
            t.fill_(float("nan"))
    for k, v in case.get("patch", {}).items():
        setattr(P, k, v(P) if callable(v) else v)
    return ENTRY[entry], P, outs
