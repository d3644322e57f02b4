"""Case table of plan_norm_linear() (zigma_amd/csrc/norm_linear_plan.h): one call per leaf of the plan — every served instantiation and every refusal —
with the status and the kernel string it must give.  test_norm_linear_cpu.py checks the table against the plan compiled with g++, test_gpu_norm_linear.py
checks the refusals against the library on the GPU (status returned, nothing launched).

A case is (name, overrides, status, kernel): `overrides` are fields set on top of BASE, a served call of 128 rows.  Pointer fields take NULL or OFF(bytes):
the test's own buffer moved by that many bytes."""
OK, ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_STRIDE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -6
F32, F16, BF16 = 0, 1, 2
NULL = "null"


class OFF:
    def __init__(self, nbytes):
        self.nbytes = nbytes


POINTERS = ("x", "w", "shift", "scale", "out")
BASE = dict(m=128, n=512, k=640, dtype=BF16, flags=0, rows_per_batch=128, eps=1e-6, x_row_stride=640, w_row_stride=640, out_row_stride=512,
            mod_batch_stride=6 * 640)

CASES = [
    # served: the three instantiated row lengths, both 16-bit types
    ("k640_bf16", {}, OK, "norm_linear_k640"),
    ("k640_f16", dict(dtype=F16), OK, "norm_linear_k640"),
    ("k512_bf16", dict(k=512, x_row_stride=512, w_row_stride=512), OK, "norm_linear_k512"),
    ("k768_f16", dict(k=768, x_row_stride=768, w_row_stride=768, dtype=F16), OK, "norm_linear_k768"),
    ("straddling_samples", dict(m=384, rows_per_batch=96), OK, "norm_linear_k640"),
    ("wide_pitches", dict(x_row_stride=1280, w_row_stride=648, out_row_stride=1024, mod_batch_stride=640), OK, "norm_linear_k640"),
    ("broadcast_mod", dict(mod_batch_stride=0), OK, "norm_linear_k640"),
    # empty call: OK without a launch, pointers not looked at
    ("empty", dict(m=0, x=NULL, out=NULL), OK, None),
    # refusals, in the order the plan takes them
    ("m_negative", dict(m=-128), ERR_SHAPE, None),
    ("n_zero", dict(n=0), ERR_SHAPE, None),
    ("k_zero", dict(k=0), ERR_SHAPE, None),
    ("rows_per_batch_zero", dict(rows_per_batch=0), ERR_SHAPE, None),
    ("flags", dict(flags=1), ERR_UNSUPPORTED, None),
    ("flags_high_bit", dict(flags=0x10), ERR_UNSUPPORTED, None),
    ("null_x", dict(x=NULL), ERR_NULL, None),
    ("null_w", dict(w=NULL), ERR_NULL, None),
    ("null_shift", dict(shift=NULL), ERR_NULL, None),
    ("null_scale", dict(scale=NULL), ERR_NULL, None),
    ("null_out", dict(out=NULL), ERR_NULL, None),
    ("fp32", dict(dtype=F32), ERR_DTYPE, None),
    ("dtype_unknown", dict(dtype=7), ERR_DTYPE, None),
    ("n_256", dict(n=256, out_row_stride=256), ERR_SHAPE, None),
    ("n_640", dict(n=640, out_row_stride=640), ERR_SHAPE, None),
    ("k_576", dict(k=576, x_row_stride=576, w_row_stride=576), ERR_SHAPE, None),
    ("k_1024", dict(k=1024, x_row_stride=1024, w_row_stride=1024), ERR_SHAPE, None),
    ("m_not_whole_tiles", dict(m=192, rows_per_batch=192), ERR_SHAPE, None),
    ("m_not_whole_samples", dict(m=384, rows_per_batch=256), ERR_SHAPE, None),
    ("x_pitch_below_k", dict(x_row_stride=632), ERR_SHAPE, None),
    ("w_pitch_below_k", dict(w_row_stride=512), ERR_SHAPE, None),
    ("out_pitch_below_n", dict(out_row_stride=504), ERR_SHAPE, None),
    ("mod_pitch_negative", dict(mod_batch_stride=-640), ERR_SHAPE, None),
    ("x_pitch_too_wide", dict(x_row_stride=1 << 28), ERR_SHAPE, None),
    ("w_pitch_too_wide", dict(w_row_stride=1 << 28), ERR_SHAPE, None),
    ("x_pitch_odd", dict(x_row_stride=644), ERR_STRIDE, None),
    ("w_pitch_odd", dict(w_row_stride=644), ERR_STRIDE, None),
    ("out_pitch_odd", dict(out_row_stride=516), ERR_STRIDE, None),
    ("mod_pitch_odd", dict(mod_batch_stride=3844), ERR_STRIDE, None),
    ("x_misaligned", dict(x=OFF(8)), ERR_STRIDE, None),
    ("w_misaligned", dict(w=OFF(2)), ERR_STRIDE, None),
    ("shift_misaligned", dict(shift=OFF(4)), ERR_STRIDE, None),
    ("scale_misaligned", dict(scale=OFF(8)), ERR_STRIDE, None),
    ("out_misaligned", dict(out=OFF(8)), ERR_STRIDE, None),
]


def make_params(params_type, overrides, pointers):
    """a parameter block for BASE + overrides; pointers: {field: address of the caller's buffer}"""
    P = params_type()
    fields = dict(BASE, **{k: v for k, v in overrides.items() if k not in POINTERS})
    for k, v in fields.items():
        setattr(P, k, v)
    for k in POINTERS:
        v = overrides.get(k)
        setattr(P, k, None if v == NULL else pointers[k] + (v.nbytes if isinstance(v, OFF) else 0))
    return P
