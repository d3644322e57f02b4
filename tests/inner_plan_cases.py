"""plan_inner calls on descriptors of the shipped shapes (BASELINE.json / bench.py) and the InnerPlan each must give.

The expected plans were RECORDED by running plan_inner of the parent commit d946088 — the last one whose predicates restated the C limits by hand —
on these same descriptors (`PYTHONPATH=<checkout> python tests/inner_plan_cases.py` prints the table of that checkout's plan_inner); they are not taken from
the code under test.  test_inner_plan_cases.py runs the table through the current plan_inner, whose predicates ask the built library.
"""
import math

import torch

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MODELS = {"readme": (1280, 40, 16), "e768": (1536, 48, 16)}      # d_inner, dt_rank, d_state; x_proj has dt_rank + 2 * d_state rows


class T:
    """a device tensor as plan_inner reads it (shape, strides, dtype, address); nothing is allocated"""
    requires_grad = False

    def __init__(self, dtype, shape, strides=None, ptr=1 << 30, is_cuda=True):
        self.dtype, self.shape, self._ptr, self.is_cuda = dtype, tuple(shape), ptr, is_cuda
        self._strides = tuple(strides) if strides else tuple(math.prod(shape[i + 1:]) for i in range(len(shape)))

    def stride(self, i):
        return self._strides[i]

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return math.prod(self.shape)

    def is_contiguous(self):
        return self._strides == tuple(math.prod(self.shape[i + 1:]) for i in range(len(self.shape)))


def _case(model="readme", B=1, L=1024, dtype=BF, video=0, cuda=True, w_pitch=0, w_off=0, add_to=False, no_bias=False, B_proj_bias=False, **kw):
    return dict(model=model, B=B, L=L, dtype=dtype, video=video, cuda=cuda, w_pitch=w_pitch, w_off=w_off, add_to=add_to, no_bias=no_bias,
                B_proj_bias=B_proj_bias, kw=kw)


CASES = {}
for _m in MODELS:
    for _b in (1, 2, 4, 8, 16, 32, 64):
        CASES[f"{_m}_L1024_B{_b}"] = _case(_m, _b)
for _b in (1, 4, 64):
    CASES[f"readme_L16384_B{_b}"] = _case(B=_b, L=16384)
CASES.update({
    # the video temporal layers: batch = pixels, sequence = (sample, frame) on the strided view of the (b * t, k, 2 d_inner) projection output
    "video_temporal_k256_bt32": _case(B=256, L=32, video=16), "video_temporal_k1024_bt128_e768": _case("e768", B=1024, L=128, video=16),
    "v2_add_to_B64": _case(B=64, add_to=True), "v2_add_to_B4_split": _case(B=4, add_to=True), "v2_add_to_e768_B16": _case("e768", B=16, add_to=True),
    "z_preactivated_B64": _case(B=64, z_preactivated=True), "z_preactivated_B4_split": _case(B=4, z_preactivated=True),
    "no_delta_bias_B64": _case(B=64, no_bias=True), "no_delta_bias_B4_split": _case(B=4, no_bias=True),
    "B_proj_bias_B64": _case(B=64, B_proj_bias=True), "B_proj_bias_B4_split": _case(B=4, B_proj_bias=True),
    "no_softplus_B64": _case(B=64, delta_softplus=False), "no_softplus_B4_split": _case(B=4, delta_softplus=False),
    "train_B64": _case(B=64, train=True), "train_B4": _case(B=4, train=True), "train_e768_B8": _case("e768", B=8, train=True),
    "fp16_B64": _case(B=64, dtype=F16), "fp16_B4_split": _case(B=4, dtype=F16), "fp16_L16384_B1": _case(B=1, L=16384, dtype=F16),
    "fp32_B64": _case(B=64, dtype=F32), "fp32_B4_split": _case(B=4, dtype=F32),
    "cpu_B64": _case(B=64, cuda=False), "cpu_B4": _case(B=4, cuda=False),
    "x_proj_w_pitch_k_plus_4_B64": _case(B=64, w_pitch=4), "x_proj_w_pitch_k_plus_4_B4": _case(B=4, w_pitch=4),
    "x_proj_w_2_byte_offset_B64": _case(B=64, w_off=1), "x_proj_w_2_byte_offset_B4": _case(B=4, w_off=1),
})


def call(plan_inner, c):
    """plan_inner on the case's descriptors: xz (B, L, 2 d_inner) as its two halves, the parameters of one Mamba layer"""
    Di, R, N = MODELS[c["model"]]
    B, L, dt, cuda = c["B"], c["L"], c["dtype"], c["cuda"]
    es = 4 if dt == F32 else 2
    t = lambda dtype, shape, strides=None, ptr=1 << 30: T(dtype, shape, strides, ptr, cuda)
    xz_strides = (2 * Di, B * 2 * Di, 1) if c["video"] else (L * 2 * Di, 2 * Di, 1)
    x_half, z_half = t(dt, (B, L, Di), xz_strides, 1 << 30), t(dt, (B, L, Di), xz_strides, (1 << 30) + Di * es)
    conv_w, conv_b = t(dt, (Di, 4), ptr=1 << 34), t(dt, (Di,), ptr=1 << 35)
    x_proj_w = t(dt, (R + 2 * N, Di), (Di + c["w_pitch"], 1), (1 << 36) + c["w_off"] * es)
    dt_proj_w, A = t(dt, (Di, R), ptr=1 << 37), t(F32, (Di, N), ptr=1 << 38)
    delta_bias = None if c["no_bias"] else t(F32, (Di,), ptr=1 << 39)
    kw = dict(c["kw"], reset_period=c["video"], perm=t(torch.int32, (L,), ptr=1 << 41))
    if c["add_to"]:
        kw["add_to"] = t(dt, (B, L, Di), ptr=1 << 42)
    if c["B_proj_bias"]:
        kw["B_proj_bias"] = t(F32, (N,), ptr=1 << 43)
    return plan_inner(x_half, z_half, conv_w, conv_b, x_proj_w, dt_proj_w, A, delta_bias, **kw)


# case: (front, dt, chunk_len, accumulate), recorded on the parent commit
EXPECTED = {
    'readme_L1024_B1': ('conv+x_proj', 'in_split', 32, False),
    'readme_L1024_B2': ('conv+x_proj', 'in_split', 64, False),
    'readme_L1024_B4': ('conv+x_proj', 'in_split', 112, False),
    'readme_L1024_B8': ('conv+x_proj', 'in_split', 208, False),
    'readme_L1024_B16': ('conv_x_proj', 'in_scan', 0, False),
    'readme_L1024_B32': ('conv_x_proj', 'in_scan', 0, False),
    'readme_L1024_B64': ('conv_x_proj', 'in_scan', 0, False),
    'e768_L1024_B1': ('conv+x_proj', 'in_split', 32, False),
    'e768_L1024_B2': ('conv+x_proj', 'in_split', 64, False),
    'e768_L1024_B4': ('conv+x_proj', 'in_split', 128, False),
    'e768_L1024_B8': ('conv+x_proj', 'in_split', 256, False),
    'e768_L1024_B16': ('conv_x_proj', 'in_scan', 0, False),
    'e768_L1024_B32': ('conv_x_proj', 'in_scan', 0, False),
    'e768_L1024_B64': ('conv_x_proj', 'in_scan', 0, False),
    'readme_L16384_B1': ('conv_x_proj', 'in_split', 256, False),
    'readme_L16384_B4': ('conv_x_proj', 'in_split', 1024, False),
    'readme_L16384_B64': ('conv_x_proj', 'in_scan', 0, False),
    'video_temporal_k256_bt32': ('conv+x_proj', 'in_scan', 0, False),
    'video_temporal_k1024_bt128_e768': ('conv+x_proj', 'in_scan', 0, False),
    'v2_add_to_B64': ('conv_x_proj', 'in_scan', 0, True),
    'v2_add_to_B4_split': ('conv+x_proj', 'in_split', 112, False),
    'v2_add_to_e768_B16': ('conv_x_proj', 'in_scan', 0, True),
    'z_preactivated_B64': ('conv_x_proj', 'in_scan', 0, False),
    'z_preactivated_B4_split': ('conv+x_proj', 'kernel', 112, False),
    'no_delta_bias_B64': ('conv_x_proj', 'in_scan', 0, False),
    'no_delta_bias_B4_split': ('conv+x_proj', 'kernel', 112, False),
    'B_proj_bias_B64': ('conv_x_proj', 'kernel', 0, False),
    'B_proj_bias_B4_split': ('conv+x_proj', 'kernel', 112, False),
    'no_softplus_B64': ('conv_x_proj', 'linear', 0, False),
    'no_softplus_B4_split': ('conv+x_proj', 'linear', 112, False),
    'train_B64': ('conv_x_proj', 'linear', 0, False),
    'train_B4': ('conv+linear', 'linear', 0, False),
    'train_e768_B8': ('conv+linear', 'linear', 0, False),
    'fp16_B64': ('conv_x_proj', 'in_scan', 0, False),
    'fp16_B4_split': ('conv+x_proj', 'in_split', 112, False),
    'fp16_L16384_B1': ('conv_x_proj', 'in_split', 256, False),
    'fp32_B64': ('conv+linear', 'linear', 0, False),
    'fp32_B4_split': ('conv+linear', 'linear', 112, False),
    'cpu_B64': ('conv+linear', 'linear', 0, False),
    'cpu_B4': ('conv+linear', 'linear', 112, False),
    'x_proj_w_pitch_k_plus_4_B64': ('conv+linear', 'in_scan', 0, False),
    'x_proj_w_pitch_k_plus_4_B4': ('conv+linear', 'in_split', 112, False),
    'x_proj_w_2_byte_offset_B64': ('conv+linear', 'in_scan', 0, False),
    'x_proj_w_2_byte_offset_B4': ('conv+linear', 'in_split', 112, False),
}


if __name__ == "__main__":
    from zigma_amd.selective_scan_interface import plan_inner
    print("EXPECTED = {")
    for name, case in CASES.items():
        print(f"    {name!r}: {tuple(call(plan_inner, case))!r},")
    print("}")
