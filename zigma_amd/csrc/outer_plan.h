// The plans of the operators around the blocks: zigma_patch_embed_fwd, zigma_timestep_embed_fwd, zigma_final_layer_fwd, zigma_final_layer_cfg_fwd
// (csrc/embed.hip) and zigma_skinny_linear_fwd (csrc/skinny_linear.hip) — a call's refusal, or the kernel instantiation and launch geometry that serve
// it, and the constants the limits are made of.  Plain C++ without HIP, so the CPU tests compile it on its own; a launcher only maps a plan to a
// template instantiation.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kFlMaxPass = 16;      // final layer: E <= 16 lanes * 8 * 16
constexpr int kSkWaves = 8;         // skinny_linear_kernel: waves per workgroup

struct OuterPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call)
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned gx = 0, gy = 1, block = 0;
    int64_t lds = 0;                // dynamic LDS bytes
    int inst = 0;                   // patch_embed_kernel<KT> (0: any K) | final_layer(_cfg)_kernel<NP> | skinny_linear_kernel<silu, KS = k / 32>
    int silu = 0;
};

inline bool outer_al(const void *q, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }

inline OuterPlan plan_patch_embed(const zigma_patch_embed_params_t &p) {
    OuterPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch < 0 || p.in_chans < 1 || p.patch < 1 || p.embed_dim < 8 || p.height < 1 || p.width < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.dtype != ZIGMA_BF16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.embed_dim % 8 != 0 || p.height % p.patch != 0 || p.width % p.patch != 0) return refuse(ZIGMA_ERR_SHAPE);
    const int64_t K = static_cast<int64_t>(p.in_chans) * p.patch * p.patch, lds = K * p.embed_dim * 4;
    if (lds > 65536) return refuse(ZIGMA_ERR_SHAPE);     // the fp32 [K][E] weight in LDS
    if (p.batch == 0) return s;
    if (!p.x || !p.weight || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!outer_al(p.out, 16) || p.out_row_stride % 8 != 0 || p.out_batch_stride % 8 != 0) return refuse(ZIGMA_ERR_STRIDE);
    if (!outer_al(p.weight, 16)) return refuse(ZIGMA_ERR_STRIDE);
    if (p.bias && !outer_al(p.bias, 16)) return refuse(ZIGMA_ERR_STRIDE);
    if (p.pos && (!outer_al(p.pos, 16) || p.pos_row_stride % 8 != 0)) return refuse(ZIGMA_ERR_STRIDE);
    const int64_t L = static_cast<int64_t>(p.height / p.patch) * (p.width / p.patch);
    if (L > 0x7fffffff || p.batch > 65535) return refuse(ZIGMA_ERR_SHAPE);
    const int64_t want = (L + 15) / 16;
    const int64_t per = p.batch >= 64 ? 16 : (p.batch >= 8 ? 64 : 1024);      // ~1024+ workgroups, each staging the weight once for several tokens
    s.gx = static_cast<unsigned>(want < per ? want : per); s.gy = static_cast<unsigned>(p.batch); s.block = 256;
    s.lds = lds;
    s.inst = K == 3 || K == 4 || K == 12 || K == 16 ? static_cast<int>(K) : 0;
    s.kernel = "patch_embed";
    return s;
}

inline OuterPlan plan_timestep_embed(const zigma_timestep_embed_params_t &p) {
    OuterPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch < 0 || p.dim < 2) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.dtype != ZIGMA_BF16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.batch == 0) return s;
    if (!p.t || !p.freqs || !p.out) return refuse(ZIGMA_ERR_NULL);
    const int n = p.batch * (p.dim / 2);
    s.gx = static_cast<unsigned>((n + 255) / 256); s.block = 256;
    s.kernel = "timestep_embed";
    return s;
}

// the launch both final layers share: 16 rows per workgroup, the (n_out, cols) weight as bf16 in LDS, NP = 5 | 8 | 16 passes of 128 features
inline OuterPlan final_layer_launch(OuterPlan s, int64_t rows, int cols, int n_out, const char *kernel) {
    const int64_t want = (rows + 15) / 16;
    s.gx = static_cast<unsigned>(want < 4096 ? want : 4096); s.block = 256;
    s.lds = static_cast<int64_t>(n_out) * cols * 2;
    const int np = (cols + 127) / 128;
    s.inst = np <= 5 ? 5 : np <= 8 ? 8 : 16;
    s.kernel = kernel;
    return s;
}

inline OuterPlan plan_final_layer(const zigma_final_layer_params_t &p) {
    OuterPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.rows < 0 || p.cols < 8 || p.n_out < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.dtype != ZIGMA_BF16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.cols % 8 != 0 || p.cols > 128 * kFlMaxPass || p.n_out > 16) return refuse(ZIGMA_ERR_SHAPE);
    if (p.rows == 0) return s;
    if (!p.x || !p.weight || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!outer_al(p.x, 16) || p.x_row_stride % 8 != 0 || !outer_al(p.weight, 16)) return refuse(ZIGMA_ERR_STRIDE);
    return final_layer_launch(s, p.rows, p.cols, p.n_out, "final_layer");
}

inline OuterPlan plan_final_layer_cfg(const zigma_final_layer_cfg_params_t &p) {
    OuterPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.rows < 0 || p.cols < 8 || p.n_out < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.dtype != ZIGMA_BF16 || (p.out_dtype != ZIGMA_F32 && p.out_dtype != ZIGMA_BF16)) return refuse(ZIGMA_ERR_DTYPE);
    if (p.cols % 8 != 0 || p.cols > 128 * kFlMaxPass || p.n_out > 16) return refuse(ZIGMA_ERR_SHAPE);
    if (p.rows_per_sample < 1 || p.tokens_per_frame < 1 || p.grid_w < 1 || p.patch < 1 || p.chans < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (static_cast<int64_t>(p.patch) * p.patch * p.chans != p.n_out) return refuse(ZIGMA_ERR_SHAPE);
    if (p.rows % p.rows_per_sample != 0 || p.rows_per_sample % p.tokens_per_frame != 0 || p.tokens_per_frame % p.grid_w != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.rows == 0) return s;
    if (!p.x_cond || !p.x_uncond || !p.weight || !p.scale || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!outer_al(p.x_cond, 16) || !outer_al(p.x_uncond, 16) || p.x_row_stride % 8 != 0 || !outer_al(p.weight, 16) || !outer_al(p.y_out, 16) ||
        !outer_al(p.scale, 4) || !outer_al(p.out, p.out_dtype == ZIGMA_F32 ? 4 : 2))
        return refuse(ZIGMA_ERR_STRIDE);
    return final_layer_launch(s, p.rows, p.cols, p.n_out, "final_layer_cfg");
}

inline OuterPlan plan_skinny_linear(const zigma_skinny_params_t &p) {
    OuterPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.m < 0 || p.n < 0 || p.k < 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags & ~1) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.dtype != ZIGMA_BF16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.m > 64 || p.n % 16 != 0 || p.k % 128 != 0 || p.k > 1024) return refuse(ZIGMA_ERR_SHAPE);       // (64 x (k + 8) bf16 of LDS <= 129 KB; k / 128 instantiations)
    if (p.m == 0 || p.n == 0) return s;
    if (p.k == 0 || !p.x || !p.w || !p.out) return refuse(ZIGMA_ERR_NULL);
    auto mis = [](const void *q, int64_t rs, int al) { return !outer_al(q, al) || rs % (al / 2) != 0; };
    if (mis(p.x, p.x_row_stride, 16) || mis(p.w, p.w_row_stride, 16) || mis(p.out, p.out_row_stride, 8)) return refuse(ZIGMA_ERR_STRIDE);
    if (p.bias && !outer_al(p.bias, 8)) return refuse(ZIGMA_ERR_STRIDE);
    const int n_strips = p.n / 16;
    const int want = (n_strips + kSkWaves - 1) / kSkWaves;
    s.gx = want < 256 ? want : 256; s.block = 64 * kSkWaves;      // one workgroup per CU (LDS), persistent over the strips: x is staged once
    s.lds = static_cast<int64_t>(64) * (p.k + 8) * 2;
    s.inst = p.k / 32; s.silu = p.flags & 1;
    s.kernel = "skinny_linear_mfma";
    return s;
}

// zigma_*_fwd_plan: the launch's status and the kernel it would report (null: a refusal or an empty call)
inline int query_outer(const OuterPlan &s, const char **kernel) {
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
