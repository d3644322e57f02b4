// The plan of a zigma_norm_linear_fwd call: its refusal, or the kernel instantiation and launch geometry that serve it, and the tile constants
// the kernel is made of.  Plain C++ without HIP, so the CPU tests compile it on its own; the launcher only maps a plan to a template instantiation.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kNlWaves = 4, kNlTok = 32;                            // norm_linear_kernel: waves per workgroup, rows per wave
constexpr int kNlTile = kNlWaves * kNlTok;                          // rows per workgroup (the token tile)
constexpr int kNlN = 512;                                           // output features (to_q: heads 8 x dim_head 64)
constexpr int kNlPass = 64;                                         // features per pass over the rows held in registers
constexpr int kNlStageBytes = 16384, kNlStages = 3;                 // ring of direct-to-LDS stages: 128 rows x 64 k of x, or 64 features x 128 k of w
constexpr int kNlOutPitch = 2 * kNlPass + 16;                       // bytes per row of a wave's output tile in LDS

struct NormLinearPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call)
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned grid = 0, block = 0;
    int ksteps = 0;                 // norm_linear_kernel <KS = k / 64, T>
};

inline bool nl_al(const void *q, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }

inline NormLinearPlan plan_norm_linear(const zigma_norm_linear_params_t &p) {
    NormLinearPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.m < 0 || p.n < 1 || p.k < 1 || p.rows_per_batch < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.m == 0) return s;         // empty: nothing to launch
    if (!p.x || !p.w || !p.shift || !p.scale || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (p.dtype != ZIGMA_BF16 && p.dtype != ZIGMA_F16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.n != kNlN || (p.k != 512 && p.k != 640 && p.k != 768)) return refuse(ZIGMA_ERR_SHAPE);       // (instantiation set: k / 64 = 8, 10, 12)
    if (p.m % kNlTile != 0 || p.m / kNlTile > 0x7fffffff) return refuse(ZIGMA_ERR_SHAPE);
    if (p.m % p.rows_per_batch != 0) return refuse(ZIGMA_ERR_SHAPE);        // whole samples: shift / scale hold m / rows_per_batch rows
    if (p.x_row_stride < p.k || p.w_row_stride < p.k || p.out_row_stride < p.n || p.mod_batch_stride < 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.x_row_stride * 16 > 0x7fffffff || p.w_row_stride * 16 > 0x7fffffff) return refuse(ZIGMA_ERR_SHAPE);   // 32-bit lane offsets over the 8 rows of a load
    // 16-byte pieces everywhere: direct-to-LDS loads of x and w, the lanes' shift / scale pieces, the output rows
    if (p.x_row_stride % 8 != 0 || p.w_row_stride % 8 != 0 || p.out_row_stride % 8 != 0 || p.mod_batch_stride % 8 != 0 || !nl_al(p.x, 16) || !nl_al(p.w, 16) ||
        !nl_al(p.shift, 16) || !nl_al(p.scale, 16) || !nl_al(p.out, 16))
        return refuse(ZIGMA_ERR_STRIDE);
    s.ksteps = p.k / 64;
    s.grid = static_cast<unsigned>(p.m / kNlTile); s.block = 64 * kNlWaves;
    s.kernel = p.k == 512 ? "norm_linear_k512" : p.k == 640 ? "norm_linear_k640" : "norm_linear_k768";
    return s;
}

// zigma_norm_linear_fwd_plan: the launch's status and the kernel it would report (null: a refusal or an empty call)
inline int query_norm_linear(const zigma_norm_linear_params_t &p, const char **kernel) {
    const NormLinearPlan s = plan_norm_linear(p);
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
