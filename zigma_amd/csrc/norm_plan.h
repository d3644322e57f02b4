// The plans of zigma_add_norm_fwd (csrc/add_norm.hip) and zigma_add_norm_bwd (csrc/norm_bwd.hip): a call's refusal, or the kernel instantiation, the
// dtype slot, the launch geometry and (backward) the workspace it needs, and the constants the limits are made of.  Plain C++ without HIP, so the CPU
// tests compile it on its own; a launcher only maps a plan to a template instantiation.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "zigma_hip.h"

namespace zigma {

constexpr int kNbWaves = 4, kNbMaxWg = 512;     // add_norm_bwd_kernel: waves per workgroup, workgroups at most (one workspace partial each)

struct NormPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call)
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned gx = 0, block = 0;
    int vec = 0, iters = 0, lpr = 0;        // add_norm_kernel<.., VEC, ITERS, LPR> | add_norm_bwd_kernel<.., VEC, ITERS> (LPR 64: one row per wave)
    int res32 = 0, w32 = 0;         // the dtype slot: residual stream / weight in fp32, else in x's type
    unsigned fin_gx = 0;            // backward: add_norm_bwd_finish
    int64_t need = 0;               // backward: zigma_add_norm_bwd_workspace_bytes(), set wherever rows and cols are positive, whatever else the block lacks
};

// an operand of the access-width test: its address (null passes) and element size; `res`: a residual-stream pointer, which 16 bytes serve at width 8
// whatever its type (the fp32 stream is read in two 16-byte pieces)
struct NormOperand { const void *ptr; int64_t elem; bool res; };

// every operand and every pitch takes accesses of `w` elements
inline bool norm_width_ok(int w, int cols, std::initializer_list<NormOperand> ptrs, std::initializer_list<int64_t> pitches) {
    if (cols % w != 0) return false;
    for (int64_t s : pitches)
        if (s % w != 0) return false;
    for (const NormOperand &o : ptrs)
        if (reinterpret_cast<uintptr_t>(o.ptr) % static_cast<uintptr_t>(w == 8 && o.res ? 16 : w * o.elem) != 0) return false;
    return true;
}

// the dtype rules both directions share: x in any of the three types, the residual stream and the weight in fp32 or in x's type
inline int norm_dtype_slot(int x_dtype, int res_dtype, int w_dtype, NormPlan &s) {
    if (x_dtype != ZIGMA_F32 && x_dtype != ZIGMA_F16 && x_dtype != ZIGMA_BF16) return ZIGMA_ERR_DTYPE;
    s.res32 = res_dtype == ZIGMA_F32; s.w32 = w_dtype == ZIGMA_F32;
    if (!s.res32 && res_dtype != x_dtype) return ZIGMA_ERR_DTYPE;
    if (!s.w32 && w_dtype != x_dtype) return ZIGMA_ERR_DTYPE;
    return ZIGMA_OK;
}

inline NormPlan plan_add_norm(const zigma_norm_params_t &p) {
    NormPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (!p.x) return refuse(ZIGMA_ERR_NULL);
    if ((p.branch == nullptr) != (p.gate == nullptr)) return refuse(ZIGMA_ERR_NULL);
    if ((p.shift == nullptr) != (p.scale == nullptr)) return refuse(ZIGMA_ERR_NULL);
    if (p.shift && !p.y_mod) return refuse(ZIGMA_ERR_NULL);
    if (!p.y_out && !p.y_mod) return refuse(ZIGMA_ERR_NULL);
    if (p.rows < 0 || p.cols < 1 || p.rows_per_batch < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags & ~1) return refuse(ZIGMA_ERR_UNSUPPORTED);         // 1: one row per wave even where four fit (A/B probe)
    if (p.rows == 0) return s;
    // residual stream is f32 or the activation dtype; weights f32 or activation dtype; keep the instantiation set small: (x, res, w, mod) in
    // {(T,F32|T,F32|T,T)}
    if (p.mod_dtype != p.x_dtype && (p.gate || p.shift)) return refuse(ZIGMA_ERR_DTYPE);
    if (const int rc = norm_dtype_slot(p.x_dtype, p.res_dtype, p.w_dtype, s)) return refuse(rc);
    const int64_t xs = p.x_dtype == ZIGMA_F32 ? 4 : 2, rs = s.res32 ? 4 : xs, ws = s.w32 ? 4 : xs, ms = xs;
    auto wide = [&](int w) {
        return norm_width_ok(w, p.cols,
                             {{p.x, xs, false}, {p.branch, xs, false}, {p.x_out, xs, false}, {p.y_out, xs, false}, {p.y_mod, xs, false},
                              {p.residual, rs, true}, {p.residual_out, rs, true}, {p.weight, ws, false}, {p.bias, ws, false}, {p.gate, ms, false},
                              {p.shift, ms, false}, {p.scale, ms, false}},
                             {p.x_row_stride, p.branch_row_stride, p.x_out_row_stride, p.res_row_stride, p.res_out_row_stride, p.y_row_stride,
                              p.y_mod_row_stride, p.mod_batch_stride});
    };
    const bool vec = wide(4), vec8 = vec && wide(8) && xs == 2;        // 16-byte accesses for 16-bit activations
    // four rows per wave where a row is light (16-bit tensors only: 32 us against 44 for the pre-attention LayerNorm of the block);
    // with the fp32 residual stream in and out a row is 5-6 KB and one row per wave is the faster form (117 against 121 us)
    const bool light_rows = (p.residual == nullptr && p.residual_out == nullptr) || rs == 2;
    s.lpr = 64;
    if (vec8 && light_rows && p.cols % 128 == 0 && p.cols <= 128 * 8 && p.rows % 4 == 0 && !(p.flags & 1)) { s.vec = 8; s.iters = p.cols / 128; s.lpr = 16; }
    else if (vec8 && p.cols <= 512 * 2) { s.vec = 8; s.iters = 2; }
    else if (vec && p.cols <= 256 * 4) { s.vec = 4; s.iters = 4; }
    else if (vec && p.cols <= 256 * 16) { s.vec = 4; s.iters = 16; }
    else if (p.cols <= 64 * 16) { s.vec = 1; s.iters = 16; }
    else if (p.cols <= 64 * 64) { s.vec = 1; s.iters = 64; }
    else return refuse(ZIGMA_ERR_SHAPE);
    const int64_t waves = s.lpr == 16 ? p.rows / 4 : p.rows;           // four waves per workgroup
    s.gx = static_cast<unsigned>((waves + 3) / 4); s.block = 256;
    s.kernel = s.lpr == 16 ? "add_norm_v8x4" : vec ? "add_norm_v4" : "add_norm_v1";
    return s;
}

inline NormPlan plan_add_norm_bwd(const zigma_norm_bwd_params_t &p) {
    NormPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.rows > 0 && p.cols > 0) {
        const int64_t wg = (static_cast<int64_t>(p.rows) + kNbWaves - 1) / kNbWaves;
        s.gx = static_cast<unsigned>(wg < kNbMaxWg ? wg : kNbMaxWg);
        s.need = static_cast<int64_t>(s.gx) * 2 * p.cols * 4;         // one fp32 dweight and dbias partial per workgroup
    }
    if (p.rows < 0 || p.cols < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.rows == 0) return s;
    if (!p.xsum || !p.dy || (!p.dx && !p.dresidual)) return refuse(ZIGMA_ERR_NULL);
    if (!p.workspace || p.workspace_bytes < s.need) return refuse(ZIGMA_ERR_NULL);
    if (const int rc = norm_dtype_slot(p.x_dtype, p.res_dtype, p.w_dtype, s)) return refuse(rc);
    const int64_t xs = p.x_dtype == ZIGMA_F32 ? 4 : 2, rs = s.res32 ? 4 : xs, ws = s.w32 ? 4 : xs;
    const bool vec = norm_width_ok(4, p.cols,
                                   {{p.xsum, rs, true}, {p.dy, xs, false}, {p.dresidual_out, rs, true}, {p.dx, xs, false}, {p.dresidual, rs, true},
                                    {p.weight, ws, false}},
                                   {p.xsum_row_stride, p.dy_row_stride, p.dres_out_row_stride, p.dx_row_stride, p.dres_row_stride});
    s.lpr = 64;
    if (vec && p.cols <= 256 * 3) { s.vec = 4; s.iters = 3; }
    else if (vec && p.cols <= 256 * 8) { s.vec = 4; s.iters = 8; }
    else if (p.cols <= 64 * 4) { s.vec = 1; s.iters = 4; }
    else if (p.cols <= 64 * 12) { s.vec = 1; s.iters = 12; }
    else if (p.cols <= 64 * 32) { s.vec = 1; s.iters = 32; }
    else return refuse(ZIGMA_ERR_SHAPE);
    s.block = 64 * kNbWaves;
    s.fin_gx = 2 * ((p.cols + 63) / 64);
    s.kernel = "add_norm_bwd";
    return s;
}

// zigma_add_norm_*_plan: the launch's status and the kernel it would report (null: a refusal or an empty call)
inline int query_norm(const NormPlan &s, const char **kernel) {
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
