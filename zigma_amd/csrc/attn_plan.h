// The plans of zigma_cross_attn_fwd (csrc/cross_attn.hip), zigma_cross_attn_bwd (csrc/cross_attn_bwd.hip) and zigma_scale_reduce_bwd
// (csrc/glue_bwd.hip): a call's refusal, or the kernel instantiation and launch geometry that serve it, and the tile constants the limits are made of.
// Plain C++ without HIP, so the CPU tests compile it on its own; a launcher only maps a plan to a template instantiation.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kXaD = 64;                 // cross_attn_kernel: head dim
constexpr int kXaWaves = 4, kXaTok = 16; // waves per workgroup, tokens per wave (MFMA M)
constexpr int kXbD = 64, kXbWaves = 4, kXbTok = 16;     // cross_attn_bwd_kernel: the same tile
constexpr int kGbRows = 64, kGbMaxIters = 64;           // scale_reduce_bwd_kernel: rows per workgroup, 128-column slabs at most

struct AttnPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call)
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned gx = 0, gy = 1, gz = 1, block = 0;
    int nkb = 0;                    // cross_attn_kernel<NKB, MASK_ALL, T> | cross_attn_bwd_kernel<NKB, ...>: 16-key blocks, n_ctx <= 16 NKB
    int masked = 0;                 // MASK_ALL: n_ctx <= 16 (NKB - 1)
    int tiles = 0;                  // 16-token tiles per wave
    int chunks = 0;                 // the backward's workgroups along the sequence = fp32 dK / dV partials the caller adds
    int has_r2 = 0;                 // scale_reduce_bwd_kernel<HAS_R2>
};

inline bool attn_mis(const void *q, int64_t rs, int64_t bs) { return reinterpret_cast<uintptr_t>(q) % 16 != 0 || rs % 8 != 0 || bs % 8 != 0; }

// 16-token tiles per wave = how many query tokens share one staging of K_h / V_h^T (20 KB): 8 (512 tokens per workgroup) where the
// sequence has them — 35.5 us against 38.0 with 4 and 40.2 with 16 at the headline shape (tools/attn_probe.py) —, 4 for short ones
inline int attn_tiles(int seqlen) { return seqlen >= 512 ? 8 : 4; }

inline AttnPlan plan_cross_attn(const zigma_xattn_params_t &p) {
    AttnPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch < 0 || p.seqlen < 0 || p.heads < 1 || p.n_ctx < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    // the softmax takes its maximum over the RAW scores and folds the scale into the exponent (fma(s, sc, -m * sc)): that is the
    // maximum of the scaled scores only for a positive scale (the reference's is head_dim^-0.5)
    if (!(p.scale > 0.f) || !(p.scale < 3.0e38f)) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.batch == 0 || p.seqlen == 0) return s;
    if (!p.q || !p.k || !p.v || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (p.dtype != ZIGMA_BF16 && p.dtype != ZIGMA_F16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.head_dim != kXaD || p.n_ctx > 128 || p.batch > 65535 || p.heads > 65535) return refuse(ZIGMA_ERR_SHAPE);
    if (attn_mis(p.q, p.q_row_stride, p.q_batch_stride) || attn_mis(p.k, p.k_row_stride, p.k_batch_stride) ||
        attn_mis(p.v, p.v_row_stride, p.v_batch_stride) || attn_mis(p.out, p.o_row_stride, p.o_batch_stride))
        return refuse(ZIGMA_ERR_STRIDE);
    s.tiles = attn_tiles(p.seqlen);
    const int tok_per_wg = kXaTok * kXaWaves * s.tiles;
    s.gx = (p.seqlen + tok_per_wg - 1) / tok_per_wg; s.gy = p.heads; s.gz = p.batch; s.block = 64 * kXaWaves;
    s.nkb = p.n_ctx <= 80 ? 5 : 8;
    s.masked = p.n_ctx <= 16 * (s.nkb - 1);
    s.kernel = "cross_attn_mfma";
    return s;
}

// zigma_cross_attn_bwd_chunks
inline int attn_bwd_chunks(int seqlen) {
    if (seqlen <= 0) return 0;
    const int tok_per_wg = kXbTok * kXbWaves * attn_tiles(seqlen);
    return (seqlen + tok_per_wg - 1) / tok_per_wg;
}

inline AttnPlan plan_cross_attn_bwd(const zigma_xattn_bwd_params_t &p) {
    AttnPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch < 0 || p.seqlen < 0 || p.heads < 1 || p.n_ctx < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    // the forward's domain (zigma_cross_attn_fwd takes a positive finite scale only): an inf or nan scale would come back as NaN gradients
    if (!(p.scale > 0.f) || !(p.scale < 3.0e38f)) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.batch == 0 || p.seqlen == 0) return s;
    if (!p.q || !p.k || !p.v || !p.dout || !p.dq || !p.dk_part || !p.dv_part) return refuse(ZIGMA_ERR_NULL);
    if (p.dtype != ZIGMA_BF16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.head_dim != kXbD || p.n_ctx > 128 || p.batch > 65535 || p.heads > 65535) return refuse(ZIGMA_ERR_SHAPE);
    s.chunks = attn_bwd_chunks(p.seqlen);
    if (p.chunks != s.chunks) return refuse(ZIGMA_ERR_SHAPE);
    if (attn_mis(p.q, p.q_row_stride, p.q_batch_stride) || attn_mis(p.k, p.k_row_stride, p.k_batch_stride) ||
        attn_mis(p.v, p.v_row_stride, p.v_batch_stride) || attn_mis(p.dout, p.do_row_stride, p.do_batch_stride) ||
        attn_mis(p.dq, p.dq_row_stride, p.dq_batch_stride) || reinterpret_cast<uintptr_t>(p.dk_part) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(p.dv_part) % 16 != 0)
        return refuse(ZIGMA_ERR_STRIDE);
    s.tiles = attn_tiles(p.seqlen);
    s.gx = p.chunks; s.gy = p.heads; s.gz = p.batch; s.block = 64 * kXbWaves;
    s.nkb = p.n_ctx <= 80 ? 5 : 8;
    s.kernel = "cross_attn_bwd_mfma";
    return s;
}

inline AttnPlan plan_scale_reduce_bwd(const zigma_glue_bwd_params_t &p) {
    AttnPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.rows < 0 || p.cols < 1 || p.rows_per_batch < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.rows == 0) return s;
    if (!p.dy || !p.a || !p.s || !p.r1) return refuse(ZIGMA_ERR_NULL);
    if (p.dtype != ZIGMA_BF16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.cols % 128 != 0 || p.cols > 128 * kGbMaxIters || p.rows_per_batch % kGbRows != 0 || p.rows % p.rows_per_batch != 0) return refuse(ZIGMA_ERR_SHAPE);
    auto bad = [](const void *q, int64_t st) { return q && (reinterpret_cast<uintptr_t>(q) % 16 != 0 || st % 8 != 0); };
    if (bad(p.dy, p.dy_row_stride) || bad(p.a, p.a_row_stride) || bad(p.out, p.out_row_stride) || bad(p.s, p.s_batch_stride)) return refuse(ZIGMA_ERR_STRIDE);
    s.gx = static_cast<unsigned>(p.rows / kGbRows); s.block = 256;
    s.has_r2 = p.r2 != nullptr;
    s.kernel = "scale_reduce_bwd";
    return s;
}

// zigma_*_plan: the launch's status and the kernel it would report (null: a refusal or an empty call)
inline int query_attn(const AttnPlan &s, const char **kernel) {
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
