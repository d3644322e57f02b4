// The plans of the four entry points of the Mamba inner's front (zigma_causal_conv1d_fwd, zigma_conv_x_proj_fwd, zigma_x_proj_fwd,
// zigma_dt_proj_softplus_fwd): a call's refusal, or the kernel, template switches and launch geometry that serve it, and the tile constants
// the grids are made of.  Plain C++ without HIP, so the CPU tests compile it on its own; the launchers only map a plan to template instantiations.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kConvTokLT = 16;                                      // conv_tok_kernel: scan positions per lane
constexpr int kCxTok = 32, kCxBK = 64;                              // conv_x_proj_kernel: positions per wave, channels per stage
constexpr int kXpWaves = 8, kXpTok = 32, kXpChunk = 256, kXpRows = 96, kXpDepth = 4;    // x_proj_kernel
constexpr int kXsWaves = 8, kXsMaxSteps = 12;                       // x_proj_splitk_kernel
constexpr int kDtTokPerWave = 32, kDtChPerBlock = 64, kDtWaves = 4; // dt_proj_softplus_kernel
#ifndef ZIGMA_DT_ITERS
#define ZIGMA_DT_ITERS 4
#endif
constexpr int kDtIters = ZIGMA_DT_ITERS;

struct FrontPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call, or batch slices)
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned gx = 1, gy = 1, gz = 1, block = 0;
    int slice = 0;                  // conv, > 0: run in batch slices of this many samples, each planned on its own
    // conv_tok_kernel <W = width, LT = kConvTokLT, SILU = silu> when tok, conv_generic_kernel <CONTIG_L = contig_l> otherwise
    bool tok = false, silu = false, contig_l = false;
    int width = 0;
    int stages = 0, waves = 0;      // conv_x_proj_kernel <NST = stages, NW = waves>
    bool splitk = false;            // x_proj_splitk_kernel, not x_proj_kernel
};

inline bool front_dtype_ok(int t) { return t == ZIGMA_F32 || t == ZIGMA_F16 || t == ZIGMA_BF16; }
inline bool front_16bit(int t) { return t == ZIGMA_BF16 || t == ZIGMA_F16; }
inline bool front_al(const void *q, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(q) % bytes == 0; }

// samples [b0, b0 + n) of a conv call
inline zigma_conv_params_t conv_slice(const zigma_conv_params_t &p, int b0, int n) {
    zigma_conv_params_t q = p;
    q.batch = p.batch - b0 < n ? p.batch - b0 : n;
    const int64_t es = p.io_dtype == ZIGMA_F32 ? 4 : 2;
    q.x = static_cast<const char *>(p.x) + static_cast<int64_t>(b0) * p.x_batch_stride * es;
    q.out = static_cast<char *>(p.out) + static_cast<int64_t>(b0) * p.out_batch_stride * es;
    return q;
}

inline FrontPlan plan_conv1d(const zigma_conv_params_t &p) {
    FrontPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    auto serve = [&s](const char *kernel, unsigned block) { s.kernel = kernel; s.block = block; return s; };
    if (p.width < 2 || p.width > 4) return refuse(ZIGMA_ERR_SHAPE);  // causal_conv1d.cpp:157
    if (p.batch < 0 || p.dim < 0 || p.seqlen < 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.batch == 0 || p.dim == 0 || p.seqlen == 0) return s;  // empty (pointers may be NULL): nothing to launch
    if (!p.x || !p.weight || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!front_dtype_ok(p.io_dtype) || !front_dtype_ok(p.w_dtype)) return refuse(ZIGMA_ERR_DTYPE);
    if (p.batch > 65535) { s.slice = 65535; return s; }     // batch rides in gridDim.z: larger batches (video: batch x tokens-per-frame rows) go in slices
    const int64_t es = p.io_dtype == ZIGMA_F32 ? 4 : 2;
    // token-major: a lane's 4 adjacent channels are one aligned access, 32-bit byte offsets inside a sample
    s.tok = p.x_c_stride == 1 && p.out_c_stride == 1 && p.dim % 4 == 0 && front_al(p.x, 4 * es) && front_al(p.out, 4 * es) &&
            p.x_l_stride % 4 == 0 && p.out_l_stride % 4 == 0 && p.x_batch_stride % 4 == 0 && p.out_batch_stride % 4 == 0 &&
            p.x_l_stride >= 0 && p.out_l_stride >= 0 &&
            (p.x_l_stride * p.seqlen + p.dim) * es < (int64_t(1) << 31) &&
            (p.out_l_stride * p.seqlen + p.dim) * es < (int64_t(1) << 31);
    if (p.reset_period < 0 || p.reset_period % 16 != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.reset_period > 0 && !s.tok) return refuse(ZIGMA_ERR_STRIDE);   // only the token-major kernel restarts sequences
    if (s.tok) {
        s.width = p.width; s.silu = p.silu_activation != 0;
        s.gx = (p.dim / 4 + 63) / 64; s.gy = (p.seqlen + kConvTokLT - 1) / kConvTokLT; s.gz = p.batch;
        return serve("conv_tok", 64);
    }
    s.contig_l = p.x_l_stride == 1;
    s.gx = static_cast<unsigned>((static_cast<int64_t>(p.batch) * p.dim * p.seqlen + 255) / 256);
    return serve("conv_generic", 256);
}

// every planned call of a zigma_causal_conv1d_fwd block, in launch order: the block itself, or its batch slices one after the other.
// each(q, plan) -> status; the first one that is not ZIGMA_OK ends the walk and is returned.  The launcher launches in it, the query reports.
template <typename Each>
inline int for_each_conv_call(const zigma_conv_params_t &p, Each each) {
    const FrontPlan plan = plan_conv1d(p);
    if (!plan.slice) return each(p, plan);
    for (int b0 = 0; b0 < p.batch; b0 += plan.slice) {
        const zigma_conv_params_t q = conv_slice(p, b0, plan.slice);
        const int rc = each(q, plan_conv1d(q));
        if (rc != ZIGMA_OK) return rc;
    }
    return ZIGMA_OK;
}

// the zigma_*_fwd_plan queries: the launch's status and the kernel it would report (null: nothing would launch)
inline int query_front(const FrontPlan &s, const char **kernel) {
    *kernel = s.kernel;
    return s.status;
}
inline int query_conv1d(const zigma_conv_params_t &p, const char **kernel) {
    const char *last = nullptr;
    const int rc = for_each_conv_call(p, [&last](const zigma_conv_params_t &, const FrontPlan &plan) {
        if (plan.kernel) last = plan.kernel;
        return plan.status;
    });
    *kernel = rc == ZIGMA_OK ? last : nullptr;
    return rc;
}

// default: 4-wave workgroups (128 positions), two stages = 66 KB of LDS: two workgroups per CU that drift apart, one computing
// while the other waits for its loads (measured 72 us; 8 waves in lockstep 75 us; a third stage does not pay, the second
// workgroup does its job).  flags: 1 = three stages, 2 = eight-wave workgroups; probes (wrong results): 4 = no u stores,
// 8 = no conv arithmetic.
inline FrontPlan plan_conv_x_proj(const zigma_conv_xproj_params_t &p) {
    FrontPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch < 0 || p.seqlen < 0 || p.dim < 1 || p.n < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags & ~15) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.batch == 0 || p.seqlen == 0) return s;
    if (!p.x || !p.conv_weight || !p.conv_bias || !p.w || !p.u || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!front_16bit(p.dtype)) return refuse(ZIGMA_ERR_DTYPE);
    if (p.n > 96 || p.n % 8 != 0 || p.dim % kCxBK != 0 || p.seqlen % kCxTok != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.out_row_stride % 8 != 0 || !front_al(p.out, 16)) return refuse(ZIGMA_ERR_STRIDE);
    const int64_t m = static_cast<int64_t>(p.batch) * p.seqlen;
    if (m % (kCxTok * 8) != 0) return refuse(ZIGMA_ERR_SHAPE);       // (either workgroup size)
    if (p.x_l_stride % 8 != 0 || p.x_batch_stride % 8 != 0 || p.u_l_stride % 8 != 0 || p.u_batch_stride % 8 != 0 || p.w_row_stride % 8 != 0 ||
        !front_al(p.x, 16) || !front_al(p.u, 16) || !front_al(p.w, 16) || !front_al(p.conv_weight, 16) || !front_al(p.conv_bias, 16))
        return refuse(ZIGMA_ERR_STRIDE);
    s.stages = (p.flags & 1) ? 3 : 2; s.waves = (p.flags & 2) ? 8 : 4;
    s.gx = static_cast<unsigned>(m / (kCxTok * s.waves)); s.block = 64 * s.waves;
    s.kernel = "conv_x_proj_mfma";
    return s;
}

inline FrontPlan plan_x_proj(const zigma_xproj_params_t &p) {
    FrontPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.m < 0 || p.n < 1 || p.k < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.m == 0) return s;
    if (!p.x || !p.w || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!front_16bit(p.dtype)) return refuse(ZIGMA_ERR_DTYPE);
    if (p.n > kXpRows || p.k % kXpChunk != 0 || p.k / 16 < kXpDepth) return refuse(ZIGMA_ERR_SHAPE);
    if (p.x_row_stride % 8 != 0 || p.w_row_stride % 8 != 0 || !front_al(p.x, 16) || !front_al(p.w, 16)) return refuse(ZIGMA_ERR_STRIDE);
    // few tokens: K split over the waves of 32-token workgroups (the streaming form would leave most CUs idle)
    s.splitk = p.m < 16384 && p.k % (16 * kXsWaves) == 0 && p.k / (16 * kXsWaves) <= kXsMaxSteps;
    const int64_t tok_per_wg = s.splitk ? kXpTok : kXpTok * kXpWaves;
    s.gx = static_cast<unsigned>((p.m + tok_per_wg - 1) / tok_per_wg); s.block = 64 * (s.splitk ? kXsWaves : kXpWaves);
    s.kernel = s.splitk ? "x_proj_splitk" : "x_proj_mfma";
    return s;
}

inline FrontPlan plan_dt_proj(const zigma_dtproj_params_t &p) {
    FrontPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.m < 0 || p.n < 0 || p.k < 1) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags & ~1) return refuse(ZIGMA_ERR_UNSUPPORTED);         // 1: four-byte stores as the accumulators lie (A/B probe)
    if (p.m == 0 || p.n == 0) return s;
    if (!p.x || !p.w || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (!front_16bit(p.dtype)) return refuse(ZIGMA_ERR_DTYPE);
    if (p.k > 48 || p.k % 8 != 0 || p.n % kDtChPerBlock != 0) return refuse(ZIGMA_ERR_SHAPE);
    // 16-byte fragment loads, 4-byte packed stores
    if (p.x_row_stride % 8 != 0 || p.w_row_stride % 8 != 0 || p.out_row_stride % 2 != 0 || !front_al(p.x, 16) || !front_al(p.w, 16) || !front_al(p.out, 4))
        return refuse(ZIGMA_ERR_STRIDE);
    const int64_t tok_per_block = kDtTokPerWave * kDtWaves * kDtIters;
    s.gx = p.n / kDtChPerBlock; s.gy = static_cast<unsigned>((p.m + tok_per_block - 1) / tok_per_block); s.block = 64 * kDtWaves;
    s.kernel = "dt_proj_softplus_mfma";
    return s;
}

}  // namespace zigma
