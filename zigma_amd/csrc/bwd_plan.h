// The plans of zigma_selective_scan_bwd (csrc/scan_bwd.hip) and zigma_causal_conv1d_bwd (csrc/conv_bwd.hip): a call's refusal, or the kernel
// instantiation, the workspace it needs and its sections, and the geometry of the main and the finishing launches, and the constants the limits are
// made of.  Plain C++ without HIP, so the CPU tests compile it on its own; a launcher only maps a plan to a template instantiation.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kBT = 16;                     // scan backward: steps per tile (one checkpoint each)
constexpr int kCbLT = 16, kCbSeg = 128;     // conv backward: positions per tile / per wave
constexpr int kBwdMaxBatch = 65535;         // both ride the batch in a 16-bit grid dimension

struct BwdPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call)
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned gx = 0, gy = 1, gz = 1, block = 0;
    int io = 0, wt = 0;             // zigma_dtype_t of the tensors / of the conv taps
    int inst = 0, silu = 0;         // scan_bwd_kernel<IO, NW = inst> | conv_bwd_tok_kernel<IO, WT, W = inst, silu>
    int64_t need = 0;               // zigma_*_bwd_workspace_bytes(): set wherever the sizes are positive, whatever else the block lacks
    int64_t ck = 0, bc = 0, pa = 0; // scan: floats of the workspace's sections (checkpoints — 0 with the forward's —, per-slab dB / dC, per-sample dA / dD / ddelta_bias)
    int n_tiles = 0, n_slabs = 0;   // scan
    int n_seg = 0, n_parts = 0;     // conv: segments of kCbSeg positions; partials the finishing kernel adds
    unsigned fin_gx = 0, fin2_gx = 0, fin_block = 256;      // scan_bwd_finish_bc, scan_bwd_finish_params | conv_bwd_finish
};

inline bool bwd_dtype_ok(int dt) { return dt == ZIGMA_F32 || dt == ZIGMA_F16 || dt == ZIGMA_BF16; }

inline BwdPlan plan_scan_bwd(const zigma_scan_bwd_params_t &p) {
    BwdPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch > 0 && p.dim > 0 && p.seqlen > 0 && p.dstate > 0) {
        const int64_t n_tiles = (p.seqlen + kBT - 1) / kBT, slabs = p.dim / 64;
        s.ck = p.checkpoints ? 0 : static_cast<int64_t>(p.batch) * slabs * n_tiles * p.dstate * 64;
        s.bc = static_cast<int64_t>(p.batch) * slabs * n_tiles * kBT * 2 * p.dstate;
        s.pa = static_cast<int64_t>(p.batch) * p.dim * (p.dstate + 2);
        s.need = (s.ck + s.bc + s.pa) * 4;
    }
    if (p.batch < 0 || p.dim < 0 || p.seqlen < 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.dim % 64 != 0 || (p.dstate != 16 && p.dstate != 8) || p.batch > kBwdMaxBatch) return refuse(ZIGMA_ERR_SHAPE);
    if (p.reset_period < 0 || p.reset_period % kBT != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.batch == 0 || p.dim == 0 || p.seqlen == 0) return s;      // nothing to write (parameter gradients: caller zero-fills)
    if (!p.u || !p.delta || !p.A || !p.B || !p.C || !p.dout || !p.du || !p.ddelta || !p.dA || !p.dB || !p.dC) return refuse(ZIGMA_ERR_NULL);
    if (p.z && (!p.out || !p.dz)) return refuse(ZIGMA_ERR_NULL);
    if ((p.D && !p.dD) || (p.delta_bias && !p.ddelta_bias)) return refuse(ZIGMA_ERR_NULL);
    if (!p.workspace || p.workspace_bytes < s.need) return refuse(ZIGMA_ERR_NULL);
    if (reinterpret_cast<uintptr_t>(p.workspace) % 16 != 0) return refuse(ZIGMA_ERR_STRIDE);
    // the 2^31 byte-offset bound over the ten pitches
    const int es = p.io_dtype == ZIGMA_F32 ? 4 : 2;
    const int64_t lim = (int64_t(1) << 31) - 1;
    const int64_t strides[] = {p.u_l_stride, p.delta_l_stride, p.z_l_stride, p.out_l_stride, p.dout_l_stride, p.du_l_stride,
                               p.ddelta_l_stride, p.dz_l_stride, p.B_l_stride, p.C_l_stride};
    for (int64_t st : strides)
        if (st < 0 || (p.seqlen - 1) * st * es + static_cast<int64_t>(p.dim) * es > lim) return refuse(ZIGMA_ERR_STRIDE);
    if (!bwd_dtype_ok(p.io_dtype)) return refuse(ZIGMA_ERR_DTYPE);
    s.io = p.io_dtype;
    s.inst = p.dstate == 16 ? 4 : 2;                                 // waves x 4 states
    s.n_tiles = (p.seqlen + kBT - 1) / kBT; s.n_slabs = p.dim / 64;
    s.gx = static_cast<unsigned>(s.n_slabs); s.gy = static_cast<unsigned>(p.batch); s.block = 64 * s.inst;
    const int64_t nbc = static_cast<int64_t>(p.batch) * p.seqlen * 2 * p.dstate, npa = static_cast<int64_t>(p.dim) * (p.dstate + 2);
    s.fin_gx = static_cast<unsigned>((nbc + 255) / 256); s.fin2_gx = static_cast<unsigned>((npa + 255) / 256);
    s.kernel = "scan_bwd_tok";
    return s;
}

inline BwdPlan plan_conv_bwd(const zigma_conv_bwd_params_t &p) {
    BwdPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (p.batch > 0 && p.dim > 0 && p.seqlen > 0) {
        s.n_seg = (p.seqlen + kCbSeg - 1) / kCbSeg;
        s.need = static_cast<int64_t>(p.batch) * s.n_seg * p.dim * (p.width + 1) * 4;      // one fp32 (dim, width + 1) partial per sample and segment
    }
    if (p.width < 2 || p.width > 4) return refuse(ZIGMA_ERR_SHAPE);
    if (p.batch < 0 || p.dim < 0 || p.seqlen < 0 || p.batch > kBwdMaxBatch) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags != 0) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.reset_period < 0 || p.reset_period % kCbLT != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.batch == 0 || p.dim == 0 || p.seqlen == 0) return s;
    if (!p.x || !p.weight || !p.dout || !p.dx || !p.dweight) return refuse(ZIGMA_ERR_NULL);
    if (p.bias && !p.dbias) return refuse(ZIGMA_ERR_NULL);
    if (!p.workspace || p.workspace_bytes < s.need) return refuse(ZIGMA_ERR_NULL);
    const int es = p.io_dtype == ZIGMA_F32 ? 4 : 2;
    auto bad = [&](const void *q, int64_t ls, int64_t bs) {
        return reinterpret_cast<uintptr_t>(q) % (4 * es) != 0 || ls % 4 != 0 || bs % 4 != 0 || ls < 0 ||
               (ls * p.seqlen + p.dim) * static_cast<int64_t>(es) >= (int64_t(1) << 31);
    };
    if (p.dim % 4 != 0 || bad(p.x, p.x_l_stride, p.x_batch_stride) || bad(p.dout, p.dout_l_stride, p.dout_batch_stride) ||
        bad(p.dx, p.dx_l_stride, p.dx_batch_stride))
        return refuse(ZIGMA_ERR_STRIDE);
    if (!bwd_dtype_ok(p.io_dtype) || !bwd_dtype_ok(p.w_dtype)) return refuse(ZIGMA_ERR_DTYPE);
    s.io = p.io_dtype; s.wt = p.w_dtype;
    s.inst = p.width; s.silu = p.silu_activation != 0;
    s.gx = static_cast<unsigned>((p.dim / 4 + 63) / 64); s.gy = static_cast<unsigned>(s.n_seg); s.gz = static_cast<unsigned>(p.batch); s.block = 64;
    s.fin_gx = static_cast<unsigned>((p.dim * (p.width + 1) + 63) / 64);
    s.n_parts = s.n_seg * p.batch;
    s.kernel = "conv_bwd_tok";
    return s;
}

// zigma_*_bwd_plan: the launch's status and the kernel it would report (null: a refusal or an empty call)
inline int query_bwd(const BwdPlan &s, const char **kernel) {
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
