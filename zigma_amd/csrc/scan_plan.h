// The plan of a zigma_selective_scan_fwd call: its refusal, or the kernel family, form and template switches that serve it.
// Plain C++ without HIP, so the CPU tests compile it on its own; the launchers only map a plan to template instantiations.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

#if defined(ZIGMA_SCAN_PROBES)      // probe library of tools/: scan_tok2_kernel's timing probes, flag bit 12 = time stamps into `checkpoints`
constexpr int kScanProbeBits = 0x7000, kScanStampBit = 0x1000, kDtpDebug = 0;
#elif defined(ZIGMA_DTP_DEBUG)      // debug library: the in-kernel dt_proj on every scan_tok2_kernel layout, dumps into `checkpoints`
constexpr int kScanProbeBits = 0, kScanStampBit = 0, kDtpDebug = 1;
#else
constexpr int kScanProbeBits = 0, kScanStampBit = 0, kDtpDebug = 0;
#endif

enum ScanForm { kScanWhole, kScanSplit, kScanSplitDtp, kScanDtp };

struct ScanPlan {
    int status = ZIGMA_OK;      // returned when family is 0: a refusal, or ZIGMA_OK (empty call, or batch slices)
    int family = 0;             // ZIGMA_SCAN_KERNEL_* (info[0])
    int slice = 0;              // > 0: run in batch slices of this many samples, each planned on its own
    ScanForm form = kScanWhole;
    int nw = 0, n_chunks = 0;   // switches: scan_tok_kernel <NW, EVEN, HAS_Z = z, HAS_OUT = out>, scan_tok2_kernel <SP, TAB, ZACT, OUT, R6, ACC>
    bool even = false, z = false, out = false, sp = false, tab = false, zact = false, r6 = false, acc = false;
    int info1 = 0;              // info[1]: `checkpoints` is being written
    const char *kernel = nullptr;   // zigma_last_kernel()
};

inline int64_t scan_slabs(const zigma_scan_params_t &p) { return static_cast<int64_t>(p.batch) * (p.dim / 64); }   // token-major workgroups
inline int scan_chunk_len(const zigma_scan_params_t &p) { return p.chunk_len > 0 ? p.chunk_len : 2048; }    // reference: selective_scan.cpp:307
inline int scan_n_chunks(const zigma_scan_params_t &p) { return (p.seqlen + scan_chunk_len(p) - 1) / scan_chunk_len(p); }

// the in-kernel dt_proj without a split reads no delta: u stands in for it, in the layout checks and in the kernel's parameters
inline zigma_scan_params_t scan_operands(const zigma_scan_params_t &p) {
    zigma_scan_params_t q = p;
    if (p.dt_x && !p.x) { q.delta = p.u; q.delta_batch_stride = p.u_batch_stride; q.delta_d_stride = p.u_d_stride; q.delta_l_stride = p.u_l_stride; }
    return q;
}

// token-major layout (both token-major kernels): channels contiguous in u / delta / z / out, input-dependent B and C in the activation dtype,
// one group, dstate 16 (4 waves x 4 states) or 8 (2 waves), dim a multiple of the 64-channel slab, 32-bit in-sample offsets
inline bool tok_layout_ok(const zigma_scan_params_t &p) {
    if (!p.is_variable_B || !p.is_variable_C || p.n_groups != 1 || p.bc_dtype != p.io_dtype) return false;
    if (p.dim % 64 != 0 || (p.dstate != 16 && p.dstate != 8) || p.u_d_stride != 1 || p.delta_d_stride != 1) return false;
    if ((p.z && (p.z_d_stride != 1 || p.out_z_d_stride != 1)) || (p.out && p.out_d_stride != 1)) return false;
    if (p.x && scan_chunk_len(p) % 16 != 0) return false;  // carries are stored at tile ends
    const int64_t lim = ((int64_t(1) << 31) - 1) / 4;     // byte offsets, up to 4-byte elements
    const int64_t ls[] = {p.u_l_stride, p.delta_l_stride, p.z ? p.z_l_stride : 0, p.out ? p.out_l_stride : 0, p.z ? p.out_z_l_stride : 0,
                          p.B_l_stride, p.C_l_stride};
    for (int64_t s : ls)
        if (s < 0 || s * p.seqlen > lim) return false;
    return true;
}

// scan_tok2_kernel, beyond tok_layout_ok(): 16-bit I/O, dstate 16, whole tiles, a gate; checkpoints only in the training form (ungated out
// as well, which has no pre-activated gate); B / C rows of even pitch on 4-byte boundaries; both row tables or neither
inline bool tok2_layout_ok(const zigma_scan_params_t &p) {
    if (p.dstate != 16 || p.seqlen % 16 != 0 || !p.z || p.io_dtype == ZIGMA_F32) return false;
    if (p.out && ((p.flags & ZIGMA_SCAN_Z_PREACTIVATED) || static_cast<int64_t>(p.out_l_stride) * 2 > 0x7fffffff)) return false;
    if (p.checkpoints && !p.out && !kDtpDebug && !(p.flags & kScanStampBit)) return false;
    if (p.B_dstate_stride != 1 || p.C_dstate_stride != 1 || ((p.B_l_stride | p.C_l_stride | p.B_batch_stride | p.C_batch_stride) & 1)) return false;
    if (((reinterpret_cast<uintptr_t>(p.B) | reinterpret_cast<uintptr_t>(p.C)) & 3) || (p.z_row_index == nullptr) != (p.out_row_index == nullptr)) return false;
    return scan_slabs(p) <= 0x7fffffff;
}

// dt_proj inside scan_tok2_kernel (whole sequence and split): softplus, 32 <= dt_rank <= 64 in steps of 8, x_dbl rows at least 64 wide,
// 16-byte aligned x_dbl / W_dt rows, 32-bit offsets into a sample's x_dbl rows
inline bool tok2_dt_operands_ok(const zigma_scan_params_t &p) {
    return p.delta_softplus && p.dt_rank >= 32 && p.dt_rank <= 64 && p.dt_rank % 8 == 0 && p.dt_x_l_stride % 8 == 0 && p.dt_x_batch_stride % 8 == 0 &&
           p.dt_w_row_stride % 8 == 0 && p.dt_x_l_stride >= 64 && reinterpret_cast<uintptr_t>(p.dt_x) % 16 == 0 &&
           reinterpret_cast<uintptr_t>(p.dt_w) % 16 == 0 && static_cast<int64_t>(p.seqlen) * p.dt_x_l_stride * 2 < 0x7fffffff;
}

// sequence split, only where the plain grid cannot fill the chip.  scan_tok2_kernel (chunks in gridDim.y): whole-tile chunks, 2 <= n_chunks
// <= 65535.  scan_tok_kernel (chunks in gridDim.z) never had the 65535 bound; its rule is kept as it is.
inline bool tok2_split_ok(const zigma_scan_params_t &p) {
    return scan_chunk_len(p) % 16 == 0 && scan_n_chunks(p) >= 2 && scan_n_chunks(p) <= 65535 && scan_slabs(p) < 768;
}
inline bool tok_split_ok(const zigma_scan_params_t &p) { return scan_n_chunks(p) >= 2 && scan_slabs(p) < 768; }

// six resident workgroups per CU where that saves a round of the grid (256 CUs: rounds of 1536 or of 1280 workgroups); probe bit 10 pins five
inline bool tok2_r6(const zigma_scan_params_t &p) {
    const int64_t w = scan_slabs(p);
    return (w + 1535) / 1536 < (w + 1279) / 1280 && !((p.flags >> ZIGMA_SCAN_PROBE_R5_SHIFT) & 1);
}

// samples [b0, b0 + n) of a token-major call; carries and checkpoints are per (sample, slab) as well
inline zigma_scan_params_t batch_slice(const zigma_scan_params_t &p, int b0, int n) {
    zigma_scan_params_t q = p;
    q.batch = p.batch - b0 < n ? p.batch - b0 : n;
    const int64_t es = p.io_dtype == ZIGMA_F32 ? 4 : 2;
    auto adv = [b0](const void *ptr, int64_t stride, int64_t esz) { return ptr ? const_cast<char *>(static_cast<const char *>(ptr)) + b0 * stride * esz : nullptr; };
    q.u = adv(p.u, p.u_batch_stride, es); q.delta = adv(p.delta, p.delta_batch_stride, es); q.z = adv(p.z, p.z_batch_stride, es);
    q.out = adv(p.out, p.out_batch_stride, es); q.out_z = adv(p.out_z, p.out_z_batch_stride, es);
    q.B = adv(p.B, p.B_batch_stride, es); q.C = adv(p.C, p.C_batch_stride, es);
    q.x = adv(p.x, int64_t(p.dim) * scan_n_chunks(p) * 2 * p.dstate, 4);
    q.checkpoints = reinterpret_cast<float *>(adv(p.checkpoints, int64_t(p.dim / 64) * ((p.seqlen + 15) / 16) * p.dstate * 64, 4));
    return q;
}

inline ScanPlan plan_scan(const zigma_scan_params_t &p) {
    ScanPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    auto serve = [&s](int family, ScanForm form, const char *kernel) { s.family = family; s.form = form; s.kernel = kernel; return s; };
    if (p.batch < 0 || p.dim < 0 || p.seqlen < 0 || p.dstate < 1 || p.dstate > 256) return refuse(ZIGMA_ERR_SHAPE);  // MAX_DSTATE
    if (p.n_groups < 1 || p.dim % p.n_groups != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.flags & ~(ZIGMA_SCAN_Z_PREACTIVATED | ZIGMA_SCAN_ACCUMULATE | ZIGMA_SCAN_PROBE_V1 | (1 << ZIGMA_SCAN_PROBE_PRIO_SHIFT) |
                    (1 << ZIGMA_SCAN_PROBE_R5_SHIFT) | kScanProbeBits))
        return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.batch == 0 || p.dim == 0 || p.seqlen == 0) return s;  // empty (pointers may be NULL): nothing to launch
    const bool pin_v1 = p.flags & ZIGMA_SCAN_PROBE_V1, zact = p.flags & ZIGMA_SCAN_Z_PREACTIVATED, acc = p.flags & ZIGMA_SCAN_ACCUMULATE;
    s.tab = p.z_row_index != nullptr; s.zact = zact; s.n_chunks = scan_n_chunks(p);

    if (p.dt_x) {       // dt_proj inside scan_tok2_kernel (ABI 9): no other kernel serves it
        if (!p.u || !p.dt_w || !p.A || !p.B || !p.C || !p.z || !p.out_z) return refuse(ZIGMA_ERR_NULL);
        if (p.reset_period < 0 || p.reset_period % 16 != 0) return refuse(ZIGMA_ERR_SHAPE);
        // with x, the sequence split (ABI 10): `delta` is a WORKSPACE of u's shape the first pass fills with softplus(dt_proj + bias)
        if (p.x && (!p.delta || p.reset_period != 0)) return refuse(p.delta ? ZIGMA_ERR_SHAPE : ZIGMA_ERR_NULL);
        const zigma_scan_params_t q = scan_operands(p);
        if ((p.io_dtype != ZIGMA_BF16 && p.io_dtype != ZIGMA_F16) || p.batch > 65535 || pin_v1 || !tok_layout_ok(q) || !tok2_layout_ok(q))
            return refuse(ZIGMA_ERR_UNSUPPORTED);
        if (p.x) {      // the first pass forms delta (MFMA + softplus) and writes it; the second reads it as a plain delta
            if (p.out || p.checkpoints || p.delta == p.u || zact || acc || !tok2_split_ok(q) || !tok2_dt_operands_ok(q)) return refuse(ZIGMA_ERR_UNSUPPORTED);
            return serve(ZIGMA_SCAN_KERNEL_TOK2, kScanSplitDtp, "scan_tok2_n16_split_dtproj");
        }
        if (!kDtpDebug && (p.out || p.checkpoints || !tok2_dt_operands_ok(q))) return refuse(ZIGMA_ERR_UNSUPPORTED);
        s.sp = true; s.r6 = tok2_r6(q); s.acc = acc;
        return serve(ZIGMA_SCAN_KERNEL_TOK2, kScanDtp, acc ? (s.r6 ? "scan_tok2_n16_dtproj_r6_acc" : "scan_tok2_n16_dtproj_acc")
                                                           : s.r6 ? "scan_tok2_n16_dtproj_r6" : "scan_tok2_n16_dtproj");
    }

    if (acc) return refuse(ZIGMA_ERR_UNSUPPORTED);       // (only the in-kernel dt_proj form adds to out_z)
    if (!p.u || !p.delta || !p.A || !p.B || !p.C || (p.z && !p.out_z) || (!p.z && !p.out)) return refuse(ZIGMA_ERR_NULL);
    if (p.reset_period < 0 || p.reset_period % 16 != 0 || (p.reset_period > 0 && p.x)) return refuse(ZIGMA_ERR_SHAPE);
    const bool tok = tok_layout_ok(p);
    auto dtype_ok = [](int t) { return t == ZIGMA_F32 || t == ZIGMA_F16 || t == ZIGMA_BF16; };
    if (p.reset_period > 0 && !tok) return refuse(ZIGMA_ERR_STRIDE);      // only the token-major kernels restart sequences
    if (zact && !(tok && p.io_dtype != ZIGMA_F32)) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (!tok) return dtype_ok(p.io_dtype) && dtype_ok(p.bc_dtype) ? serve(ZIGMA_SCAN_KERNEL_GENERIC, kScanWhole, "scan_generic") : refuse(ZIGMA_ERR_DTYPE);
    if (p.batch > 65535) { s.slice = 65535; return s; }      // the token-major grids carry the batch in gridDim.y
    if (!dtype_ok(p.io_dtype)) return refuse(ZIGMA_ERR_DTYPE);
    s.sp = p.delta_softplus != 0 || p.delta_bias != nullptr; s.out = p.out != nullptr;
    const bool split = p.x && !p.out && p.reset_period <= 0 && tok2_split_ok(p);
    if (tok2_layout_ok(p) && !pin_v1 && (!p.x || split)) {
        s.info1 = p.checkpoints && p.out && !(p.flags & kScanStampBit);
        return serve(ZIGMA_SCAN_KERNEL_TOK2, split ? kScanSplit : kScanWhole, "scan_tok2_n16");
    }
    if (zact) return refuse(ZIGMA_ERR_UNSUPPORTED);      // scan_tok2_kernel only
    s.nw = p.dstate == 16 ? 4 : 2; s.even = p.seqlen % 16 == 0; s.z = p.z != nullptr; s.info1 = p.checkpoints && p.z && p.out;
    return serve(ZIGMA_SCAN_KERNEL_TOK, p.x && tok_split_ok(p) ? kScanSplit : kScanWhole, p.dstate == 16 ? "scan_tok_n16" : "scan_tok_n8");
}

// every planned call of a zigma_selective_scan_fwd block, in launch order: the block itself, or its batch slices one after the other.
// each(q, plan) -> status; the first one that is not ZIGMA_OK ends the walk and is returned.  The launcher launches in it, the query reports.
template <typename Each>
inline int for_each_scan_call(const zigma_scan_params_t &p, Each each) {
    const ScanPlan plan = plan_scan(p);
    if (!plan.slice) return each(p, plan);
    for (int b0 = 0; b0 < p.batch; b0 += plan.slice) {
        const zigma_scan_params_t q = batch_slice(p, b0, plan.slice);
        const int rc = each(q, plan_scan(q));
        if (rc != ZIGMA_OK) return rc;
    }
    return ZIGMA_OK;
}

// zigma_selective_scan_fwd_plan: the launch's status and, where every call is served, the kernel of the last one
inline int query_scan(const zigma_scan_params_t &p, const char **kernel) {
    const char *last = nullptr;
    const int rc = for_each_scan_call(p, [&last](const zigma_scan_params_t &, const ScanPlan &plan) {
        if (plan.family) last = plan.kernel;
        return plan.family ? ZIGMA_OK : plan.status;
    });
    *kernel = rc == ZIGMA_OK ? last : nullptr;
    return rc;
}

}  // namespace zigma
