// The plans of a zigma_linear_fwd call and of a zigma_linear_f32_split call: the refusal, or the kernel family, template switches and launch geometry that
// serve it.
// Plain C++ without HIP, so the CPU tests compile it on its own; the launchers only map a plan to template instantiations.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

#if defined(ZIGMA_LINEAR4W_PROBES)  // probe library of tools/: timing variants of linear4w_kernel and linear_ws_kernel in flag bits 16 .. 18, start skew in bits 20 .. 23
constexpr int kLin4wFlags = 0xf70000;
constexpr bool kLinProbes = true;
#else
constexpr int kLin4wFlags = 0;
constexpr bool kLinProbes = false;
#endif

enum LinearFamily { kLinNone, kLinTn, kLin4w, kLinWs, kLinSm };     // csrc/linear.hip (8 waves), linear4w.hip, linear_ws.hip, linear_sm.hip

struct LinearPlan {
    int status = ZIGMA_OK;          // returned when family is kLinNone: a refusal, or ZIGMA_OK (empty call)
    LinearFamily family = kLinNone;
    const char *kernel = nullptr;   // zigma_last_kernel()
    int grid = 0, tiles_m = 0, tiles_n = 0;
    // linear_tn_kernel <WN_ = wide ? 4 : 2, NST = stages, HAS_BIAS = bias, RES = res>
    bool wide = false, bias = false, res = false;
    int stages = 0;
    // linear4w_kernel <EPI = epi, VARIANT = probe>; linear_sm_kernel <NBLK = nblk, EPI = epi != 0>
    int epi = 0, n_wide = 0, n_tiles = 0, nblk = 0;
    // linear_ws_kernel <KG = k / 16, FB = pw / 128, PROBE = probe, SL = silu>
    int pw = 0, panels = 0, ranges = 0, tiles_per_xcd = 0, probe = 0;
    bool silu = false;
};

// linear4w_kernel: the epilogue variant that serves the call (0 = 256-wide tiles only, 1 = + a narrow tile column, 2 = + gated residual, 3 = + bias), or -1.
// Whole 256-token tiles, k >= 192, at least one tile per CU (smaller: the 8-wave kernel), 16-byte stores, 32-bit tile offsets; gated residual: residual rows in
// the output's pitch (a multiple of 128 elements), samples of 2^i >= 128 rows; a bias only together with the gated residual, n <= 8192.  Any flag of the
// shipped library pins the 8-wave kernel; the probe variants exist for the epilogue-free form only.
inline int linear4w_variant(const zigma_linear_params_t &p) {
    if (p.flags & ~kLin4wFlags) return -1;
    if (p.silu_from_col < p.n) return -1;
    if (p.m % 256 != 0 || p.n % 128 != 0 || p.k % 64 != 0 || p.k < 192 || p.k / 64 > 4095) return -1;
    if (p.out_row_stride % 8 != 0 || reinterpret_cast<uintptr_t>(p.out) % 16 != 0) return -1;
    if (p.m * p.out_row_stride * 2 > 0xffffffffll) return -1;
    const int64_t tiles_n = p.n / 256 + (p.n % 256 != 0), n_tiles = (p.m / 256) * tiles_n;
    if (n_tiles < 256 || n_tiles > 0x7fffffff || tiles_n > 1023 || p.m / 256 > 0xfffff) return -1;
    int epi = p.n % 256 != 0 ? 1 : 0;
    if (p.residual) {
        if (!p.gate || p.res_row_stride != p.out_row_stride || p.out_row_stride % 128 != 0) return -1;
        if (p.rows_per_batch < 128 || (p.rows_per_batch & (p.rows_per_batch - 1)) != 0 || p.m % p.rows_per_batch != 0) return -1;
        if (reinterpret_cast<uintptr_t>(p.residual) % 16 != 0 || reinterpret_cast<uintptr_t>(p.gate) % 16 != 0 || p.gate_batch_stride % 8 != 0) return -1;
        epi = 2;
    }
    if (p.bias) {
        if (!p.residual || p.n > 8192 || reinterpret_cast<uintptr_t>(p.bias) % 2 != 0) return -1;
        epi = 3;
    }
    if (epi != 0 && (p.flags >> 16)) return -1;
    return epi;
}

// linear_ws_kernel: features per weight panel (256: k = 512 / 640, two 32-feature blocks per wave; 128: k = 1280 / 1536, one block per wave), or 0 if the
// kernel does not serve the call.  No bias / residual; SiLU on whole 128-column groups (a wave is all-or-nothing), 256-feature panels only; whole panels, at
// most 32 of them; every workgroup of an XCD owns at least one 512-token tile; 16-byte stores; x rows a multiple of 128 elements apart (the slot swizzle
// sits in the low byte of the lane offset); 32-bit lane offsets inside a slice and over the 16 rows of a store.
inline int linear_ws_panel(const zigma_linear_params_t &p) {
    if (p.bias || p.residual) return 0;
    const bool narrow = p.k == 1280 || p.k == 1536;
    if (!narrow && p.k != 512 && p.k != 640) return 0;          // (instantiation set: k / 16 = 32, 40 | 80, 96)
    const int pw = narrow ? 128 : 256;
    if (p.silu_from_col < p.n && (narrow || p.silu_from_col < 0 || p.silu_from_col % 128 != 0)) return 0;
    if (p.n % pw != 0 || p.n > 8192 || p.m % 512 != 0) return 0;
    if (p.out_row_stride % 8 != 0 || reinterpret_cast<uintptr_t>(p.out) % 16 != 0) return 0;
    const int panels = p.n / pw;
    if (panels > 32) return 0;
    const int ranges = 32 / panels;
    const int64_t tiles_per_xcd = p.m / 512;
    if (tiles_per_xcd < ranges || tiles_per_xcd > 0x7fffff) return 0;
    if (p.out_row_stride * 2 * 16 > 0x7fffffff) return 0;
    if (p.x_row_stride % 128 != 0 || 64 * p.x_row_stride * 2 >= 0x7fffffff) return 0;
    return pw;
}

// linear_sm_kernel: 32-feature blocks per tile (5: n % 160 == 0; 6: n % 192 == 0; 4: n % 128 == 0, tried in that order), or 0 if the kernel does not serve
// the call.  No activation, k >= 128, whole 128-token tiles, 16-byte stores, a bias on an 8-byte boundary (plan_linear has checked the residual's pointers,
// pitches and rows_per_batch % 256 == 0 already).
inline int linear_sm_blocks(const zigma_linear_params_t &p) {
    if (p.silu_from_col < p.n) return 0;
    if (p.k % 64 != 0 || p.k < 128 || p.m % 128 != 0 || p.m < 128) return 0;
    if (p.out_row_stride % 8 != 0 || reinterpret_cast<uintptr_t>(p.out) % 16 != 0) return 0;
    if (128 * p.x_row_stride * 2 > 0x7fffffff || 192 * p.w_row_stride * 2 > 0x7fffffff) return 0;
    if (p.bias && reinterpret_cast<uintptr_t>(p.bias) % 8 != 0) return 0;
    if (p.residual && (!p.gate || p.rows_per_batch % 128 != 0)) return 0;
    const int nblk = p.n % 160 == 0 ? 5 : p.n % 192 == 0 ? 6 : p.n % 128 == 0 ? 4 : 0;
    if (!nblk) return 0;
    if ((p.m / 128) * (p.n / (32 * nblk)) > 0x7fffffff) return 0;
    return nblk;
}

inline LinearPlan plan_linear(const zigma_linear_params_t &p) {
    LinearPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    auto serve = [&s](LinearFamily family, const char *kernel) { s.family = family; s.kernel = kernel; return s; };
    if (p.m < 0 || p.n < 1 || p.k < 1) return refuse(ZIGMA_ERR_SHAPE);
    // 0x100 ... 0x1000: timing / A-B probes of the 8-wave kernel (tools/linear_probe.py); 0x2000: the 8-wave kernel; 0x10000 ... 0xf00000: kLin4wFlags
    if (p.flags & ~(0xf73f00 | ZIGMA_LINEAR_WS | ZIGMA_LINEAR_SM)) return refuse(ZIGMA_ERR_UNSUPPORTED);
    if (p.m == 0) return s;     // empty: nothing to launch
    if (!p.x || !p.w || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (p.dtype != ZIGMA_BF16 && p.dtype != ZIGMA_F16) return refuse(ZIGMA_ERR_DTYPE);
    if (p.k % 64 != 0 || p.n % 128 != 0 || p.m % 8 != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.m * p.x_row_stride * 2 > 0x7fffffff || static_cast<int64_t>(p.n) * p.w_row_stride * 2 > 0x7fffffff || 256 * p.out_row_stride * 2 > 0x7fffffff)
        return refuse(ZIGMA_ERR_SHAPE);     // 32-bit lane offsets inside an operand tile / a wave's output rows
    if (p.silu_from_col < 0 || p.silu_from_col % 32 != 0) return refuse(ZIGMA_ERR_SHAPE);
    if (p.x_row_stride % 8 != 0 || p.w_row_stride % 8 != 0 || p.out_row_stride % 4 != 0 ||
        (reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.w)) % 16 != 0 || reinterpret_cast<uintptr_t>(p.out) % 8 != 0)
        return refuse(ZIGMA_ERR_STRIDE);
    if (p.residual) {           // gated residual epilogue
        if (!p.gate || p.rows_per_batch < 1 || p.rows_per_batch % 256 != 0 || p.m % p.rows_per_batch != 0) return refuse(ZIGMA_ERR_SHAPE);
        if (p.res_row_stride % 8 != 0 || p.gate_batch_stride % 8 != 0 || reinterpret_cast<uintptr_t>(p.residual) % 16 != 0 ||
            reinterpret_cast<uintptr_t>(p.gate) % 16 != 0 || 256 * p.res_row_stride * 2 > 0x7fffffff)
            return refuse(ZIGMA_ERR_STRIDE);
    }
    if (p.bias && (p.n > 4096 || reinterpret_cast<uintptr_t>(p.bias) % 4 != 0)) return refuse(ZIGMA_ERR_SHAPE);   // (the 8-wave kernel stages it in 8 KB of LDS)
    const int probe = (p.flags >> 16) & 7;

    if (p.flags & ZIGMA_LINEAR_WS) {
        s.pw = linear_ws_panel(p);
        s.silu = p.silu_from_col < p.n;
        // the probe forms exist in the probe library and for 256-feature panels only; the 128-feature panels have no SiLU form
        if (!s.pw || (s.pw == 128 ? probe || s.silu : probe && !kLinProbes)) return refuse(ZIGMA_ERR_UNSUPPORTED);
        s.panels = p.n / s.pw; s.ranges = 32 / s.panels; s.tiles_per_xcd = static_cast<int>(p.m / 512);
        s.probe = probe <= 4 ? probe : 0; s.grid = 256;
        return serve(kLinWs, s.silu ? "linear_ws_silu" : s.pw == 128 ? "linear_ws_128" : "linear_ws");
    }
    if (p.flags & ZIGMA_LINEAR_SM) {
        s.nblk = linear_sm_blocks(p);
        if (!s.nblk) return refuse(ZIGMA_ERR_UNSUPPORTED);
        s.tiles_n = p.n / (32 * s.nblk); s.grid = static_cast<int>((p.m / 128) * s.tiles_n); s.epi = p.bias || p.residual;
        return serve(kLinSm, s.nblk == 5 ? "linear_sm_128x160" : s.nblk == 6 ? "linear_sm_128x192" : "linear_sm_128x128");
    }
    s.epi = linear4w_variant(p);
    if (s.epi >= 0) {
        if (p.dtype == ZIGMA_F16 && probe) return refuse(ZIGMA_ERR_UNSUPPORTED);      // (probe variants: bf16 only)
        s.probe = probe; s.n_wide = p.n / 256; s.tiles_n = s.n_wide + (p.n % 256 != 0); s.n_tiles = static_cast<int>((p.m / 256) * s.tiles_n); s.grid = 256;
        return serve(kLin4w, p.n % 256 ? "linear4w_256x256+128" : "linear4w_256x256");
    }
    s.epi = 0;
    s.wide = p.n % 256 == 0 && !(p.flags & 0x1000) && !p.residual;       // 0x1000: force the 256 x 128 tile (probe)
    s.tiles_m = static_cast<int>((p.m + 255) / 256); s.tiles_n = p.n / (s.wide ? 256 : 128);
    const int64_t n_tiles = static_cast<int64_t>(s.tiles_m) * s.tiles_n;
    if (n_tiles > 0x7fffffff) return refuse(ZIGMA_ERR_SHAPE);
    s.grid = n_tiles < 256 ? static_cast<int>((n_tiles + 7) / 8 * 8) : 256;      // one persistent workgroup per CU; multiples of 8 keep the XCD map
    s.stages = (s.wide || (p.flags & 0x800)) ? 2 : 3;                              // 0x800: two stages on the 256 x 128 tile (probe)
    s.bias = p.bias != nullptr; s.res = p.residual && s.stages == 3;
    return serve(kLinTn, s.wide ? "linear_tn_256x256" : "linear_tn_256x128");
}

// zigma_linear_fwd_plan: the launch's status and the kernel it would report (null: a refusal or an empty call)
inline int query_linear(const zigma_linear_params_t &p, const char **kernel) {
    const LinearPlan s = plan_linear(p);
    *kernel = s.family == kLinNone ? nullptr : s.kernel;
    return s.status;
}

// The plan of a zigma_linear_f32_split call (csrc/linear_split.hip): its refusal, or the instantiation (one pass or three) and the grid of
// 128-token x 128-feature tiles that serve it.
constexpr int kSplitBM = 128, kSplitBN = 128;

struct LinearSplitPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal, or ZIGMA_OK (empty call)
    const char *kernel = nullptr;   // zigma_last_kernel()
    bool lo = false;                // three passes: the w_lo plane is read
    int64_t tiles = 0;
};

inline LinearSplitPlan plan_linear_split(const zigma_linear_split_params_t &p) {
    LinearSplitPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    if (!p.x || !p.w_hi || !p.out || (p.passes == 3 && !p.w_lo)) return refuse(ZIGMA_ERR_NULL);
    if (p.flags != 0 || (p.passes != 1 && p.passes != 3)) return refuse(ZIGMA_ERR_UNSUPPORTED);
    s.lo = p.passes == 3;
    if (p.m < 0 || p.m % 8 != 0 || p.n < 128 || p.n % 128 != 0 || p.n > 65536 || p.k < 64 || p.k % 64 != 0 || p.k > 65536) return refuse(ZIGMA_ERR_SHAPE);
    if (p.x_row_stride < p.k || p.w_hi_row_stride < p.k || (s.lo && p.w_lo_row_stride < p.k) || p.out_row_stride < p.n) return refuse(ZIGMA_ERR_SHAPE);
    s.tiles = (p.m + kSplitBM - 1) / kSplitBM * (p.n / kSplitBN);
    if (s.tiles > 0x7fffffff) return refuse(ZIGMA_ERR_SHAPE);
    const auto misaligned = [](const void *q) { return reinterpret_cast<uintptr_t>(q) % 16 != 0; };
    if (misaligned(p.x) || misaligned(p.w_hi) || (s.lo && misaligned(p.w_lo)) || misaligned(p.out) || (p.bias && misaligned(p.bias)) ||
        p.x_row_stride % 4 != 0 || p.out_row_stride % 4 != 0 || p.w_hi_row_stride % 8 != 0 || (s.lo && p.w_lo_row_stride % 8 != 0))
        return refuse(ZIGMA_ERR_STRIDE);
    if (p.m == 0) return s;         // empty: nothing to launch
    s.kernel = s.lo ? "linear_split3_128x128" : "linear_split1_128x128";
    return s;
}

inline int query_linear_split(const zigma_linear_split_params_t &p, const char **kernel) {
    const LinearSplitPlan s = plan_linear_split(p);
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
