// The plan of a zigma_linear_wgrad call (csrc/wgrad.hip): its refusal, or the kernel instantiation, the slab count, the workspace it needs and the launch
// geometry, and the tile constants the kernel is made of.  Plain C++ without HIP, so the CPU tests compile it on its own; the launcher only maps a plan
// to a template instantiation.
#pragma once
#include <stdint.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kWgBN = 128, kWgKT = 64, kWgThreads = 256;
constexpr int kWgMaxSlabs = 4096;

struct WgradPlan {
    int status = ZIGMA_OK;          // returned when kernel is null: a refusal
    const char *kernel = nullptr;   // zigma_last_kernel()
    unsigned gx = 0, gy = 0, block = 0;     // tiles x slabs
    int bk = 0;                     // wgrad_kernel<T, BK>
    int slabs = 0;                  // S: token slabs; S > 1 goes through the workspace and wgrad_reduce_kernel
    int64_t need = 0;               // zigma_linear_wgrad_workspace_bytes(): set wherever shape, types and flags pass, whatever else the block lacks
    int64_t slab_rows = 0;          // whole 64-token steps; slabs past m write zero partials
    int n_tiles = 0;
};

inline int wgrad_bk(const zigma_linear_wgrad_params_t &p) { return p.k <= 64 ? 64 : 128; }
inline int64_t wgrad_tiles(const zigma_linear_wgrad_params_t &p) {
    const int bk = wgrad_bk(p);
    return static_cast<int64_t>((p.n + kWgBN - 1) / kWgBN) * ((p.k + bk - 1) / bk);
}
// S: about two workgroups per CU (256 CUs) while a slab keeps >= 512 tokens; a non-zero `slabs` forces it
inline int wgrad_slabs(const zigma_linear_wgrad_params_t &p) {
    if (p.slabs > 0) return p.slabs;
    const int64_t tiles = wgrad_tiles(p);
    int64_t s = (512 + tiles - 1) / tiles;
    const int64_t most = p.m / 512;
    if (s > most) s = most;
    if (s > 64) s = 64;
    return s < 1 ? 1 : static_cast<int>(s);
}
inline int wgrad_check(const zigma_linear_wgrad_params_t &p) {
    if (p.dtype != ZIGMA_BF16 && p.dtype != ZIGMA_F16) return ZIGMA_ERR_DTYPE;
    if (p.out_dtype != p.dtype && p.out_dtype != ZIGMA_F32) return ZIGMA_ERR_DTYPE;
    if (p.m < 1 || p.n < 8 || p.k < 8 || p.n % 8 != 0 || p.k % 8 != 0 || p.n > 8192 || p.k > 8192 || p.slabs < 0 || p.slabs > kWgMaxSlabs)
        return ZIGMA_ERR_SHAPE;
    if (p.flags != 0) return ZIGMA_ERR_UNSUPPORTED;
    return ZIGMA_OK;
}

inline WgradPlan plan_wgrad(const zigma_linear_wgrad_params_t &p) {
    WgradPlan s;
    auto refuse = [&s](int status) { s.status = status; return s; };
    const int rc = wgrad_check(p);
    if (rc == ZIGMA_OK) {
        s.slabs = wgrad_slabs(p);
        s.need = s.slabs > 1 ? static_cast<int64_t>(s.slabs) * p.n * p.k * 4 : 0;
    }
    if (!p.dy || !p.x || !p.out) return refuse(ZIGMA_ERR_NULL);
    if (rc != ZIGMA_OK) return refuse(rc);
    if (s.need > 0 && !p.workspace) return refuse(ZIGMA_ERR_NULL);
    if (p.workspace_bytes < s.need) return refuse(ZIGMA_ERR_SHAPE);
    const int64_t out_elem = p.out_dtype == ZIGMA_F32 ? 4 : 2;
    if (p.dy_row_stride < p.n || p.x_row_stride < p.k || p.out_row_stride < p.k || p.dy_row_stride % 8 != 0 || p.x_row_stride % 8 != 0 ||
        reinterpret_cast<uintptr_t>(p.dy) % 16 != 0 || reinterpret_cast<uintptr_t>(p.x) % 16 != 0 || reinterpret_cast<uintptr_t>(p.out) % 16 != 0 ||
        (p.out_row_stride * out_elem) % 16 != 0 || (s.need > 0 && reinterpret_cast<uintptr_t>(p.workspace) % 16 != 0))
        return refuse(ZIGMA_ERR_STRIDE);
    const int S = s.slabs;
    s.bk = wgrad_bk(p);
    s.slab_rows = ((p.m + S - 1) / S + kWgKT - 1) / kWgKT * kWgKT;
    s.n_tiles = (p.n + kWgBN - 1) / kWgBN;
    s.gx = static_cast<unsigned>(wgrad_tiles(p)); s.gy = static_cast<unsigned>(S); s.block = kWgThreads;
    s.kernel = s.bk == 64 ? (S == 1 ? "wgrad_128x64" : "wgrad_128x64_splitk") : (S == 1 ? "wgrad_128x128" : "wgrad_128x128_splitk");
    return s;
}

// zigma_linear_wgrad_plan: the launch's status and the kernel it would report (null: a refusal)
inline int query_wgrad(const zigma_linear_wgrad_params_t &p, const char **kernel) {
    const WgradPlan s = plan_wgrad(p);
    *kernel = s.kernel;
    return s.status;
}

}  // namespace zigma
