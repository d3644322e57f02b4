// zigma_sde_step_fwd / zigma_sde_advance: one launch of an SDE sampler's step with the Wiener increment drawn inside the kernel (include/zigma_hip.h).
// out = c0 a + c1 b + c2 c + cn xi over n contiguous elements; the coefficients, the Philox key, the stream and the step counter all come from device
// memory, so a captured step replays for every step of a trajectory.  Launch-bound at every shape a sampler has (64 latents are 1 MB): the accurate
// library logf / sqrtf / sincospif are used, not the fast intrinsics.
#include <cmath>

#include "zigma_common.h"

namespace zigma {

constexpr int kSdeThreads = 256;
constexpr int kSdeOct = 8;                                      // elements per lane: two quads of the noise field

// (philox4x32_10: zigma_common.h)
// two words -> two normals (the map of the header): u in (0, 1] and x in [0, 2) are exact in fp32
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float &even, float &odd) {
    const float u = static_cast<float>((ra >> 8) + 1u) * 0x1p-24f;
    const float x = static_cast<float>(rb >> 8) * 0x1p-23f;
    const float rho = sqrtf(-2.f * logf(u));
    float s, k;
    sincospif(x, &s, &k);
    even = __fmul_rn(rho, k);
    odd = __fmul_rn(rho, s);
}

// the 8 elements of a lane (cnt < 8: the call's last elements, one by one; the rest reads as 0 and is never stored)
template <typename T> __device__ __forceinline__ void load_oct(const void *base, int64_t at, int cnt, float (&v)[kSdeOct]) {
    if (cnt == kSdeOct) {
        if constexpr (T::id == ZIGMA_F32) {
            const v4f lo = *reinterpret_cast<const v4f *>(static_cast<const float *>(base) + at);
            const v4f hi = *reinterpret_cast<const v4f *>(static_cast<const float *>(base) + at + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = lo[j];
                v[4 + j] = hi[j];
            }
        } else {
            const u32x4 w = *reinterpret_cast<const u32x4 *>(static_cast<const uint16_t *>(base) + at);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[2 * j] = lo16<T>(w[j]);
                v[2 * j + 1] = hi16<T>(w[j]);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kSdeOct; ++j) v[j] = j < cnt ? ld<T>(base, at + j) : 0.f;
}

template <typename T> __device__ __forceinline__ void store_oct(void *base, int64_t at, int cnt, const float (&v)[kSdeOct]) {
    if (cnt == kSdeOct) {
        if constexpr (T::id == ZIGMA_F32) {
            *reinterpret_cast<v4f *>(static_cast<float *>(base) + at) = v4f{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<v4f *>(static_cast<float *>(base) + at + 4) = v4f{v[4], v[5], v[6], v[7]};
        } else {
            *reinterpret_cast<u32x4 *>(static_cast<uint16_t *>(base) + at) = u32x4{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])};
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kSdeOct; ++j)
        if (j < cnt) st<T>(base, at + j, v[j]);
}

// (out may be a: no __restrict__ on the operands)
template <typename T>
__global__ __launch_bounds__(kSdeThreads) void sde_step_kernel(const void *a, const void *b, const void *c, void *out, const float *__restrict__ coef,
                                                               const zigma_sde_state_t *__restrict__ state, uint32_t *__restrict__ bits_out, int64_t n,
                                                               int64_t elem_offset, int64_t coef_rows, int rows_per_step, int row, int absolute) {
    const int64_t at = (static_cast<int64_t>(blockIdx.x) * kSdeThreads + threadIdx.x) * kSdeOct;
    if (at >= n) return;
    const int cnt = n - at < kSdeOct ? static_cast<int>(n - at) : kSdeOct;
    zigma_sde_state_t s = {0u, 0u, 0u, 0u};
    if (state) s = *state;
    int64_t r = absolute ? static_cast<int64_t>(row) : static_cast<int64_t>(s.step) * rows_per_step + row;
    r = r < coef_rows ? r : coef_rows - 1;                                          // a relative row past the table: the last row
    const v4f k = *reinterpret_cast<const v4f *>(coef + 4 * r);
    float acc[kSdeOct] = {};
    if (state && k.w != 0.f) {
        const uint64_t quad = static_cast<uint64_t>(elem_offset + at) >> 2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (4 * h < cnt) {                                                      // (the second quad of the call's last lane may not exist)
                const uint64_t q = quad + h;
                const u32x4 w = philox4x32_10(u32x4{static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), s.step, s.stream}, s.seed_lo, s.seed_hi);
                if (bits_out) *reinterpret_cast<u32x4 *>(bits_out + at + 4 * h) = w;
                float z[4];
                box_muller(w.x, w.y, z[0], z[1]);
                box_muller(w.z, w.w, z[2], z[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * h + j] = __builtin_fmaf(k.w, z[j], 0.f);
            }
        }
    }
    float v[kSdeOct];
    if (c) {
        load_oct<T>(c, at, cnt, v);
#pragma unroll
        for (int j = 0; j < kSdeOct; ++j) acc[j] = __builtin_fmaf(k.z, v[j], acc[j]);
    }
    if (b) {
        load_oct<T>(b, at, cnt, v);
#pragma unroll
        for (int j = 0; j < kSdeOct; ++j) acc[j] = __builtin_fmaf(k.y, v[j], acc[j]);
    }
    if (a) {
        load_oct<T>(a, at, cnt, v);
#pragma unroll
        for (int j = 0; j < kSdeOct; ++j) acc[j] = __builtin_fmaf(k.x, v[j], acc[j]);
    }
    store_oct<T>(out, at, cnt, acc);
}

// one workgroup: every lane reads the counter before lane 0 writes it back
__global__ __launch_bounds__(kSdeThreads) void sde_advance_kernel(zigma_sde_state_t *state, const float *__restrict__ times, float *__restrict__ t_out, int64_t n_rows,
                                                                  int n_t, int batch) {
    const uint32_t step = state->step + 1u;
    __syncthreads();
    if (threadIdx.x == 0) state->step = step;
    const int64_t r = static_cast<int64_t>(step) < n_rows ? static_cast<int64_t>(step) : n_rows - 1;
    const int64_t total = static_cast<int64_t>(n_t) * batch;
    for (int64_t i = threadIdx.x; i < total; i += kSdeThreads) t_out[i] = times[r * n_t + i / batch];
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace zigma

using namespace zigma;

extern "C" int zigma_sde_step_fwd(const zigma_sde_step_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_sde_step_params_t &p = *pp;
    const int64_t per_group = static_cast<int64_t>(kSdeThreads) * kSdeOct;
    if (p.n < 0 || p.n > 0x7fffffffLL * per_group) return ZIGMA_ERR_SHAPE;
    if (p.elem_offset < 0 || p.elem_offset % 4 != 0 || p.elem_offset > INT64_MAX - p.n) return ZIGMA_ERR_SHAPE;
    if (p.rows_per_step < 1) return ZIGMA_ERR_SHAPE;
    if (p.row < 0) return ZIGMA_ERR_SHAPE;
    const bool absolute = (p.flags & ZIGMA_SDE_ROW_ABSOLUTE) != 0;
    if (p.coef_rows < 1 || (absolute && p.row >= p.coef_rows)) return ZIGMA_ERR_SHAPE;
    if (p.flags & ~ZIGMA_SDE_ROW_ABSOLUTE) return ZIGMA_ERR_UNSUPPORTED;
    if (p.dtype != ZIGMA_F32 && p.dtype != ZIGMA_F16 && p.dtype != ZIGMA_BF16) return ZIGMA_ERR_DTYPE;
    if (p.n == 0) return ZIGMA_OK;
    if (!p.out || !p.coef) return ZIGMA_ERR_NULL;
    if (!p.state && (!absolute || p.bits_out)) return ZIGMA_ERR_NULL;
    if (!aligned16(p.a) || !aligned16(p.b) || !aligned16(p.c) || !aligned16(p.out) || !aligned16(p.coef) || !aligned16(p.state) || !aligned16(p.bits_out))
        return ZIGMA_ERR_STRIDE;
    const dim3 grid(static_cast<unsigned>((p.n + per_group - 1) / per_group));
    ZIGMA_DISPATCH_DTYPE(p.dtype, T,
                         hipLaunchKernelGGL((sde_step_kernel<T>), grid, dim3(kSdeThreads), 0, static_cast<hipStream_t>(stream_), p.a, p.b, p.c, p.out, p.coef, p.state,
                                            p.bits_out, p.n, p.elem_offset, p.coef_rows, p.rows_per_step, p.row, absolute ? 1 : 0));
    set_last_kernel("sde_step");
    return check_launch();
}

extern "C" int zigma_sde_advance(const zigma_sde_advance_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_sde_advance_params_t &p = *pp;
    if ((p.n_t != 1 && p.n_t != 2) || p.batch < 1 || p.n_rows < 1) return ZIGMA_ERR_SHAPE;
    if (p.flags != 0) return ZIGMA_ERR_UNSUPPORTED;
    if (!p.state || !p.times || !p.t_out) return ZIGMA_ERR_NULL;
    if (!aligned16(p.state)) return ZIGMA_ERR_STRIDE;
    hipLaunchKernelGGL(sde_advance_kernel, dim3(1), dim3(kSdeThreads), 0, static_cast<hipStream_t>(stream_), p.state, p.times, p.t_out, p.n_rows, p.n_t, p.batch);
    set_last_kernel("sde_advance");
    return check_launch();
}
