// zigma_optim_*: the tail of a training step over many fp32 parameters (include/zigma_hip.h) — global-norm clipping, AdamW, the parameters' moving
// average and their 16-bit shadows.  The device table + chunk map of multi_cast.hip: one row per parameter, one map row per workgroup.  Three launches:
// multi_sumsq_kernel (4 bytes per element read), step_prepare_kernel (one workgroup: norm, skip, step counter, the step's scalars, all on the device, so
// the host never waits) and multi_adamw_kernel (one pass: 20 bytes per element read, 18 written with EMA and shadow).  No atomics anywhere.
// zigma_optim16_* (below): the same three launches for bf16 parameters and gradients — multi_sumsq16_kernel, the SAME step_prepare_kernel, and
// multi_adamw16_kernel, which keeps the moments and the EMA in fp32 and stores the parameter with stochastic rounding (16 bytes read, 14 written).
#include <cmath>

#include "zigma_common.h"

namespace zigma {

constexpr int kOptThreads = 256;
// (the pointers come out of memory, so the compiler cannot see their address space: say that they are global, or every access is a flat one)
typedef float __attribute__((address_space(1))) *gf32_ptr;
typedef const float __attribute__((address_space(1))) *gcf32_ptr;
typedef uint16_t __attribute__((address_space(1))) *gu16_ptr;
typedef v4f __attribute__((address_space(1))) *gv4f_ptr;
typedef const v4f __attribute__((address_space(1))) *gcv4f_ptr;

// the piece of workgroup blockIdx.x: false for a map row outside the table or past the tensor's end (skipped, never followed)
__device__ __forceinline__ bool optim_piece(const zigma_optim_row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map, int64_t n_entries,
                                            int chunk, zigma_optim_row_t &e, int64_t &offset, int &n) {
    const zigma_multi_cast_chunk_t c = chunk_map[blockIdx.x];
    if (c.entry < 0 || c.entry >= n_entries) return false;
    e = table[c.entry];
    if (c.offset < 0 || c.offset >= e.numel) return false;
    const int64_t left = e.numel - c.offset;
    offset = c.offset;
    n = left < chunk ? static_cast<int>(left) : chunk;
    return true;
}

__global__ __launch_bounds__(kOptThreads) void multi_sumsq_kernel(const zigma_optim_row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map,
                                                                  int64_t n_entries, int chunk, float *__restrict__ partials) {
    __shared__ float wave_sum[kOptThreads / kWave];
    zigma_optim_row_t e;
    int64_t offset;
    int n;
    const int tid = threadIdx.x;
    float acc = 0.f;
    if (optim_piece(table, chunk_map, n_entries, chunk, e, offset, n)) {            // (uniform over the workgroup)
        const gcf32_ptr g = (gcf32_ptr)(e.g + offset);
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const int n8 = n & ~7;
            for (int i = tid * 8; i < n8; i += kOptThreads * 8) {
                const v4f a = *(gcv4f_ptr)(g + i);
                const v4f b = *(gcv4f_ptr)(g + i + 4);
                acc += a.x * a.x;
                acc += a.y * a.y;
                acc += a.z * a.z;
                acc += a.w * a.w;
                acc += b.x * b.x;
                acc += b.y * b.y;
                acc += b.z * b.z;
                acc += b.w * b.w;
            }
            done = n8;
        }
        for (int i = done + tid; i < n; i += kOptThreads) acc += g[i] * g[i];
    }
    // fixed order: the wave by halving distances, then the four waves in order
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    if ((tid & (kWave - 1)) == 0) wave_sum[tid / kWave] = acc;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];       // (0 for a skipped map row)
}

__global__ __launch_bounds__(kOptThreads) void step_prepare_kernel(const float *__restrict__ partials, int64_t n_chunks, zigma_optim_state_t *__restrict__ state,
                                                                   const float *__restrict__ grad_scale, const float *__restrict__ found_inf, double lr,
                                                                   double beta1, double beta2, double max_grad_norm) {
    __shared__ double red[kOptThreads];
    const int tid = threadIdx.x;
    double s = 0.0;
    if (partials)
        for (int64_t i = tid; i < n_chunks; i += kOptThreads) s += static_cast<double>(partials[i]);
    red[tid] = s;
    __syncthreads();
    for (int off = kOptThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid != 0) return;
    const double scale = grad_scale ? static_cast<double>(*grad_scale) : 1.0;
    const double norm = partials ? sqrt(red[0]) / scale : 0.0;
    const bool skip = (found_inf && *found_inf != 0.f) || !isfinite(norm);
    zigma_optim_state_t st = *state;
    st.skipped = skip ? 1 : 0;
    st.grad_norm = partials ? static_cast<float>(norm) : __builtin_nanf("");
    if (skip) {
        st.grad_mult = 0.f;
        st.step_size = 0.f;
        st.bc2_sqrt = 1.f;
    } else {
        st.step += 1.f;
        const double step = static_cast<double>(st.step);
        const double clip = (partials && max_grad_norm > 0.0) ? fmin(1.0, max_grad_norm / (norm + 1e-6)) : 1.0;
        st.grad_mult = static_cast<float>(clip / scale);
        st.step_size = static_cast<float>(lr / (1.0 - pow(beta1, step)));
        st.bc2_sqrt = static_cast<float>(sqrt(1.0 - pow(beta2, step)));
    }
    *state = st;
}

struct AdamConsts {
    float lr_wd, one_minus_beta1, beta2, one_minus_beta2, eps, one_minus_decay;
};

__device__ __forceinline__ void adamw_element(float &p, float g, float &m, float &v, const AdamConsts &c, float grad_mult, float step_size, float bc2_sqrt) {
    g = g * grad_mult;
    p = p - __fmul_rn(c.lr_wd, p);                                       // (two roundings, never one fma: the decay alone is reproducible bit for bit)
    m = m + (g - m) * c.one_minus_beta1;
    v = c.beta2 * v + c.one_minus_beta2 * g * g;
    p = p - step_size * m / (sqrtf(v) / bc2_sqrt + c.eps);
}

__device__ __forceinline__ float ema_element(float ema, float p, const AdamConsts &c) { return ema + (p - ema) * c.one_minus_decay; }

// SHADOW = false: no row has a shadow (the column of the table is ignored); T is then unused
template <typename T, bool SHADOW>
__global__ __launch_bounds__(kOptThreads) void multi_adamw_kernel(const zigma_optim_row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map,
                                                                  int64_t n_entries, int chunk, const zigma_optim_state_t *__restrict__ state, AdamConsts c) {
    const zigma_optim_state_t st = *state;
    if (st.skipped) return;                                              // before any store: a skipped step changes nothing
    zigma_optim_row_t e;
    int64_t offset;
    int n;
    if (!optim_piece(table, chunk_map, n_entries, chunk, e, offset, n)) return;
    const gf32_ptr p = (gf32_ptr)(e.p + offset);
    const gcf32_ptr g = (gcf32_ptr)(e.g + offset);
    const gf32_ptr m = (gf32_ptr)(e.m + offset);
    const gf32_ptr v = (gf32_ptr)(e.v + offset);
    const bool has_ema = e.ema != nullptr;
    const bool has_shadow = SHADOW && e.shadow != nullptr;
    const gf32_ptr ema = (gf32_ptr)(has_ema ? e.ema + offset : nullptr);
    const gu16_ptr shadow = (gu16_ptr)(has_shadow ? static_cast<uint16_t *>(e.shadow) + offset : nullptr);
    const float grad_mult = st.grad_mult, step_size = st.step_size, bc2_sqrt = st.bc2_sqrt;
    const int tid = threadIdx.x;
    // uniform over the workgroup: every present stream of the piece starts on a 16-byte boundary -> 8 elements per lane and iteration
    const uintptr_t low = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                          reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(shadow);
    int done = 0;
    if ((low & 15) == 0) {
        const int n8 = n & ~7;
        for (int i = tid * 8; i < n8; i += kOptThreads * 8) {
            v4f pv[2] = {*(gcv4f_ptr)(p + i), *(gcv4f_ptr)(p + i + 4)};
            const v4f gv[2] = {*(gcv4f_ptr)(g + i), *(gcv4f_ptr)(g + i + 4)};
            v4f mv[2] = {*(gcv4f_ptr)(m + i), *(gcv4f_ptr)(m + i + 4)};
            v4f vv[2] = {*(gcv4f_ptr)(v + i), *(gcv4f_ptr)(v + i + 4)};
            v4f ev[2] = {};
            if (has_ema) {
                ev[0] = *(gcv4f_ptr)(ema + i);
                ev[1] = *(gcv4f_ptr)(ema + i + 4);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pe = pv[h][j], me = mv[h][j], ve = vv[h][j];
                    adamw_element(pe, gv[h][j], me, ve, c, grad_mult, step_size, bc2_sqrt);
                    pv[h][j] = pe;
                    mv[h][j] = me;
                    vv[h][j] = ve;
                    ev[h][j] = ema_element(ev[h][j], pe, c);
                }
            *(gv4f_ptr)(p + i) = pv[0];
            *(gv4f_ptr)(p + i + 4) = pv[1];
            *(gv4f_ptr)(m + i) = mv[0];
            *(gv4f_ptr)(m + i + 4) = mv[1];
            *(gv4f_ptr)(v + i) = vv[0];
            *(gv4f_ptr)(v + i + 4) = vv[1];
            if (has_ema) {
                *(gv4f_ptr)(ema + i) = ev[0];
                *(gv4f_ptr)(ema + i + 4) = ev[1];
            }
            if constexpr (SHADOW) {
                if (has_shadow) {
                    u32x4 o;
                    o.x = pack2_pk<T>(pv[0].x, pv[0].y);
                    o.y = pack2_pk<T>(pv[0].z, pv[0].w);
                    o.z = pack2_pk<T>(pv[1].x, pv[1].y);
                    o.w = pack2_pk<T>(pv[1].z, pv[1].w);
                    *(u32x4 __attribute__((address_space(1))) *)(shadow + i) = o;
                }
            }
        }
        done = n8;
    }
    for (int i = done + tid; i < n; i += kOptThreads) {                  // unaligned pieces, and a tensor's last numel % 8
        float pe = p[i], me = m[i], ve = v[i];
        adamw_element(pe, g[i], me, ve, c, grad_mult, step_size, bc2_sqrt);
        p[i] = pe;
        m[i] = me;
        v[i] = ve;
        if (has_ema) ema[i] = ema_element(ema[i], pe, c);
        if constexpr (SHADOW) {
            if (has_shadow) shadow[i] = from_float<T>(pe);
        }
    }
}

enum { kOptSumsq, kOptPrepare, kOptAdamw };

// the refusals of all three entry points, in the header's order; 1: nothing to launch
static int optim_check(const zigma_optim_params_t &p, int which) {
    if (p.n_entries < 0 || p.n_chunks < 0 || p.n_chunks > 0x7fffffffLL) return ZIGMA_ERR_SHAPE;
    if (p.shadow_dtype != ZIGMA_BF16 && p.shadow_dtype != ZIGMA_F16 && p.shadow_dtype != -1) return ZIGMA_ERR_DTYPE;
    if (p.flags != 0) return ZIGMA_ERR_UNSUPPORTED;
    if (p.n_entries == 0 || p.n_chunks == 0) return 1;
    if (which == kOptPrepare ? !p.state : (!p.table || !p.chunk_map || !(which == kOptSumsq ? static_cast<const void *>(p.partials) : static_cast<const void *>(p.state))))
        return ZIGMA_ERR_NULL;
    if (p.chunk < 8 || p.chunk > 65536 || p.chunk % 8 != 0) return ZIGMA_ERR_SHAPE;
    if (!(p.beta1 >= 0.0 && p.beta1 < 1.0) || !(p.beta2 >= 0.0 && p.beta2 < 1.0)) return ZIGMA_ERR_UNSUPPORTED;
    if (!(p.eps > 0.0) || !std::isfinite(p.eps)) return ZIGMA_ERR_UNSUPPORTED;
    if (!std::isfinite(p.lr) || !std::isfinite(p.weight_decay) || !std::isfinite(p.max_grad_norm) || !std::isfinite(p.ema_decay)) return ZIGMA_ERR_UNSUPPORTED;
    return ZIGMA_OK;
}

// ---- zigma_optim16_*: bf16 parameters and gradients, fp32 moments and EMA, the parameter stored with stochastic rounding ------------------------------
typedef const uint16_t __attribute__((address_space(1))) *gcu16_ptr;
typedef u32x4 __attribute__((address_space(1))) *gu32x4_ptr;
typedef const u32x4 __attribute__((address_space(1))) *gcu32x4_ptr;

// the piece of workgroup blockIdx.x: false for a map row outside the table, off the octet grid or past the tensor's end, and for every piece of a
// table row the header refuses (a NULL required stream, numel above max_numel) — skipped, never followed
__device__ __forceinline__ bool optim16_piece(const zigma_optim16_row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map, int64_t n_entries,
                                              int chunk, int64_t max_numel, zigma_optim16_row_t &e, int64_t &offset, int &n) {
    const zigma_multi_cast_chunk_t c = chunk_map[blockIdx.x];
    if (c.entry < 0 || c.entry >= n_entries) return false;
    e = table[c.entry];
    if (e.numel > max_numel || !e.p || !e.g || !e.m || !e.v) return false;
    if (c.offset < 0 || c.offset >= e.numel || (c.offset & 7) != 0) return false;
    const int64_t left = e.numel - c.offset;
    offset = c.offset;
    n = left < chunk ? static_cast<int>(left) : chunk;
    return true;
}

__global__ __launch_bounds__(kOptThreads) void multi_sumsq16_kernel(const zigma_optim16_row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map,
                                                                    int64_t n_entries, int chunk, int64_t max_numel, float *__restrict__ partials) {
    __shared__ float wave_sum[kOptThreads / kWave];
    zigma_optim16_row_t e;
    int64_t offset;
    int n;
    const int tid = threadIdx.x;
    float acc = 0.f;
    if (optim16_piece(table, chunk_map, n_entries, chunk, max_numel, e, offset, n)) {            // (uniform over the workgroup)
        const gcu16_ptr g = (gcu16_ptr)(static_cast<const uint16_t *>(e.g) + offset);
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const int n8 = n & ~7;
            for (int i = tid * 8; i < n8; i += kOptThreads * 8) {
                const u32x4 w = *(gcu32x4_ptr)(g + i);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float a = lo16<BF16>(w[h]), b = hi16<BF16>(w[h]);
                    acc += a * a;
                    acc += b * b;
                }
            }
            done = n8;
        }
        for (int i = done + tid; i < n; i += kOptThreads) {
            const float a = to_float<BF16>(g[i]);
            acc += a * a;
        }
    }
    // fixed order: the wave by halving distances, then the four waves in order
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    if ((tid & (kWave - 1)) == 0) wave_sum[tid / kWave] = acc;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];       // (0 for a skipped map row)
}

// the header's rounding: sign-magnitude add of 16 random bits, then truncation; inf and NaN by from_float
__device__ __forceinline__ uint32_t sr_bf16(float x, uint32_t r16) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) return from_float<BF16>(x);
    return (u + r16) >> 16;
}

// SR = false: ZIGMA_OPTIM16_NEAREST, no Philox work
template <bool SR>
__global__ __launch_bounds__(kOptThreads) void multi_adamw16_kernel(const zigma_optim16_row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map,
                                                                    int64_t n_entries, int chunk, int64_t max_numel, const zigma_optim_state_t *__restrict__ state,
                                                                    AdamConsts c, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream) {
    const zigma_optim_state_t st = *state;
    if (st.skipped) return;                                              // before any store: a skipped step changes nothing
    zigma_optim16_row_t e;
    int64_t offset;
    int n;
    if (!optim16_piece(table, chunk_map, n_entries, chunk, max_numel, e, offset, n)) return;
    const gu16_ptr p = (gu16_ptr)(static_cast<uint16_t *>(e.p) + offset);
    const gcu16_ptr g = (gcu16_ptr)(static_cast<const uint16_t *>(e.g) + offset);
    const gf32_ptr m = (gf32_ptr)(e.m + offset);
    const gf32_ptr v = (gf32_ptr)(e.v + offset);
    const bool has_ema = e.ema != nullptr;
    const gf32_ptr ema = (gf32_ptr)(has_ema ? e.ema + offset : nullptr);
    const gf32_ptr dbg_x = (gf32_ptr)(e.dbg_x32 ? e.dbg_x32 + offset : nullptr);
    const gu16_ptr dbg_b = (gu16_ptr)(SR && e.dbg_bits ? e.dbg_bits + offset : nullptr);
    const float grad_mult = st.grad_mult, step_size = st.step_size, bc2_sqrt = st.bc2_sqrt;
    const uint32_t step = static_cast<uint32_t>(st.step), pid = static_cast<uint32_t>(e.pid);
    const uint32_t oct0 = static_cast<uint32_t>(offset >> 3);            // (offset is a multiple of 8 and numel < 2^35)
    const int tid = threadIdx.x;
    // uniform over the workgroup: every present stream of the piece starts on a 16-byte boundary -> 8 elements per lane and iteration
    const uintptr_t low = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                          reinterpret_cast<uintptr_t>(ema);
    int done = 0;
    if ((low & 15) == 0) {
        const int n8 = n & ~7;
        for (int i = tid * 8; i < n8; i += kOptThreads * 8) {
            const u32x4 pw = *(gcu32x4_ptr)(p + i);
            const u32x4 gw = *(gcu32x4_ptr)(g + i);
            v4f mv[2] = {*(gcv4f_ptr)(m + i), *(gcv4f_ptr)(m + i + 4)};
            v4f vv[2] = {*(gcv4f_ptr)(v + i), *(gcv4f_ptr)(v + i + 4)};
            v4f ev[2] = {};
            if (has_ema) {
                ev[0] = *(gcv4f_ptr)(ema + i);
                ev[1] = *(gcv4f_ptr)(ema + i + 4);
            }
            u32x4 w = {0u, 0u, 0u, 0u};
            if constexpr (SR) w = philox4x32_10(u32x4{oct0 + static_cast<uint32_t>(i >> 3), pid, step, stream}, seed_lo, seed_hi);      // one call for the lane's octet
            u32x4 o;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                uint32_t q[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int j = 2 * h + s;
                    float pe = s ? hi16<BF16>(pw[h]) : lo16<BF16>(pw[h]);
                    const float ge = s ? hi16<BF16>(gw[h]) : lo16<BF16>(gw[h]);
                    float me = mv[j >> 2][j & 3], ve = vv[j >> 2][j & 3];
                    adamw_element(pe, ge, me, ve, c, grad_mult, step_size, bc2_sqrt);
                    mv[j >> 2][j & 3] = me;
                    vv[j >> 2][j & 3] = ve;
                    ev[j >> 2][j & 3] = ema_element(ev[j >> 2][j & 3], pe, c);
                    const uint32_t r = (w[h] >> (16 * s)) & 0xffffu;
                    q[s] = SR ? sr_bf16(pe, r) : static_cast<uint32_t>(from_float<BF16>(pe));
                    if (dbg_x) dbg_x[i + j] = pe;
                    if constexpr (SR) {
                        if (dbg_b) dbg_b[i + j] = static_cast<uint16_t>(r);
                    }
                }
                o[h] = q[0] | (q[1] << 16);
            }
            *(gu32x4_ptr)(p + i) = o;
            *(gv4f_ptr)(m + i) = mv[0];
            *(gv4f_ptr)(m + i + 4) = mv[1];
            *(gv4f_ptr)(v + i) = vv[0];
            *(gv4f_ptr)(v + i + 4) = vv[1];
            if (has_ema) {
                *(gv4f_ptr)(ema + i) = ev[0];
                *(gv4f_ptr)(ema + i + 4) = ev[1];
            }
        }
        done = n8;
    }
    for (int i = done + tid; i < n; i += kOptThreads) {                  // unaligned pieces, and a tensor's last numel % 8: the element's own octet and half-word
        float pe = to_float<BF16>(p[i]), me = m[i], ve = v[i];
        adamw_element(pe, to_float<BF16>(g[i]), me, ve, c, grad_mult, step_size, bc2_sqrt);
        m[i] = me;
        v[i] = ve;
        if (has_ema) ema[i] = ema_element(ema[i], pe, c);
        if (dbg_x) dbg_x[i] = pe;
        if constexpr (SR) {
            const u32x4 w = philox4x32_10(u32x4{oct0 + static_cast<uint32_t>(i >> 3), pid, step, stream}, seed_lo, seed_hi);
            const int j = i & 7;
            const uint32_t lo = (j & 2) ? w.y : w.x, hi = (j & 2) ? w.w : w.z;
            const uint32_t r = (((j & 4) ? hi : lo) >> (16 * (j & 1))) & 0xffffu;
            if (dbg_b) dbg_b[i] = static_cast<uint16_t>(r);
            p[i] = static_cast<uint16_t>(sr_bf16(pe, r));
        } else {
            p[i] = from_float<BF16>(pe);
        }
    }
}

// the refusals of both entry points, in the header's order; 1: nothing to launch
static int optim16_check(const zigma_optim16_params_t &p, bool sumsq) {
    if (!p.table || !p.chunk_map || !(sumsq ? static_cast<const void *>(p.partials) : static_cast<const void *>(p.state))) return ZIGMA_ERR_NULL;
    if (p.n_entries < 0 || p.n_chunks < 0 || p.n_chunks > 0x7fffffffLL) return ZIGMA_ERR_SHAPE;
    if (p.max_numel < 0 || p.max_numel >= (1LL << 35)) return ZIGMA_ERR_SHAPE;
    if (p.chunk < 8 || p.chunk > 65536 || p.chunk % 8 != 0) return ZIGMA_ERR_SHAPE;
    if (p.flags & ~ZIGMA_OPTIM16_NEAREST) return ZIGMA_ERR_UNSUPPORTED;
    if (!(p.beta1 >= 0.0 && p.beta1 < 1.0) || !(p.beta2 >= 0.0 && p.beta2 < 1.0)) return ZIGMA_ERR_UNSUPPORTED;
    if (!(p.eps > 0.0) || !std::isfinite(p.eps)) return ZIGMA_ERR_UNSUPPORTED;
    if (!std::isfinite(p.lr) || !std::isfinite(p.weight_decay) || !std::isfinite(p.max_grad_norm) || !std::isfinite(p.ema_decay)) return ZIGMA_ERR_UNSUPPORTED;
    if (p.n_entries == 0 || p.n_chunks == 0) return 1;
    return ZIGMA_OK;
}

}  // namespace zigma

using namespace zigma;

extern "C" int zigma_optim16_grad_sumsq(const zigma_optim16_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_optim16_params_t &p = *pp;
    const int rc = optim16_check(p, true);
    if (rc != ZIGMA_OK) return rc == 1 ? ZIGMA_OK : rc;
    hipLaunchKernelGGL(multi_sumsq16_kernel, dim3(static_cast<unsigned>(p.n_chunks)), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream_), p.table, p.chunk_map,
                       p.n_entries, p.chunk, p.max_numel, p.partials);
    set_last_kernel("multi_sumsq16");
    return check_launch();
}

extern "C" int zigma_optim16_adamw(const zigma_optim16_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_optim16_params_t &p = *pp;
    const int rc = optim16_check(p, false);
    if (rc != ZIGMA_OK) return rc == 1 ? ZIGMA_OK : rc;
    const AdamConsts c = {static_cast<float>(p.lr * p.weight_decay), static_cast<float>(1.0 - p.beta1), static_cast<float>(p.beta2), static_cast<float>(1.0 - p.beta2),
                          static_cast<float>(p.eps), static_cast<float>(1.0 - p.ema_decay)};
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>(p.n_chunks));
    const zigma_optim_state_t *state = p.state;
    if (p.flags & ZIGMA_OPTIM16_NEAREST) {
        hipLaunchKernelGGL((multi_adamw16_kernel<false>), grid, dim3(kOptThreads), 0, stream, p.table, p.chunk_map, p.n_entries, p.chunk, p.max_numel, state, c, p.seed_lo,
                           p.seed_hi, p.stream);
        set_last_kernel("multi_adamw16_nearest");
    } else {
        hipLaunchKernelGGL((multi_adamw16_kernel<true>), grid, dim3(kOptThreads), 0, stream, p.table, p.chunk_map, p.n_entries, p.chunk, p.max_numel, state, c, p.seed_lo,
                           p.seed_hi, p.stream);
        set_last_kernel("multi_adamw16_sr");
    }
    return check_launch();
}

extern "C" int zigma_optim_grad_sumsq(const zigma_optim_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_optim_params_t &p = *pp;
    const int rc = optim_check(p, kOptSumsq);
    if (rc != ZIGMA_OK) return rc == 1 ? ZIGMA_OK : rc;
    hipLaunchKernelGGL(multi_sumsq_kernel, dim3(static_cast<unsigned>(p.n_chunks)), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream_), p.table, p.chunk_map,
                       p.n_entries, p.chunk, p.partials);
    set_last_kernel("multi_sumsq");
    return check_launch();
}

extern "C" int zigma_optim_prepare(const zigma_optim_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_optim_params_t &p = *pp;
    const int rc = optim_check(p, kOptPrepare);
    if (rc != ZIGMA_OK) return rc == 1 ? ZIGMA_OK : rc;
    hipLaunchKernelGGL(step_prepare_kernel, dim3(1), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream_), static_cast<const float *>(p.partials), p.n_chunks,
                       p.state, p.grad_scale, p.found_inf, p.lr, p.beta1, p.beta2, p.max_grad_norm);
    set_last_kernel("step_prepare");
    return check_launch();
}

extern "C" int zigma_optim_adamw(const zigma_optim_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_optim_params_t &p = *pp;
    const int rc = optim_check(p, kOptAdamw);
    if (rc != ZIGMA_OK) return rc == 1 ? ZIGMA_OK : rc;
    const AdamConsts c = {static_cast<float>(p.lr * p.weight_decay), static_cast<float>(1.0 - p.beta1), static_cast<float>(p.beta2), static_cast<float>(1.0 - p.beta2),
                          static_cast<float>(p.eps), static_cast<float>(1.0 - p.ema_decay)};
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>(p.n_chunks));
    const zigma_optim_state_t *state = p.state;
    if (p.shadow_dtype == -1) {
        hipLaunchKernelGGL((multi_adamw_kernel<BF16, false>), grid, dim3(kOptThreads), 0, stream, p.table, p.chunk_map, p.n_entries, p.chunk, state, c);
        set_last_kernel("multi_adamw");
    } else {
        ZIGMA_DISPATCH_16BIT(p.shadow_dtype, T,
                             hipLaunchKernelGGL((multi_adamw_kernel<T, true>), grid, dim3(kOptThreads), 0, stream, p.table, p.chunk_map, p.n_entries, p.chunk, state, c));
        set_last_kernel(p.shadow_dtype == ZIGMA_BF16 ? "multi_adamw_bf16" : "multi_adamw_f16");
    }
    return check_launch();
}
