// zigma_optim_* and zigma_optim16_*: the tail of a training step over many parameters (include/zigma_hip.h) — global-norm clipping, AdamW, the
// parameters' moving average, and either the 16-bit shadows of fp32 parameters or the stochastic rounding of bf16 ones.  The device table + chunk map of
// multi_cast.hip: one row per parameter, one map row per workgroup (piece, below).  Three launches, no atomics anywhere:
//   multi_sumsq_kernel<Row>    the gradients' squares, 4 (fp32) or 2 (bf16) bytes per element read
//   step_prepare_kernel        one workgroup: norm, skip, step counter, the step's scalars, all on the device, so the host never waits
//   multi_adamw_kernel<Store>  one pass; the arithmetic and the fp32 m / v / ema streams are written once, a Store says where the parameter lives:
//                              StoreF32<T, SHADOW> (20 bytes per element read, 18 written with EMA and shadow) or StoreBf16<SR> (16 read, 14 written)
#include <cmath>

#include "zigma_common.h"

namespace zigma {

constexpr int kOptThreads = 256;
// (the pointers come out of memory, so the compiler cannot see their address space: say that they are global, or every access is a flat one)
typedef float __attribute__((address_space(1))) *gf32_ptr;
typedef const float __attribute__((address_space(1))) *gcf32_ptr;
typedef uint16_t __attribute__((address_space(1))) *gu16_ptr;
typedef const uint16_t __attribute__((address_space(1))) *gcu16_ptr;
typedef v4f __attribute__((address_space(1))) *gv4f_ptr;
typedef const v4f __attribute__((address_space(1))) *gcv4f_ptr;
typedef u32x4 __attribute__((address_space(1))) *gu32x4_ptr;
typedef const u32x4 __attribute__((address_space(1))) *gcu32x4_ptr;

// what the 16-bit step's rows add to the walk's refusals (include/zigma_hip.h): a NULL required stream, numel above max_numel, an offset off the octet grid
__device__ __forceinline__ bool row_ok(const zigma_optim_row_t &, int64_t, int64_t) { return true; }
__device__ __forceinline__ bool row_ok(const zigma_optim16_row_t &e, int64_t offset, int64_t max_numel) {
    return e.numel <= max_numel && e.p && e.g && e.m && e.v && (offset & 7) == 0;
}

// the piece of workgroup blockIdx.x: false for a map row outside the table or past the tensor's end and for one its row refuses (skipped, never followed).
// (multi_cast.hip keeps its own copy of this walk: calling this one there changes its register allocation, and its device code is to stay as it is)
template <typename Row>
__device__ __forceinline__ bool piece(const Row *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map, int64_t n_entries, int chunk,
                                      int64_t max_numel, Row &e, int64_t &offset, int &n) {
    const zigma_multi_cast_chunk_t c = chunk_map[blockIdx.x];
    if (c.entry < 0 || c.entry >= n_entries) return false;
    e = table[c.entry];
    if (c.offset < 0 || c.offset >= e.numel || !row_ok(e, c.offset, max_numel)) return false;
    const int64_t left = e.numel - c.offset;
    offset = c.offset;
    n = left < chunk ? static_cast<int>(left) : chunk;
    return true;
}

// the gradient stream of a row's piece
__device__ __forceinline__ gcf32_ptr grad_of(const zigma_optim_row_t &e, int64_t offset) { return (gcf32_ptr)(e.g + offset); }
__device__ __forceinline__ gcu16_ptr grad_of(const zigma_optim16_row_t &e, int64_t offset) { return (gcu16_ptr)(static_cast<const uint16_t *>(e.g) + offset); }

// eight elements from a 16-byte boundary, or one element, as float: fp32, or bf16 widened (exact)
__device__ __forceinline__ void load8(gcf32_ptr s, float (&x)[8]) {
    const v4f a = *(gcv4f_ptr)s, b = *(gcv4f_ptr)(s + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = a[j];
        x[4 + j] = b[j];
    }
}
__device__ __forceinline__ void load8(gcu16_ptr s, float (&x)[8]) {
    const u32x4 w = *(gcu32x4_ptr)s;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        x[2 * h] = lo16<BF16>(w[h]);
        x[2 * h + 1] = hi16<BF16>(w[h]);
    }
}
__device__ __forceinline__ float load1(gcf32_ptr s) { return *s; }
__device__ __forceinline__ float load1(gcu16_ptr s) { return to_float<BF16>(*s); }
__device__ __forceinline__ void store8(gf32_ptr d, const float (&x)[8]) {
    *(gv4f_ptr)d = v4f{x[0], x[1], x[2], x[3]};
    *(gv4f_ptr)(d + 4) = v4f{x[4], x[5], x[6], x[7]};
}

template <typename Row>
__global__ __launch_bounds__(kOptThreads) void multi_sumsq_kernel(const Row *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map,
                                                                  int64_t n_entries, int chunk, int64_t max_numel, float *__restrict__ partials) {
    __shared__ float wave_sum[kOptThreads / kWave];
    Row e;
    int64_t offset;
    int n;
    const int tid = threadIdx.x;
    float acc = 0.f;
    if (piece(table, chunk_map, n_entries, chunk, max_numel, e, offset, n)) {       // (uniform over the workgroup)
        const auto g = grad_of(e, offset);
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const int n8 = n & ~7;
            for (int i = tid * 8; i < n8; i += kOptThreads * 8) {
                float x[8];
                load8(g + i, x);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc += x[j] * x[j];
            }
            done = n8;
        }
        for (int i = done + tid; i < n; i += kOptThreads) {
            const float a = load1(g + i);
            acc += a * a;
        }
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

// ---- where the parameter of a piece lives: `p` to load it from, low() for the alignment rule, store8 / store1 for the new fp32 values ------------------
// fp32 parameters, written as they are, plus their 16-bit shadow (the bits of the cast kernel).  SHADOW = false: no row has one (the column of the table
// is ignored); T is then unused
template <typename T, bool SHADOW>
struct StoreF32 {
    typedef zigma_optim_row_t row_t;
    struct arg_t {};
    gf32_ptr p;
    gu16_ptr shadow;
    __device__ __forceinline__ StoreF32(const row_t &e, int64_t offset, const zigma_optim_state_t &, arg_t)
        : p((gf32_ptr)(e.p + offset)), shadow((gu16_ptr)(SHADOW && e.shadow ? static_cast<uint16_t *>(e.shadow) + offset : nullptr)) {}
    __device__ __forceinline__ uintptr_t low() const { return reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(shadow); }
    __device__ __forceinline__ void store8(int i, const float (&x)[8]) const {
        zigma::store8(p + i, x);
        if constexpr (SHADOW) {
            if (shadow) *(gu32x4_ptr)(shadow + i) = u32x4{pack2_pk<T>(x[0], x[1]), pack2_pk<T>(x[2], x[3]), pack2_pk<T>(x[4], x[5]), pack2_pk<T>(x[6], x[7])};
        }
    }
    __device__ __forceinline__ void store1(int i, float x) const {
        p[i] = x;
        if constexpr (SHADOW) {
            if (shadow) shadow[i] = from_float<T>(x);
        }
    }
};

// the header's rounding: sign-magnitude add of 16 random bits, then truncation; inf and NaN by from_float
__device__ __forceinline__ uint32_t sr_bf16(float x, uint32_t r16) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) return from_float<BF16>(x);
    return (u + r16) >> 16;
}

// bf16 parameters, rounded stochastically with the bits of the element's octet (one Philox call per octet), or, SR = false (ZIGMA_OPTIM16_NEAREST), to
// nearest with no Philox work; the two debug streams receive the fp32 value and the bits
template <bool SR>
struct StoreBf16 {
    typedef zigma_optim16_row_t row_t;
    struct arg_t {
        uint32_t seed_lo, seed_hi, stream;
    };
    gu16_ptr p, dbg_b;
    gf32_ptr dbg_x;
    uint32_t oct0, pid, step;
    arg_t key;
    __device__ __forceinline__ StoreBf16(const row_t &e, int64_t offset, const zigma_optim_state_t &st, arg_t key_)
        : p((gu16_ptr)(static_cast<uint16_t *>(e.p) + offset)), dbg_b((gu16_ptr)(SR && e.dbg_bits ? e.dbg_bits + offset : nullptr)),
          dbg_x((gf32_ptr)(e.dbg_x32 ? e.dbg_x32 + offset : nullptr)), oct0(static_cast<uint32_t>(offset >> 3)),       // (offset is a multiple of 8 and numel < 2^35)
          pid(static_cast<uint32_t>(e.pid)), step(static_cast<uint32_t>(st.step)), key(key_) {}
    __device__ __forceinline__ uintptr_t low() const { return reinterpret_cast<uintptr_t>(p); }
    __device__ __forceinline__ u32x4 octet_bits(int i) const {
        return philox4x32_10(u32x4{oct0 + static_cast<uint32_t>(i >> 3), pid, step, key.stream}, key.seed_lo, key.seed_hi);
    }
    __device__ __forceinline__ void store8(int i, const float (&x)[8]) const {
        u32x4 w = {0u, 0u, 0u, 0u}, o;
        if constexpr (SR) w = octet_bits(i);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            uint32_t q[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = 2 * h + s;
                const uint32_t r = (w[h] >> (16 * s)) & 0xffffu;
                q[s] = SR ? sr_bf16(x[j], r) : static_cast<uint32_t>(from_float<BF16>(x[j]));
                if (dbg_x) dbg_x[i + j] = x[j];
                if constexpr (SR) {
                    if (dbg_b) dbg_b[i + j] = static_cast<uint16_t>(r);
                }
            }
            o[h] = q[0] | (q[1] << 16);
        }
        *(gu32x4_ptr)(p + i) = o;
    }
    __device__ __forceinline__ void store1(int i, float x) const {     // the element's own octet and half-word
        if (dbg_x) dbg_x[i] = x;
        if constexpr (SR) {
            const u32x4 w = octet_bits(i);
            const int j = i & 7;
            const uint32_t lo = (j & 2) ? w.y : w.x, hi = (j & 2) ? w.w : w.z;
            const uint32_t r = (((j & 4) ? hi : lo) >> (16 * (j & 1))) & 0xffffu;
            if (dbg_b) dbg_b[i] = static_cast<uint16_t>(r);
            p[i] = static_cast<uint16_t>(sr_bf16(x, r));
        } else {
            p[i] = from_float<BF16>(x);
        }
    }
};

template <typename Store>
__global__ __launch_bounds__(kOptThreads) void multi_adamw_kernel(const typename Store::row_t *__restrict__ table, const zigma_multi_cast_chunk_t *__restrict__ chunk_map,
                                                                  int64_t n_entries, int chunk, int64_t max_numel, const zigma_optim_state_t *__restrict__ state,
                                                                  AdamConsts c, typename Store::arg_t arg) {
    const zigma_optim_state_t st = *state;
    if (st.skipped) return;                                              // before any store: a skipped step changes nothing
    typename Store::row_t e;
    int64_t offset;
    int n;
    if (!piece(table, chunk_map, n_entries, chunk, max_numel, e, offset, n)) return;
    const Store out(e, offset, st, arg);
    const auto g = grad_of(e, offset);
    const gf32_ptr m = (gf32_ptr)(e.m + offset);
    const gf32_ptr v = (gf32_ptr)(e.v + offset);
    const bool has_ema = e.ema != nullptr;
    const gf32_ptr ema = (gf32_ptr)(has_ema ? e.ema + offset : nullptr);
    const float grad_mult = st.grad_mult, step_size = st.step_size, bc2_sqrt = st.bc2_sqrt;
    const int tid = threadIdx.x;
    // uniform over the workgroup: every present stream of the piece starts on a 16-byte boundary -> 8 elements per lane and iteration
    const uintptr_t low = out.low() | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(ema);
    int done = 0;
    if ((low & 15) == 0) {
        const int n8 = n & ~7;
        for (int i = tid * 8; i < n8; i += kOptThreads * 8) {
            float px[8], gx[8], mx[8], vx[8], ex[8] = {};
            load8(out.p + i, px);
            load8(g + i, gx);
            load8(m + i, mx);
            load8(v + i, vx);
            if (has_ema) load8(ema + i, ex);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                adamw_element(px[j], gx[j], mx[j], vx[j], c, grad_mult, step_size, bc2_sqrt);
                ex[j] = ema_element(ex[j], px[j], c);
            }
            out.store8(i, px);
            store8(m + i, mx);
            store8(v + i, vx);
            if (has_ema) store8(ema + i, ex);
        }
        done = n8;
    }
    for (int i = done + tid; i < n; i += kOptThreads) {                  // unaligned pieces, and a tensor's last numel % 8
        float pe = load1(out.p + i), me = m[i], ve = v[i];
        adamw_element(pe, load1(g + i), me, ve, c, grad_mult, step_size, bc2_sqrt);
        m[i] = me;
        v[i] = ve;
        if (has_ema) ema[i] = ema_element(ema[i], pe, c);
        out.store1(i, pe);
    }
}

// ---- the host half ------------------------------------------------------------------------------------------------------------------------------------
enum { kOptSumsq, kOptPrepare, kOptAdamw };

// the hyperparameter refusals of both blocks (ZIGMA_ERR_UNSUPPORTED, all of them): beta1 or beta2 outside [0, 1), eps <= 0, anything non-finite or NaN
template <typename P> static bool hyper_ok(const P &p) {
    return p.beta1 >= 0.0 && p.beta1 < 1.0 && p.beta2 >= 0.0 && p.beta2 < 1.0 && p.eps > 0.0 && std::isfinite(p.eps) && std::isfinite(p.lr) &&
           std::isfinite(p.weight_decay) && std::isfinite(p.max_grad_norm) && std::isfinite(p.ema_decay);
}
template <typename P> static bool counts_ok(const P &p) { return p.n_entries >= 0 && p.n_chunks >= 0 && p.n_chunks <= 0x7fffffffLL; }
template <typename P> static bool chunk_ok(const P &p) { return p.chunk >= 8 && p.chunk <= 65536 && p.chunk % 8 == 0; }

// the refusals of the three fp32 entry points, in the header's order; 1: nothing to launch
static int optim_check(const zigma_optim_params_t &p, int which) {
    if (!counts_ok(p)) return ZIGMA_ERR_SHAPE;
    if (p.shadow_dtype != ZIGMA_BF16 && p.shadow_dtype != ZIGMA_F16 && p.shadow_dtype != -1) return ZIGMA_ERR_DTYPE;
    if (p.flags != 0) return ZIGMA_ERR_UNSUPPORTED;
    if (p.n_entries == 0 || p.n_chunks == 0) return 1;
    if (which == kOptPrepare ? !p.state : (!p.table || !p.chunk_map || !(which == kOptSumsq ? static_cast<const void *>(p.partials) : static_cast<const void *>(p.state))))
        return ZIGMA_ERR_NULL;
    if (!chunk_ok(p)) return ZIGMA_ERR_SHAPE;
    return hyper_ok(p) ? ZIGMA_OK : ZIGMA_ERR_UNSUPPORTED;
}

// the refusals of the two 16-bit entry points, in the header's order (not the one above); 1: nothing to launch
static int optim_check(const zigma_optim16_params_t &p, int which) {
    if (!p.table || !p.chunk_map || !(which == kOptSumsq ? static_cast<const void *>(p.partials) : static_cast<const void *>(p.state))) return ZIGMA_ERR_NULL;
    if (!counts_ok(p)) return ZIGMA_ERR_SHAPE;
    if (p.max_numel < 0 || p.max_numel >= (1LL << 35)) return ZIGMA_ERR_SHAPE;
    if (!chunk_ok(p)) return ZIGMA_ERR_SHAPE;
    if (p.flags & ~ZIGMA_OPTIM16_NEAREST) return ZIGMA_ERR_UNSUPPORTED;
    if (!hyper_ok(p)) return ZIGMA_ERR_UNSUPPORTED;
    return p.n_entries == 0 || p.n_chunks == 0 ? 1 : ZIGMA_OK;
}

template <typename P> static AdamConsts adam_consts(const P &p) {
    return {static_cast<float>(p.lr * p.weight_decay), static_cast<float>(1.0 - p.beta1), static_cast<float>(p.beta2), static_cast<float>(1.0 - p.beta2),
            static_cast<float>(p.eps), static_cast<float>(1.0 - p.ema_decay)};
}

// every entry point: a NULL block, a clean error state, the block's refusals, then `launch` (which names its kernel) if there is anything to launch
template <typename P, typename Launch> static int optim_entry(const P *pp, int which, Launch launch) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const int rc = optim_check(*pp, which);
    if (rc != ZIGMA_OK) return rc == 1 ? ZIGMA_OK : rc;
    set_last_kernel(launch(*pp));
    return check_launch();
}

template <typename Store, typename P> static void launch_adamw(const P &p, int64_t max_numel, typename Store::arg_t arg, void *stream) {
    hipLaunchKernelGGL(multi_adamw_kernel<Store>, dim3(static_cast<unsigned>(p.n_chunks)), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), p.table, p.chunk_map,
                       p.n_entries, p.chunk, max_numel, static_cast<const zigma_optim_state_t *>(p.state), adam_consts(p), arg);
}

}  // namespace zigma

using namespace zigma;

extern "C" int zigma_optim16_grad_sumsq(const zigma_optim16_params_t *pp, void *stream) {
    return optim_entry(pp, kOptSumsq, [=](const zigma_optim16_params_t &p) {
        hipLaunchKernelGGL(multi_sumsq_kernel<zigma_optim16_row_t>, dim3(static_cast<unsigned>(p.n_chunks)), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), p.table,
                           p.chunk_map, p.n_entries, p.chunk, p.max_numel, p.partials);
        return "multi_sumsq16";
    });
}

extern "C" int zigma_optim16_adamw(const zigma_optim16_params_t *pp, void *stream) {
    return optim_entry(pp, kOptAdamw, [=](const zigma_optim16_params_t &p) {
        const bool nearest = p.flags & ZIGMA_OPTIM16_NEAREST;
        if (nearest) launch_adamw<StoreBf16<false>>(p, p.max_numel, {p.seed_lo, p.seed_hi, p.stream}, stream);
        else launch_adamw<StoreBf16<true>>(p, p.max_numel, {p.seed_lo, p.seed_hi, p.stream}, stream);
        return nearest ? "multi_adamw16_nearest" : "multi_adamw16_sr";
    });
}

extern "C" int zigma_optim_grad_sumsq(const zigma_optim_params_t *pp, void *stream) {
    return optim_entry(pp, kOptSumsq, [=](const zigma_optim_params_t &p) {
        hipLaunchKernelGGL(multi_sumsq_kernel<zigma_optim_row_t>, dim3(static_cast<unsigned>(p.n_chunks)), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), p.table,
                           p.chunk_map, p.n_entries, p.chunk, int64_t{0}, p.partials);
        return "multi_sumsq";
    });
}

extern "C" int zigma_optim_prepare(const zigma_optim_params_t *pp, void *stream) {
    return optim_entry(pp, kOptPrepare, [=](const zigma_optim_params_t &p) {
        hipLaunchKernelGGL(step_prepare_kernel, dim3(1), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), static_cast<const float *>(p.partials), p.n_chunks, p.state,
                           p.grad_scale, p.found_inf, p.lr, p.beta1, p.beta2, p.max_grad_norm);
        return "step_prepare";
    });
}

extern "C" int zigma_optim_adamw(const zigma_optim_params_t *pp, void *stream) {
    return optim_entry(pp, kOptAdamw, [=](const zigma_optim_params_t &p) {
        if (p.shadow_dtype == -1) launch_adamw<StoreF32<BF16, false>>(p, 0, {}, stream);
        else if (p.shadow_dtype == ZIGMA_BF16) launch_adamw<StoreF32<BF16, true>>(p, 0, {}, stream);
        else launch_adamw<StoreF32<F16, true>>(p, 0, {}, stream);
        return p.shadow_dtype == -1 ? "multi_adamw" : p.shadow_dtype == ZIGMA_BF16 ? "multi_adamw_bf16" : "multi_adamw_f16";
    });
}
