// Shared device/host helpers for libzigma_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "zigma_hip.h"

namespace zigma {

constexpr int kWave = 64;

// register vectors (ext vectors: an array of HIP's uint4 / float4 structs would live in memory) and the address spaces the builtins ask for
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // 16 bytes in registers
typedef __attribute__((address_space(3))) unsigned char *lds_ptr_t;
typedef const __attribute__((address_space(1))) void *gbl_ptr_t;

// sum over the LPR lanes that share a row (LPR = 64: the whole wave)
template <int LPR> __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = LPR / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator of the SDE step's
// noise (sde_step.hip) and of the 16-bit optimizer's stochastic rounding (optim_step.hip)
__device__ __forceinline__ u32x4 philox4x32_10(u32x4 ctr, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * ctr.x;
        const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * ctr.z;
        ctr = u32x4{static_cast<uint32_t>(p1 >> 32) ^ ctr.y ^ k0, static_cast<uint32_t>(p1), static_cast<uint32_t>(p0 >> 32) ^ ctr.w ^ k1, static_cast<uint32_t>(p0)};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ctr;
}

// ---- element types -----------------------------------------------------------------------------
// I/O element wrappers: 16-bit types are carried as raw uint16_t and widened by bit ops (bf16) or
// the hardware converter (f16); arithmetic is always float32.
struct F32 { using raw = float;    static constexpr int id = ZIGMA_F32;  };
struct F16 { using raw = uint16_t; static constexpr int id = ZIGMA_F16;  };
struct BF16 { using raw = uint16_t; static constexpr int id = ZIGMA_BF16; };

template <typename T> __device__ __forceinline__ float to_float(typename T::raw v);
template <> __device__ __forceinline__ float to_float<F32>(float v) { return v; }
template <> __device__ __forceinline__ float to_float<BF16>(uint16_t v) {
    return __uint_as_float(static_cast<uint32_t>(v) << 16);
}
template <> __device__ __forceinline__ float to_float<F16>(uint16_t v) {
    _Float16 h;
    __builtin_memcpy(&h, &v, 2);
    return static_cast<float>(h);
}

template <typename T> __device__ __forceinline__ typename T::raw from_float(float f);
template <> __device__ __forceinline__ float from_float<F32>(float f) { return f; }
template <> __device__ __forceinline__ uint16_t from_float<BF16>(float f) {
    // round-to-nearest-even (same as at::BFloat16); one v_cvt_pk_bf16_f32 on gfx950
    const __bf16 h = static_cast<__bf16>(f);
    uint16_t v;
    __builtin_memcpy(&v, &h, 2);
    return v;
}
template <> __device__ __forceinline__ uint16_t from_float<F16>(float f) {
    _Float16 h = static_cast<_Float16>(f);
    uint16_t v;
    __builtin_memcpy(&v, &h, 2);
    return v;
}

template <typename T> __device__ __forceinline__ float ld(const void *base, int64_t idx) {
    return to_float<T>(reinterpret_cast<const typename T::raw *>(base)[idx]);
}
template <typename T> __device__ __forceinline__ void st(void *base, int64_t idx, float v) {
    reinterpret_cast<typename T::raw *>(base)[idx] = from_float<T>(v);
}

// ---- 16-bit pairs and MFMA fragments by I/O type (the matrix-core kernels serve BF16 and F16) -------
// Two 16-bit values travel in one dword.  bf16 widens by bit ops, f16 by the hardware converter (v_cvt_f32_f16 and its
// WORD_1 form); both narrow with round-to-nearest-even, so every kernel family rounds at the same points to the same bits.
template <typename T> __device__ __forceinline__ float lo16(uint32_t v);
template <typename T> __device__ __forceinline__ float hi16(uint32_t v);
template <> __device__ __forceinline__ float lo16<BF16>(uint32_t v) { return __uint_as_float(v << 16); }
template <> __device__ __forceinline__ float hi16<BF16>(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }
template <> __device__ __forceinline__ float lo16<F16>(uint32_t v) { return to_float<F16>(static_cast<uint16_t>(v & 0xffffu)); }
template <> __device__ __forceinline__ float hi16<F16>(uint32_t v) { return to_float<F16>(static_cast<uint16_t>(v >> 16)); }

template <typename T> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    return static_cast<uint32_t>(from_float<T>(lo)) | (static_cast<uint32_t>(from_float<T>(hi)) << 16);
}
// the same as one packed conversion (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32)
template <typename T> __device__ __forceinline__ uint32_t pack2_pk(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack2_pk<BF16>(float lo, float hi) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v2f{lo, hi}, bf16x2_t));
}
template <> __device__ __forceinline__ uint32_t pack2_pk<F16>(float lo, float hi) {
    typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v2f{lo, hi}, f16x2_t));
}

typedef __bf16 mfma_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 mfma_f16x8 __attribute__((ext_vector_type(8)));
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));
typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Frag8;
template <> struct Frag8<BF16> { typedef mfma_bf16x8 type; };
template <> struct Frag8<F16> { typedef mfma_f16x8 type; };
template <typename T> using frag8_t = typename Frag8<T>::type;      // 8 elements of a row: one 16-byte MFMA operand

// v_mfma_f32_32x32x16_{bf16,f16} / v_mfma_f32_16x16x32_{bf16,f16}: same rate, same operand and accumulator lane maps
template <typename T> __device__ __forceinline__ mfma_f32x16 mfma_32x32x16(frag8_t<T> a, frag8_t<T> b, mfma_f32x16 c);
template <> __device__ __forceinline__ mfma_f32x16 mfma_32x32x16<BF16>(mfma_bf16x8 a, mfma_bf16x8 b, mfma_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ mfma_f32x16 mfma_32x32x16<F16>(mfma_f16x8 a, mfma_f16x8 b, mfma_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
template <typename T> __device__ __forceinline__ mfma_f32x4 mfma_16x16x32(frag8_t<T> a, frag8_t<T> b, mfma_f32x4 c);
template <> __device__ __forceinline__ mfma_f32x4 mfma_16x16x32<BF16>(mfma_bf16x8 a, mfma_bf16x8 b, mfma_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ mfma_f32x4 mfma_16x16x32<F16>(mfma_f16x8 a, mfma_f16x8 b, mfma_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---- math (reference numerics: selective_scan_fwd_kernel.cuh:153-156,216,293) ------------------
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32
__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }    // v_log_f32
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }     // v_rcp_f32

// softplus with pass-through above 20 (reference: x <= 20 ? log1pf(expf(x)) : x).
// log1p(t), t = e^x: short alternating series while t is small (keeps full relative accuracy for
// very negative x, where 1+t would round t away), hardware log2 otherwise.
__device__ __forceinline__ float softplus20(float x) {
    const float t = fast_exp2(fminf(x, 20.f) * kLog2e);
    const float series = t * (1.f + t * (-0.5f + t * 0.33333334f));   // |err| < t^4/4 <= 6e-8 t  for t < 2^-6
    const float big = fast_log2(1.f + t) * kLn2;                       // abs err ~1e-7 on a result >= 0.0155
    const float sp = t < 0.015625f ? series : big;
    return x > 20.f ? x : sp;
}

// The same function for results that are rounded to 16 bits right away (dt_proj's epilogue): softplus(x) = max(x, 0) +
// log1p(exp(-|x|)), 10 instructions instead of 14 (no clamp, no pass-through select: above 20 the log term is below 2e-9
// and vanishes in the rounding, like the reference's pass-through).  t = exp(-|x|) <= 1; below 2^-8 the log1p is the
// two-term series (relative error < 2^-17), above it log2(1 + t) (absolute error 2^-24 on a term >= 2^-8.5).
__device__ __forceinline__ float softplus20_r16(float x) {
    const float t = fast_exp2(-fabsf(x) * kLog2e);
    const float series = __builtin_fmaf(t * -0.5f, t, t);
    const float big = fast_log2(1.f + t) * kLn2;
    return fmaxf(x, 0.f) + (t < 0.00390625f ? series : big);
}

// x * sigmoid(x) written as z / (1 + exp(-z)) like the reference kernel.
__device__ __forceinline__ float silu(float z) { return z * fast_rcp(1.f + fast_exp2(-z * kLog2e)); }

// ---- host side -----------------------------------------------------------------------------------
inline int check_launch() {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return ZIGMA_OK;
    fprintf(stderr, "libzigma_hip: kernel launch failed: %s (%s)\n", hipGetErrorName(e), hipGetErrorString(e));
    return ZIGMA_ERR_LAUNCH;
}
void set_last_kernel(const char *name);

#define ZIGMA_DISPATCH_DTYPE(DT, T, ...)                                   \
    switch (DT) {                                                          \
        case ZIGMA_F32: { using T = ::zigma::F32; __VA_ARGS__; break; }    \
        case ZIGMA_F16: { using T = ::zigma::F16; __VA_ARGS__; break; }    \
        case ZIGMA_BF16: { using T = ::zigma::BF16; __VA_ARGS__; break; }  \
        default: return ZIGMA_ERR_DTYPE;                                   \
    }

// add-norm in both directions: x in any of the three types, the residual stream and the weight in fp32 (RES32 / W32: the slot of csrc/norm_plan.h) or in x's
#define ZIGMA_DISPATCH_NORM_SLOT(DT, RES32, W32, XT, RT, WT, ...)                               \
    ZIGMA_DISPATCH_DTYPE(DT, XT, {                                                                \
        if ((RES32) && (W32)) { using RT = ::zigma::F32; using WT = ::zigma::F32; __VA_ARGS__; } \
        else if (RES32) { using RT = ::zigma::F32; using WT = XT; __VA_ARGS__; }                 \
        else if (W32) { using RT = XT; using WT = ::zigma::F32; __VA_ARGS__; }                   \
        else { using RT = XT; using WT = XT; __VA_ARGS__; }                                      \
    })

// the matrix-core kernels: the two 16-bit types only
#define ZIGMA_DISPATCH_16BIT(DT, T, ...)                                   \
    switch (DT) {                                                          \
        case ZIGMA_F16: { using T = ::zigma::F16; __VA_ARGS__; break; }    \
        case ZIGMA_BF16: { using T = ::zigma::BF16; __VA_ARGS__; break; }  \
        default: return ZIGMA_ERR_DTYPE;                                   \
    }

}  // namespace zigma
