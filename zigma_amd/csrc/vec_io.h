// Packed element I/O by dtype: VEC consecutive elements of a row <-> float32 values, for the streaming kernels (add_norm, norm_bwd, causal conv1d
// forward and backward).  16-bit elements widen by to_float and narrow by from_float (zigma_common.h): one rounding, to nearest even.
#pragma once
#include "zigma_common.h"

#include <type_traits>

namespace zigma {

template <typename T, int VEC> struct Pack {      // VEC consecutive elements as one register value of 8 or 16 bytes
    static_assert(sizeof(typename T::raw) * VEC == 8 || sizeof(typename T::raw) * VEC == 16, "");
    using type = typename std::conditional<sizeof(typename T::raw) * VEC == 16, uint4, uint2>::type;
};

template <typename T> __device__ __forceinline__ void unpack4(const typename Pack<T, 4>::type &r, float (&f)[4]) {
    if constexpr (T::id == ZIGMA_F32) {
        f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
    } else {
        f[0] = to_float<T>(r.x & 0xffffu); f[1] = to_float<T>(r.x >> 16);
        f[2] = to_float<T>(r.y & 0xffffu); f[3] = to_float<T>(r.y >> 16);
    }
}
template <typename T> __device__ __forceinline__ typename Pack<T, 4>::type pack4(const float (&f)[4]) {
    if constexpr (T::id == ZIGMA_F32) {
        return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
    } else {
        return make_uint2(from_float<T>(f[0]) | (uint32_t(from_float<T>(f[1])) << 16),
                          from_float<T>(f[2]) | (uint32_t(from_float<T>(f[3])) << 16));
    }
}

// VEC consecutive elements from / to element index idx: 1 (scalar, any alignment), 4, or 8 (two float4 / one 16-byte piece of 16-bit elements)
template <typename T, int VEC> __device__ __forceinline__ void loadv(const void *base, int64_t idx, float (&f)[VEC]) {
    if constexpr (VEC == 1) {
        f[0] = ld<T>(base, idx);
    } else if constexpr (VEC == 4) {
        unpack4<T>(*reinterpret_cast<const typename Pack<T, 4>::type *>(reinterpret_cast<const typename T::raw *>(base) + idx), f);
    } else if constexpr (T::id == ZIGMA_F32) {
        float a[4], b[4];
        loadv<T, 4>(base, idx, a);
        loadv<T, 4>(base, idx + 4, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[i] = a[i]; f[4 + i] = b[i]; }
    } else {
        const uint4 r = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(base) + idx);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[2 * i] = to_float<T>(w[i] & 0xffffu); f[2 * i + 1] = to_float<T>(w[i] >> 16); }
    }
}
template <typename T, int VEC> __device__ __forceinline__ void storev(void *base, int64_t idx, const float (&f)[VEC]) {
    if constexpr (VEC == 1) {
        st<T>(base, idx, f[0]);
    } else if constexpr (VEC == 4) {
        *reinterpret_cast<typename Pack<T, 4>::type *>(reinterpret_cast<typename T::raw *>(base) + idx) = pack4<T>(f);
    } else if constexpr (T::id == ZIGMA_F32) {
        const float a[4] = {f[0], f[1], f[2], f[3]}, b[4] = {f[4], f[5], f[6], f[7]};
        storev<T, 4>(base, idx, a);
        storev<T, 4>(base, idx + 4, b);
    } else {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = from_float<T>(f[2 * i]) | (uint32_t(from_float<T>(f[2 * i + 1])) << 16);
        *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(base) + idx) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}
// value the tensor would hold after being stored in dtype T (the reference materialises these tensors)
template <typename T> __device__ __forceinline__ float rnd(float v) { return to_float<T>(from_float<T>(v)); }

}  // namespace zigma
