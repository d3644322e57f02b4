// Buffer-addressed element access (descriptor + 32-bit lane offset + scalar offset): accesses beyond the descriptor's extent read zero and store nothing.
#pragma once
#include "vec_io.h"

namespace zigma {

using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *base, int64_t bytes) {
    const unsigned n = bytes > 0x7fffffff ? 0x7fffffffu : static_cast<unsigned>(bytes < 0 ? 0 : bytes);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, static_cast<int>(n), 0x00020000);
}
// one element
template <typename T> __device__ __forceinline__ typename T::raw buf_ld(rsrc_t r, unsigned voff, int soff) {
    if constexpr (sizeof(typename T::raw) == 2) return static_cast<uint16_t>(__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0));
    else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
template <typename T> __device__ __forceinline__ void buf_st(typename T::raw v, rsrc_t r, unsigned voff, int soff) {
    if constexpr (sizeof(typename T::raw) == 2) __builtin_amdgcn_raw_buffer_store_b16(v, r, voff, soff, 0);
    else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
}
// four consecutive elements
template <typename IO> __device__ __forceinline__ typename Pack<IO, 4>::type buf_ld4(rsrc_t r, unsigned voff, int soff) {
    if constexpr (sizeof(typename IO::raw) == 2) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        return make_uint2(v[0], v[1]);
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
        return make_uint4(v[0], v[1], v[2], v[3]);
    }
}
template <typename IO> __device__ __forceinline__ void buf_st4(const typename Pack<IO, 4>::type &v, rsrc_t r, unsigned voff, int soff) {
    if constexpr (sizeof(typename IO::raw) == 2) __builtin_amdgcn_raw_buffer_store_b64(u32x2{v.x, v.y}, r, voff, soff, 0);
    else __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, r, voff, soff, 0);
}

}  // namespace zigma
