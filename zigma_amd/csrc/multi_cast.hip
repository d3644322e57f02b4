// zigma_multi_cast_fwd: round many float32 tensors to bf16 / fp16 in ONE launch (include/zigma_hip.h).  Mixed-precision training keeps fp32
// parameters and 16-bit copies of the matrix weights for the projection kernels; the copies go stale once per optimizer step, and
// refreshing ~400 of them with one `.to()` each is ~400 launches.  Here a device table names every (src, dst, numel) and a chunk map
// names, per workgroup, the table entry and the first element of its piece: one HBM-bound pass of 6 bytes per element, no LDS.
#include "zigma_common.h"

namespace zigma {

constexpr int kCastThreads = 256;

template <typename T>
__global__ __launch_bounds__(kCastThreads) void multi_cast_kernel(const zigma_multi_cast_entry_t *__restrict__ table,
                                                                  const zigma_multi_cast_chunk_t *__restrict__ chunk_map, int64_t n_entries, int chunk) {
    const zigma_multi_cast_chunk_t c = chunk_map[blockIdx.x];
    if (c.entry < 0 || c.entry >= n_entries) return;                  // (a map row outside the table: skipped, never followed)
    const zigma_multi_cast_entry_t e = table[c.entry];
    if (c.offset < 0 || c.offset >= e.numel) return;
    const int64_t left = e.numel - c.offset;
    const int n = left < chunk ? static_cast<int>(left) : chunk;
    // (the pointers come out of memory, so the compiler cannot see their address space: say that they are global, or every access is a flat one)
    typedef const float __attribute__((address_space(1))) *src_ptr;
    typedef uint16_t __attribute__((address_space(1))) *dst_ptr;
    const src_ptr src = (src_ptr)(e.src + c.offset);
    const dst_ptr dst = (dst_ptr)(static_cast<uint16_t *>(e.dst) + c.offset);
    const int tid = threadIdx.x;
    // uniform over the workgroup: both pieces start on 16-byte boundaries -> 8 elements per lane and access
    const bool wide = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    int done = 0;
    if (wide) {
        const int n8 = n & ~7;
        for (int i = tid * 8; i < n8; i += kCastThreads * 8) {
            const v4f a = *(const v4f __attribute__((address_space(1))) *)(src + i);
            const v4f b = *(const v4f __attribute__((address_space(1))) *)(src + i + 4);
            u32x4 o;
            o.x = pack2_pk<T>(a.x, a.y);
            o.y = pack2_pk<T>(a.z, a.w);
            o.z = pack2_pk<T>(b.x, b.y);
            o.w = pack2_pk<T>(b.z, b.w);
            *(u32x4 __attribute__((address_space(1))) *)(dst + i) = o;
        }
        done = n8;
    }
    for (int i = done + tid; i < n; i += kCastThreads) dst[i] = from_float<T>(src[i]);       // unaligned pieces, and a tensor's last numel % 8
}

}  // namespace zigma

using namespace zigma;

extern "C" int zigma_multi_cast_fwd(const zigma_multi_cast_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_multi_cast_params_t &p = *pp;
    if (p.n_entries < 0 || p.n_chunks < 0 || p.n_chunks > 0x7fffffffLL) return ZIGMA_ERR_SHAPE;
    if (p.out_dtype != ZIGMA_BF16 && p.out_dtype != ZIGMA_F16) return ZIGMA_ERR_DTYPE;
    if (p.flags != 0) return ZIGMA_ERR_UNSUPPORTED;
    if (p.n_entries == 0 || p.n_chunks == 0) return ZIGMA_OK;
    if (!p.table || !p.chunk_map) return ZIGMA_ERR_NULL;
    if (p.chunk < 8 || p.chunk > 65536 || p.chunk % 8 != 0) return ZIGMA_ERR_SHAPE;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(static_cast<unsigned>(p.n_chunks));
    ZIGMA_DISPATCH_16BIT(p.out_dtype, T,
                         hipLaunchKernelGGL(multi_cast_kernel<T>, grid, dim3(kCastThreads), 0, stream, p.table, p.chunk_map, p.n_entries, p.chunk));
    set_last_kernel(p.out_dtype == ZIGMA_BF16 ? "multi_cast_bf16" : "multi_cast_f16");
    return check_launch();
}
