// Hand-issued LDS and wait primitives of the direct-to-LDS pipelines (linear*.hip, norm_linear.hip, conv_x_proj.hip), and their bank swizzle.
//
// Why inline assembly (cdna_hip_programming.md §5 / T2 / rule 21).  The pipelines keep several stages of global_load_lds_dwordx4 in flight and
// track their landing by hand: a COUNTED s_waitcnt vmcnt (VM_CNT retires in issue order, so the count is "what was issued after the batch that
// is needed now") and one s_barrier per stage.  hipcc cannot know which bytes an LDS-DMA in flight targets, so in front of every ds_read or
// ds_write IT CAN SEE it drains vmcnt to 0 — the younger stages included, and with them the whole pipeline.  Hence:
//   * LDS accesses next to a running load ring are issued with lds_rd / lds_wr8, which the compiler does not look into;
//   * their data is waited for explicitly: wait_lgkm<N>(), or an `asm volatile("s_waitcnt lgkmcnt(N)" : "+v"(dst)...)` that names the destination
//     registers, so that no use can be scheduled above it (the `settle` forms of the kernels: they differ in what they name and stay with them);
//   * a kernel keeps ONE LDS object: a second one makes hipcc drain vmcnt in front of every fragment read all the same.
// The LDS queue of one wave executes in order, so a wave's own writes and later reads of a private tile need no barrier between them.
#pragma once
#include "zigma_common.h"

namespace zigma {

// ds_read_b128 / ds_write_b64 at a byte address + immediate offset
template <int OFF = 0> __device__ __forceinline__ void lds_rd(u32x4 &d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int OFF = 0> __device__ __forceinline__ void lds_wr8(unsigned addr, const u32x2 &v) {
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void barrier() { asm volatile("s_barrier" ::: "memory"); }

// Bank swizzle of an LDS image of 128-byte rows (T2): the 16-byte slot of a row is XORed with swz_slot(row), which makes ds_read_b128 of the
// same logical slot of 32 consecutive rows conflict-free.  A direct-to-LDS image is lane-linear, so there the term is applied to the per-lane
// SOURCE address, and again on the fragment reads.
template <typename I> __device__ __forceinline__ constexpr I swz_slot(const I row) { return (row >> 1) & 7; }
// byte offset of 16-byte piece `piece` of row `row`
__device__ __forceinline__ int swz(const int row, const int piece) { return row * 128 + ((piece ^ swz_slot(row)) << 4); }

}  // namespace zigma
