// norm_linear: LayerNorm (no affine weight) + adaLN modulate of the rows of x AND the dense projection of the result, in one pass over x, gfx950.
// C ABI: zigma_norm_linear_fwd.
//
// Replaces, together, the pre-attention call of add_norm_kernel (csrc/add_norm.hip: y_mod = r16(r16(LN(x)) * (1 + scale) + shift)) and the to_q call of
// zigma_linear_fwd that is its only reader (reference model_zigma.py:441-446 and :104-128).  Apart, the two kernels move  read h + write xa + read xa +
// write q; here xa is formed in registers in exactly the MFMA operand layout of the projection and never reaches memory:  read h + write q.
//
//   workgroup = 128 rows = 4 waves x 32 rows, two workgroups per CU.  A lane = (row j = lane & 31, k half kh = lane >> 5) holds its row as k / 16
//   fragments of 8 consecutive k (fragment f: k = (2 f + kh) * 8 ...), the operand layout of v_mfma_f32_32x32x16: 160 registers at k = 640.
//   Everything comes in through ONE ring of three 16 KB direct-to-LDS stages (global_load_lds_dwordx4, source-side swizzle, full 128-byte lines):
//   first k / 64 stages of x (128 rows x 64 k; a wave fetches and reads only its own 32 rows), then 8 passes x k / 128 stages of w (64 features x 128 k).
//   The weight stream starts behind the last x stage, so its first stages land while the rows are normalised.
//   Statistics as in add_norm_kernel: fp32 sum while the stages are read, then the two-pass variance on the register copy; a row is shared by the lanes
//   l and l + 32, one exchange per statistic.  Normalise, round, modulate, round, pack: the registers now hold xa.
//   The products are taken transposed (w rows as the MFMA A operand, D[feature][row]) so that a lane holds 4 consecutive features of its row: the
//   32 x 64 output tile of a pass goes through wave-private LDS as 8-byte pieces and leaves as full 128-byte row pieces while the next pass runs.
//   Per pass 32 accumulator registers: 160 + 32 + 24 (three fragment groups of w in flight) stay inside 256, i.e. two waves per SIMD, so one workgroup's
//   prologue and stores hide behind the other's MFMAs.  Every wave reads the whole w stage from LDS: 1 KB per MFMA and wave, the rate LDS delivers.
// bf16 or fp16 (template parameter T); n = 512; k = 512, 640, 768 (template parameter KS = k / 64); m % 128 == 0.
#include "lds_pipe.h"
#include "norm_linear_plan.h"

namespace zigma {
namespace nl {

// LDS accesses are hand-issued (csrc/lds_pipe.h); reads are settled by an explicit s_waitcnt lgkmcnt that names the destination registers.
// lds_rd is lds_pipe.h's but for the constraint letter of the offset ("i", there "n"): the letter changes this kernel's schedule, so the local form stays
template <int OFF = 0> __device__ __forceinline__ void lds_rd(u32x4 &d, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
template <int N> __device__ __forceinline__ void settle2(u32x4 &a, u32x4 &b) {
    static_assert(N == 0 || N == 2 || N == 4, "");
    if (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b));
    else if (N == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(a), "+v"(b));
    else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void settle4(u32x4 &a, u32x4 &b, u32x4 &c, u32x4 &d) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
// s_waitcnt vmcnt(n), n a run-time (wave-uniform) value of {0, 4, 8}: the instruction takes an immediate
__device__ __forceinline__ void wait_vm_n(int n) {
    if (n >= 8) wait_vm<8>();
    else if (n >= 4) wait_vm<4>();
    else wait_vm<0>();
}
template <typename T> __device__ __forceinline__ v2f unpk(unsigned w) { return v2f{lo16<T>(w), hi16<T>(w)}; }

template <int KS, typename T>
__global__ __launch_bounds__(64 * kNlWaves, KS <= 10 ? 2 : 1) void norm_linear_kernel(const zigma_norm_linear_params_t p) {
    constexpr int NF = KS * 4;                       // fragments of a row
    constexpr int NXS = KS;                          // x stages: 64 k each
    constexpr int WPP = KS / 2;                      // w stages per pass: 128 k each
    constexpr int NPASS = kNlN / kNlPass;
    constexpr int NST = kNlStages, SB = kNlStageBytes;
    constexpr int kTileOff = NST * SB, kTileBytes = kNlTok * kNlOutPitch;
    static_assert(KS % 2 == 0 && WPP >= NST && NXS >= NST && NST == 3 && SB == 16384 && kNlPass == 64 && kNlWaves == 4 && kNlTok == 32, "");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[kTileOff + kNlWaves * kTileBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kh = lane >> 5, l3 = lane >> 3;
    const int64_t m0 = (static_cast<int64_t>(blockIdx.x) * kNlWaves + wave) * kNlTok;      // first row of this wave
    const unsigned smem_lds = static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_ptr_t)(smem)));      // LDS byte address

    // ---- sources of the stage loads.  One load instruction = 8 rows x 128 B; lane -> (row l3 of the 8, 16-byte slot (lane & 7) ^ swizzle of the row);
    // the swizzle of row r is swz_slot(r): for rows 8 i + l3 that is (l3 >> 1) ^ ((i & 1) << 2)
    const int64_t x_pitch = p.x_row_stride * 2, w_pitch = p.w_row_stride * 2, o_pitch = p.out_row_stride * 2;
    const unsigned char *xb = reinterpret_cast<const unsigned char *>(p.x) + m0 * x_pitch;                     // (wave-uniform)
    const unsigned char *wb = reinterpret_cast<const unsigned char *>(p.w) + static_cast<int64_t>(wave) * 8 * w_pitch;
    const unsigned slot = static_cast<unsigned>((lane & 7) ^ (l3 >> 1));
    const unsigned xoff0 = static_cast<unsigned>(l3 * x_pitch) + (slot << 4), xoff1 = static_cast<unsigned>(l3 * x_pitch) + ((slot ^ 4u) << 4);
    const unsigned woff = static_cast<unsigned>(l3 * w_pitch) + ((slot ^ static_cast<unsigned>((wave & 1) << 2)) << 4);   // rows 8 (wave + 4 h) + l3

    // x stage st (64 k of this wave's 32 rows) into ring buffer bi: 4 instructions
    auto issue_x = [&](int st, int bi) {
        unsigned char *dst = smem + bi * SB + wave * 4096;
        const unsigned char *src = xb + st * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + static_cast<int64_t>(i) * 8 * x_pitch + ((i & 1) ? xoff1 : xoff0)), (lds_ptr_t)(dst) + i * 1024, 16, 0, 0);
    };
    // w stage (pass, kk): features 64 pass ..., k chunks 2 kk + c (c = 0, 1: sub-block c of the stage, 64 rows x 128 B) into ring buffer bi: 4 instructions
    auto issue_w = [&](int pass, int kk, int bi) {
        unsigned char *dst = smem + bi * SB + wave * 1024;
        const unsigned char *src = wb + static_cast<int64_t>(pass) * kNlPass * w_pitch + kk * 256 + woff;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i >> 1, h = i & 1;
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src + static_cast<int64_t>(h) * 32 * w_pitch + c * 128), (lds_ptr_t)(dst) + c * 8192 + h * 4096, 16, 0, 0);
        }
    };

    // this lane's 16-byte piece at k-step 0 of row j of a 32-row block; k-step ks is ^ (ks << 5): the slot is ((ks << 1) | kh) ^ swizzle
    const unsigned lrd = smem_lds + static_cast<unsigned>(j * 128 + ((kh ^ swz_slot(j)) << 4));

    // ---- the rows: x stages -> registers, fp32 sum on the way ----
    u32x4 xf[NF];
    v2f sum2 = {0.f, 0.f};
    issue_x(0, 0);
    issue_x(1, 1);
#pragma unroll
    for (int s = 0; s < NXS; ++s) {
        // stage s has landed (this wave's loads: vmcnt, VM_CNT retires in issue order and one younger stage may stay in flight; every wave's: barrier);
        // stage s - 1 is consumed by every wave, its buffer takes stage s + 2
        wait_vm_n(4);
        __builtin_amdgcn_s_barrier();
        if (s + 2 < NXS) issue_x(s + 2, (s + 2) % NST);
        else issue_w(0, s + 2 - NXS, (s + 2) % NST);
        const unsigned a = lrd + (s % NST) * SB + wave * 4096;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) lds_rd(xf[s * 4 + ks], a ^ (ks << 5));
        settle4(xf[s * 4], xf[s * 4 + 1], xf[s * 4 + 2], xf[s * 4 + 3]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int d = 0; d < 4; ++d) sum2 += unpk<T>(xf[s * 4 + ks][d]);
    }

    // ---- LayerNorm + modulate on the register copy: the arithmetic and the two rounding points of add_norm_kernel ----
    {
        float sum = sum2.x + sum2.y;
        sum += __shfl_xor(sum, 32, 64);
        const float mean = sum / p.k;
        v2f var2 = {0.f, 0.f};
        // (each pass over the row widens its 16-bit values again: the empty asm makes a fragment a new value, or the compiler would keep the fp32 copies
        // of an earlier pass — 320 registers — alive for the next one)
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            asm volatile("" : "+v"(xf[f]));
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const v2f dl = unpk<T>(xf[f][d]) - mean;
                var2 += dl * dl;
            }
        }
        float var = var2.x + var2.y;
        var += __shfl_xor(var, 32, 64);
        const float rstd = rsqrtf(var / p.k + p.eps);
        const int64_t b = (m0 + j) / p.rows_per_batch;                 // per row: a tile may straddle samples
        const unsigned char *shp = reinterpret_cast<const unsigned char *>(p.shift) + b * p.mod_batch_stride * 2 + kh * 16;
        const unsigned char *scp = reinterpret_cast<const unsigned char *>(p.scale) + b * p.mod_batch_stride * 2 + kh * 16;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const u32x4 sh = *reinterpret_cast<const u32x4 *>(shp + f * 32), sc = *reinterpret_cast<const u32x4 *>(scp + f * 32);
            asm volatile("" : "+v"(xf[f]));
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const v2f y = (unpk<T>(xf[f][d]) - mean) * rstd;
                const v2f yr = unpk<T>(pack2_pk<T>(y.x, y.y));
                const v2f o = yr * (1.f + unpk<T>(sc[d])) + unpk<T>(sh[d]);
                xf[f][d] = pack2_pk<T>(o.x, o.y);
            }
            if (f % 4 == 3) asm volatile("" ::: "memory");            // (keeps the shift / scale loads of later fragments from piling up in registers)
        }
    }

    // ---- the projection: 8 passes of 64 features over the rows in registers ----
    const unsigned tile = smem_lds + kTileOff + wave * kTileBytes;
    unsigned char *ob = reinterpret_cast<unsigned char *>(p.out) + (m0 + l3) * o_pitch + (lane & 7) * 16;
    int buf = NXS % NST;
#pragma unroll 1
    for (int pass = 0; pass < NPASS; ++pass) {
        mfma_f32x16 acc[2];
        acc[0] = mfma_f32x16{};
        acc[1] = mfma_f32x16{};
#pragma unroll
        for (int kk = 0; kk < WPP; ++kk) {
            // behind this stage's loads in the queue: the next stage's (none at the very end) and, in the first two stages of a pass, the 4 stores of
            // the previous pass's tile (issued behind the loads of this stage and of the next one at most).  ASSUMPTION the synchronisation rests on: on gfx9
            // VM_CNT counts global stores and direct-to-LDS loads in ONE queue that retires in issue order (there is no separate store counter as on gfx10+;
            // LLVM's waitcnt insertion assumes the same, and conv_x_proj.hip counts its u stores this way) — stores retiring early would let the wait pass
            // before the stage has landed.
            {
                const int younger = (pass == NPASS - 1 && kk == WPP - 1) ? 0 : 4;
                const int stores = (pass > 0 && kk < NST - 1) ? 4 : 0;
                wait_vm_n(younger + stores);
            }
            __builtin_amdgcn_s_barrier();
            {
                const int prev = buf == 0 ? NST - 1 : buf - 1;
                if (kk + 2 < WPP) issue_w(pass, kk + 2, prev);
                else if (pass + 1 < NPASS) issue_w(pass + 1, kk + 2 - WPP, prev);
            }
            const unsigned a0 = lrd + buf * SB;
            // groups g = (c, ks): the two feature blocks' fragments of one k-step; two groups are read ahead of the one being multiplied
            u32x4 wf[3][2];
            auto reads = [&](int g) {
                const unsigned a = a0 ^ ((g & 3) << 5);
                if (g < 4) { lds_rd(wf[g % 3][0], a); lds_rd<4096>(wf[g % 3][1], a); }
                else { lds_rd<8192>(wf[g % 3][0], a); lds_rd<8192 + 4096>(wf[g % 3][1], a); }
            };
            reads(0);
            reads(1);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if (g + 2 < 8) { reads(g + 2); settle2<4>(wf[g % 3][0], wf[g % 3][1]); }
                else if (g + 1 < 8) settle2<2>(wf[g % 3][0], wf[g % 3][1]);
                else settle2<0>(wf[g % 3][0], wf[g % 3][1]);
                const frag8_t<T> xa = __builtin_bit_cast(frag8_t<T>, xf[kk * 8 + g]);
                acc[0] = mfma_32x32x16<T>(__builtin_bit_cast(frag8_t<T>, wf[g % 3][0]), xa, acc[0]);
                acc[1] = mfma_32x32x16<T>(__builtin_bit_cast(frag8_t<T>, wf[g % 3][1]), xa, acc[1]);
            }
            buf = buf + 1 == NST ? 0 : buf + 1;
        }
        // the pass's 32 rows x 64 features: a lane holds row j and the features nb * 32 + (r & 3) + 8 (r >> 2) + 4 kh — 4 consecutive features per register
        // group, one 8-byte piece.  Through the wave's own LDS tile (in order behind the reads of the previous pass, which have been settled) and out as
        // 16-byte pieces, 8 lanes = one full 128-byte line of a row.
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x2 pk = {pack2_pk<T>(acc[nb][q * 4], acc[nb][q * 4 + 1]), pack2_pk<T>(acc[nb][q * 4 + 2], acc[nb][q * 4 + 3])};
                lds_wr8(tile + j * kNlOutPitch + nb * 64 + q * 16 + kh * 8, pk);
            }
        u32x4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_rd(t[i], tile + (i * 8 + l3) * kNlOutPitch + (lane & 7) * 16);
        settle4(t[0], t[1], t[2], t[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4 *>(ob + static_cast<int64_t>(i) * 8 * o_pitch + pass * (2 * kNlPass)) = t[i];
    }
}

}  // namespace nl
}  // namespace zigma

using namespace zigma;

extern "C" int zigma_norm_linear_fwd(const zigma_norm_linear_params_t *pp, void *stream_) {
    if (!pp) return ZIGMA_ERR_NULL;
    (void)hipGetLastError();
    const zigma_norm_linear_params_t &p = *pp;
    const NormLinearPlan plan = plan_norm_linear(p);
    if (!plan.kernel) return plan.status;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(plan.grid), block(plan.block);
#define ZIGMA_NL(KS_) ZIGMA_DISPATCH_16BIT(p.dtype, T, hipLaunchKernelGGL((nl::norm_linear_kernel<KS_, T>), grid, block, 0, stream, p))
    if (plan.ksteps == 8) { ZIGMA_NL(8) } else if (plan.ksteps == 10) { ZIGMA_NL(10) } else { ZIGMA_NL(12) }
#undef ZIGMA_NL
    set_last_kernel(plan.kernel);
    return check_launch();
}

extern "C" int zigma_norm_linear_fwd_plan(const zigma_norm_linear_params_t *pp, const char **kernel) {
    return pp && kernel ? query_norm_linear(*pp, kernel) : ZIGMA_ERR_NULL;
}
