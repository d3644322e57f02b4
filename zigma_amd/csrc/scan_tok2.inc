// Token-major selective scan, second-generation hot kernel (16-bit I/O, dstate 16, seqlen % 16 == 0; gated output, and as
// template flag OUT the training form: ungated `out` + per-tile checkpoints; sequence split (MODE 1 / 2); reset_period).
// Included by scan_tok_{bf16,f16}.hip next to scan_tok.inc; f32 I/O, ragged lengths, dstate 8 and carries without a split stay
// on scan_tok_kernel.
//
// Same decomposition as scan_tok_kernel (workgroup = sample x 64-channel slab, 4 waves x 4 states, lane = channel, time
// sequential in the lane, per-element work shared through LDS between 16-step tiles).  What changed, and why
// (measurements: tools/ubench2, profiles/r02_ubench2_valu_rates.txt — wall ns per wave-instruction per SIMD at 5 waves/SIMD:
// plain VOP2 1.35, DPP-operand 1.87, v_exp_f32 3.43, v_pk_{mul,fma}_f32 2.28 for two results):
//   * B_l / C_l no longer ride DPP operands.  The workgroup converts the tile's 16 x (16 + 16) values to fp32 ONCE
//     (one 4-byte load per thread per tile) into LDS; every wave fetches its 4 states of a step with one ds_read_b128
//     whose address is wave-uniform (a broadcast read: no bank conflict, no VALU slot) and uses them as PLAIN operands.
//   * with plain operands the five products of the recurrence pack two states per instruction (VOP3P v_pk_mul_f32 /
//     v_pk_fma_f32, the scalar dt / dt*u broadcast by op_sel): per (step, 4 states) 8 packed + 1 add + 4 v_exp instead of
//     16 VOP2/DPP + 4 v_exp.
//   * no run-time feature switches inside the loop (row tables are template parameters, no carries, no bounds).
#pragma once
#include "buffer_io.h"
#include "scan_helpers.h"

#include <type_traits>

namespace zigma {

template <typename IO> __device__ __forceinline__ v2f unpack2(uint32_t v);
template <> __device__ __forceinline__ v2f unpack2<BF16>(uint32_t v) {
    return v2f{__uint_as_float(v << 16), __uint_as_float(v & 0xffff0000u)};
}
template <> __device__ __forceinline__ v2f unpack2<F16>(uint32_t v) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h = __builtin_bit_cast(h2, v);
    return v2f{static_cast<float>(h.x), static_cast<float>(h.y)};
}

// SP: delta + bias and (run-time flag) softplus in the prologue, for callers that did not fuse them into dt_proj.
// TAB: z / out row tables.  ZACT: z already holds silu(z) (ZIGMA_SCAN_Z_PREACTIVATED).
// MODE 0: whole sequence in one workgroup.  MODE 1 / 2: sequence split (long sequences of few samples, or small batches:
// batch * dim / 64 workgroups cannot fill 256 CUs): gridDim.y chunks of chunk_len steps run in parallel —
//   MODE 1: recurrence only, from h = 0, writes the chunk-local carry (prod a, h_end) to x;
//   zigma_scan_combine_kernel turns the local carries into running prefixes in place (this IS the reference's x tensor,
//   selective_scan_fwd_kernel.cuh:251-254);  MODE 2: every chunk starts from x[chunk - 1] and produces the outputs.
// s_setprio takes an immediate: run-time levels go through a (scalar) switch
__device__ __forceinline__ void set_prio_rt(int q) {
    switch (q) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// OUT (MODE 0 only): the training forward — also write the UNGATED y (`out`, what the backward's dz needs) and, if the caller passed
// `checkpoints`, the state before every tile (zigma_selective_scan_bwd then skips its own forward phase).
// (Not taken, measured: B_l / C_l through the SCALAR unit instead of LDS broadcast reads — s_load_dwordx2 per step + SALU widening, SGPR
// operands.  A replica of the tile loop with a cache-resident table gains 8 % (tools/ubench3), the kernel LOSES 43 % (329 vs 231 us):
// every step's B / C row is a fresh 64-byte line from L2, and the 102-SGPR budget allows a queue of 2 steps, not the tile the latency
// needs.  The variant is archived as tools/experiments/scan_tok2_scalar_bc_r03.patch.)
// DTP (MODE 0, 16-bit I/O; round 4): dt_proj + bias + softplus INSIDE the kernel.  delta is not read: every tile, wave w forms
// delta'[16 steps][channels 16 w .. 16 w + 15] = softplus(x_dbl[:, :dt_rank] . W_dt^T + bias) with two MFMAs on the matrix pipe this
// kernel otherwise leaves idle (two v_mfma_f32_16x16x32_bf16: r < 32 and 32 <= r < 64, zero weights beyond dt_rank; W_dt of the wave's 16
// channels stays in 8 registers, the bias enters as the C operand) from the dt columns of the SAME x_dbl rows B_l / C_l come
// from, and writes (dt, dt * u) of its 4 x 16 elements per lane to s_dtdu in the accumulator layout (lane = channel n, steps
// 4 q .. 4 q + 3).  The (batch, seqlen, dim) delta tensor — 168 MB written by dt_proj_softplus_kernel and read back here at the
// headline shape — and that kernel's launch disappear; the price is the softplus on this kernel's VALU (7 instructions per element).
// R6 (round 5; DTP form only): six resident workgroups per CU instead of five — 80 registers (operands one step ahead instead of two) and the
// 26 KB of LDS every form now uses (B / C staging single-buffered: like s_dtdu it is written between the two barriers and read behind the
// second).  For grids that are ONE round of six per CU and one round + a tail of five: Di = 1536 (the reference's E = 768 models) at B = 64 is
// 1536 workgroups — with five resident the last 256 ran one per CU.
// ACC (round 6; DTP form only): out_z = out_z + y * silu(z) — the second sweep of the bidirectional `v2` scan type adds itself to the first sweep's result
// (reference mamba_simple.py:335-339: `out + out_b.flip([-1])`, an elementwise pass over (B, L, d_inner) of its own: 91 us per layer at B = 64, E = 768).
// The rows to add to are requested at the END of the core phase (their registers are the dead operand queue: the six-resident form has no register to
// spare across the core) and land behind the tile's fence like every other 16-bit row.
template <typename IO, bool SP, bool TAB, bool ZACT, int MODE, bool OUT = false, bool DTP = false, bool R6 = false, bool ACC = false>
__global__ __launch_bounds__(256, R6 ? 6 : 5) void scan_tok2_kernel(const zigma_scan_params_t p, const int n_slabs) {
    static_assert(!DTP || (MODE != 2 && !OUT && sizeof(typename IO::raw) == 2), "in-kernel dt_proj: whole-sequence inference form, or the state-only first pass of the sequence split");
    static_assert(!DTP || MODE == 0 || (!R6 && !ACC && !TAB && !ZACT), "split first pass with the in-kernel dt_proj: one instantiation");
    static_assert(!ACC || DTP, "accumulating form: instantiated for the in-kernel dt_proj form only");
    static_assert(!R6 || DTP, "six resident workgroups: instantiated for the in-kernel dt_proj form only");
    constexpr int LT = 16, NW = 4, RPT = 4, NG = 4, ES = 2;
    using io_t = typename IO::raw;
    static_assert(sizeof(io_t) == 2, "16-bit I/O only");
    __shared__ __attribute__((aligned(16))) float s_dtdu[LT][64][2];        // [step][channel][dt, dt*u]             8 KB
    __shared__ __attribute__((aligned(16))) float s_bc[LT][2][16];          // [step][B | C][state]                  2 KB
    __shared__ __attribute__((aligned(16))) float s_y[NW][LT][64];          // partial y of every wave, [wave][step][channel]  16 KB

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slab = blockIdx.x % n_slabs, b = blockIdx.x / n_slabs;      // batch folded into grid.x (no 65535 limit)
    const int c = slab * 64 + lane;
    const int L = p.seqlen;
    const int n0 = wave * 4;
    const int chunk_len = p.chunk_len > 0 ? p.chunk_len : 2048;
    const int chunk = MODE ? blockIdx.y : 0;
    const int kb = MODE ? chunk * chunk_len : 0;                                       // first step of this workgroup
    const int k_end = MODE ? (kb + chunk_len < L ? kb + chunk_len : L) : L;
    const int n_chunks = (L + chunk_len - 1) / chunk_len;

    // DTP keeps the step size in LOG2 units: dt' = dt * log2(e) = log2(1 + 2^(x log2 e)) comes straight out of v_log_f32, so the
    // softplus needs no `* ln 2`; exp(dt A) = exp2(dt' A) takes A as stored (no `* log2 e`), and dt u = ln 2 * dt' u is restored by
    // scaling B_l ONCE per tile in the B / C staging (one multiply per thread per tile instead of one per element) — the state then
    // carries exactly the h of the reference (selective_scan_fwd_kernel.cuh:153-171 computes the same delta, delta * A, delta * u).
    // MODE 1 with DTP (round 6: the sequence split's first pass forms delta itself — the dt_proj kernel of its own and one read of delta go) keeps NATURAL
    // units: there delta is rounded to the I/O type and WRITTEN for the second pass (both passes must see the same rounded step sizes, or the
    // chunk carries would belong to another recurrence than the one the second pass continues).
    constexpr bool LOG2U = DTP && MODE == 0;
    constexpr float kAScale = LOG2U ? 1.f : kLog2e;
    v2f a2A, a2B, hA = {0.f, 0.f}, hB = {0.f, 0.f};
    {
        const float *Ar = reinterpret_cast<const float *>(p.A) + c * p.A_d_stride;
        a2A = v2f{Ar[(n0 + 0) * p.A_dstate_stride], Ar[(n0 + 1) * p.A_dstate_stride]} * kAScale;
        a2B = v2f{Ar[(n0 + 2) * p.A_dstate_stride], Ar[(n0 + 3) * p.A_dstate_stride]} * kAScale;
    }
    if (MODE == 2 && chunk > 0) {
        const float *xr = reinterpret_cast<const float *>(p.x) + ((static_cast<int64_t>(b) * p.dim + c) * n_chunks + chunk - 1) * 2 * p.dstate;
        hA = v2f{xr[2 * n0 + 1], xr[2 * n0 + 3]};
        hB = v2f{xr[2 * n0 + 5], xr[2 * n0 + 7]};
    }
    float a2s[4] = {a2A.x, a2A.y, a2B.x, a2B.y}, hs[4] = {0.f, 0.f, 0.f, 0.f};      // MODE 1 works on scalars (asm block per step)
    const float Dv = p.D ? reinterpret_cast<const float *>(p.D)[c] : 0.f;
    const float bias = (SP && p.delta_bias) ? reinterpret_cast<const float *>(p.delta_bias)[c] : 0.f;
    const bool sp_on = p.delta_softplus != 0;

    const unsigned lane_off = static_cast<unsigned>(c) * ES;
    const int u_ls = static_cast<int>(p.u_l_stride) * ES, d_ls = static_cast<int>(p.delta_l_stride) * ES;
    const int z_ls = static_cast<int>(p.z_l_stride) * ES, oz_ls = static_cast<int>(p.out_z_l_stride) * ES;
    const int B_ls = static_cast<int>(p.B_l_stride) * ES, C_ls = static_cast<int>(p.C_l_stride) * ES;
    const int64_t Lm1 = L - 1, dimb = static_cast<int64_t>(p.dim) * ES;
    const rsrc_t u_rs = make_rsrc(reinterpret_cast<const io_t *>(p.u) + b * p.u_batch_stride, Lm1 * u_ls + dimb);
    const rsrc_t d_rs = make_rsrc(reinterpret_cast<const io_t *>(p.delta) + b * p.delta_batch_stride, Lm1 * d_ls + dimb);
    const rsrc_t z_rs = make_rsrc(reinterpret_cast<const io_t *>(p.z) + b * p.z_batch_stride, Lm1 * z_ls + dimb);
    const rsrc_t oz_rs = make_rsrc(reinterpret_cast<const io_t *>(p.out_z) + b * p.out_z_batch_stride, Lm1 * oz_ls + dimb);
    const int o_ls = OUT ? static_cast<int>(p.out_l_stride) * ES : 0;
    const rsrc_t o_rs = make_rsrc(OUT ? reinterpret_cast<const io_t *>(p.out) + b * p.out_batch_stride : nullptr, OUT ? Lm1 * o_ls + dimb : 0);
    // B / C staging: waves 0, 1 fetch B, waves 2, 3 fetch C (wave-uniform descriptor); thread -> (step = (tid & 127) / 8,
    // state pair = tid & 7): one dword = two adjacent states
    const int bc_is_c = wave >> 1, bc_step = (tid & 127) >> 3, bc_pair = tid & 7;
    const int bc_ls = bc_is_c ? C_ls : B_ls;
    const rsrc_t bc_rs = bc_is_c ? make_rsrc(reinterpret_cast<const io_t *>(p.C) + b * p.C_batch_stride, Lm1 * C_ls + p.dstate * ES)
                                 : make_rsrc(reinterpret_cast<const io_t *>(p.B) + b * p.B_batch_stride, Lm1 * B_ls + p.dstate * ES);
    const unsigned bc_voff = static_cast<unsigned>(bc_step * bc_ls + bc_pair * 4);
    const float bc_scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((LOG2U && !bc_is_c) ? 0x3f317218 : 0x3f800000));   // ln 2 | 1 (wave-uniform: an SGPR; see kAScale)
    const int n_tiles = (k_end - kb) / LT;
    // ---- DTP: W_dt fragments of this wave's 16 channels (B operand: lane = (channel n16, k-group kq)), bias, row descriptors
    const int n16 = lane & 15, kq = lane >> 4;
    u32x4 wdt0 = {0, 0, 0, 0};
    u32x4 wdt1 = {0, 0, 0, 0};
    float dbias = 0.f;
    rsrc_t x_rs = u_rs;
    unsigned xa_voff = 0, up_voff = 0;
    int x_ls = 0;
    if constexpr (DTP) {
        const int cw = slab * 64 + wave * 16 + n16;
        const unsigned char *wr = reinterpret_cast<const unsigned char *>(p.dt_w) + static_cast<int64_t>(cw) * p.dt_w_row_stride * 2;
        wdt0 = *reinterpret_cast<const u32x4 *>(wr + kq * 16);                               // r = 8 kq .. 8 kq + 7 (dt_rank >= 32)
        if (32 + 8 * kq < p.dt_rank) wdt1 = *reinterpret_cast<const u32x4 *>(wr + 64 + kq * 16);     // r = 32 + 8 kq .. + 7, zero beyond dt_rank
        dbias = p.delta_bias ? reinterpret_cast<const float *>(p.delta_bias)[cw] : 0.f;
        x_ls = static_cast<int>(p.dt_x_l_stride) * ES;
        x_rs = make_rsrc(reinterpret_cast<const io_t *>(p.dt_x) + b * p.dt_x_batch_stride, Lm1 * x_ls + 128);
        xa_voff = static_cast<unsigned>(n16 * x_ls + kq * 16);                                   // A operand: lane = (step n16, k-group kq)
        up_voff = static_cast<unsigned>(cw * ES + 4 * kq * u_ls);                                // u of (steps 4 kq + i, channel cw)
    }

    // Wave priority of the core phase.  The SIMD arbiter serves the OLDEST wave first: of the 5 workgroups a CU holds (the grid is
    // exactly one round of them) the first-dispatched ones run ahead and finish at 47 % of the kernel's time, the last ones at 97 %
    // (tools/scan_stamps.py) — the tail runs with too few partner waves to fill the VALU.  So the base priority ROTATES: 5 positions
    // (dispatch round of the workgroup + tile index, mod 5) over the 4 levels, advanced every tile; every workgroup is the favoured
    // one a fifth of the time and the finish times close up to 80 ... 97 %: 264 -> 257 us (tools/scan_ab.py; slower rotation periods
    // and a rotation inside the tile measured worse; probe bit 9 turns it off).
    // (round 5: the two passes of the sequence-split mode rotate as well — their grids are sized for the same one round of 5 workgroups
    // per CU; the dispatch round of a workgroup is its LINEAR index / 256, chunks being the slow grid dimension)
    const bool prio_rot = !((p.flags >> ZIGMA_SCAN_PROBE_PRIO_SHIFT) & 1);
    const int kslot = static_cast<int>((blockIdx.x + (MODE ? blockIdx.y * gridDim.x : 0u)) >> 8);
    int base_q = 0;
    // timing probes, compiled only into the probe library of tools/ (-DZIGMA_SCAN_PROBES, tools/scan_stamps.py, tools/scan_ab.py):
    // flags bit 12: start / end time stamps of every workgroup into the (otherwise unused) checkpoints buffer; bits 13 / 14 (results
    // wrong): no barriers / no y hand-over.  As run-time switches they cost the shipped core loop a branch per 4 steps
#ifdef ZIGMA_SCAN_PROBES
    const bool stamp = MODE == 0 && (p.flags & 0x1000) && p.checkpoints;
    const bool nobar = MODE == 0 && (p.flags & 0x2000) != 0;
    const bool noy = MODE == 0 && (p.flags & 0x4000) != 0;
#else
    constexpr bool stamp = false;
#ifdef ZIGMA_SCAN_PROBE_NOBAR      // (compile-time forms of the two probes, tools/scan_idle_probe.py: no branch in the loop)
    constexpr bool nobar = MODE == 0;
#else
    constexpr bool nobar = false;
#endif
#ifdef ZIGMA_SCAN_PROBE_NOY
    constexpr bool noy = MODE == 0;
#else
    constexpr bool noy = false;
#endif
#endif
    auto now = []() { uint64_t t; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory"); return t; };
    if (stamp && tid == 0) reinterpret_cast<uint64_t *>(p.checkpoints)[2 * blockIdx.x] = now();

    // bf16 rows land as FLOATS: buffer_load_short_d16_hi writes the HIGH half of its destination and keeps the low half, so a register
    // whose low half was zeroed once holds the fp32 value of every bf16 it receives — the 12 (16 without dt_proj) v_lshlrev per tile-wave
    // of the u / delta / z conversions disappear.  The load is inline assembly (hipcc has no selection pattern for the tied form on buffer
    // loads), so its arrival is NOT tracked by the compiler's s_waitcnt insertion: fence16() below is the wait — one s_waitcnt vmcnt(0) per
    // tile at the head of the inter-barrier phase, a whole core phase after the loads were issued (every register is an operand of the
    // fence, so no use can be scheduled above it).  Compiler-tracked loads / stores of the loop stay correct: counters retire in order and
    // extra older or younger operations only make the compiler's counted waits stricter.
#ifdef ZIGMA_SCAN_NO_D16HI
    constexpr bool HI16 = false;
#else
    constexpr bool HI16 = std::is_same<IO, BF16>::value;
#endif
    using r16_t = typename std::conditional<HI16, uint32_t, io_t>::type;
    r16_t ru[RPT] = {}, rd[RPT] = {}, rz[RPT] = {};
    r16_t up[RPT] = {};            // DTP: u in the accumulator layout
    r16_t rac[RPT];                // ACC: the rows of out_z this tile adds to
    auto ld16 = [&](r16_t &dst, const rsrc_t &rs, unsigned voff, int soff) {
#ifdef ZIGMA_SCAN_PROBE_NOLOAD          // timing probe (probe builds of tools/ only; results wrong): no 16-bit row loads at all — what would hiding them completely buy?
        return;
#endif
        if constexpr (HI16) asm volatile("buffer_load_short_d16_hi %0, %1, %2, %3 offen" : "+v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
        else dst = buf_ld<IO>(rs, voff, soff);
    };
    auto f32of = [&](const r16_t &v) -> float {
        if constexpr (HI16) return __uint_as_float(v);
        else return to_float<IO>(v);
    };
    auto fence16 = [&]() {
        if constexpr (HI16) {       // (only the registers this instantiation loads into: an unused operand would cost a live register)
            if constexpr (DTP && MODE == 1)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(up[0]), "+v"(up[1]), "+v"(up[2]), "+v"(up[3]));
            else if constexpr (DTP)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(ru[0]), "+v"(ru[1]), "+v"(ru[2]), "+v"(ru[3]), "+v"(rz[0]), "+v"(rz[1]), "+v"(rz[2]), "+v"(rz[3]),
                                                   "+v"(up[0]), "+v"(up[1]), "+v"(up[2]), "+v"(up[3]));
            else if constexpr (MODE == 1)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(ru[0]), "+v"(ru[1]), "+v"(ru[2]), "+v"(ru[3]), "+v"(rd[0]), "+v"(rd[1]), "+v"(rd[2]), "+v"(rd[3]));
            else
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(ru[0]), "+v"(ru[1]), "+v"(ru[2]), "+v"(ru[3]), "+v"(rd[0]), "+v"(rd[1]), "+v"(rd[2]), "+v"(rd[3]),
                                                   "+v"(rz[0]), "+v"(rz[1]), "+v"(rz[2]), "+v"(rz[3]));
        }
    };
    auto fence_acc = [&]() {
        if constexpr (HI16 && ACC) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rac[0]), "+v"(rac[1]), "+v"(rac[2]), "+v"(rac[3]));
    };
    u32x4 xa0 = {0, 0, 0, 0};   // DTP: the dt columns of the tile's 16 x_dbl rows as MFMA A fragments
    u32x4 xa1 = {0, 0, 0, 0};   // (columns 32 .. 63 of the rows: beyond dt_rank they meet zero weights)
    uint32_t rbc;
    float Du[RPT];                 // D * u of this wave's rows (forms without the in-kernel dt_proj)
    float cum = 0.f;               // MODE 1: sum of dt over the chunk (every wave sees all steps in its core loop)
    int zrow[RPT], orow[RPT];      // this wave's 4 entries of the row tables for the current tile: wave-uniform -> SGPRs (s_load)

    auto load_ud = [&](int t) {
        const int r0 = kb + t * LT + wave * RPT;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            if constexpr (!DTP) {       // (DTP: u of the wave's rows only serves D u in the epilogue: fetched with the tile's z rows, see the loop)
                ld16(ru[i], u_rs, lane_off, (r0 + i) * u_ls);
                ld16(rd[i], d_rs, lane_off, (r0 + i) * d_ls);
            }
        }
        if constexpr (DTP) {
            const int row0 = kb + t * LT;
            xa0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xa_voff, row0 * x_ls, 0));
            xa1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, xa_voff + 64, row0 * x_ls, 0));
#pragma unroll
            for (int i = 0; i < RPT; ++i) ld16(up[i], u_rs, up_voff, (row0 + i) * u_ls);       // (the row of the quad in the SCALAR offset: one lane-offset register)
        }
    };
    auto load_bc = [&](int t) {     // all 256 threads, one dword each
        rbc = __builtin_amdgcn_raw_buffer_load_b32(bc_rs, bc_voff, (kb + t * LT) * bc_ls, 0);
    };
    // The wave's 4 entries of each row table are wave-uniform: fetched by the scalar unit (s_load_dword, issued one tile
    // ahead; hipcc will not emit scalar loads here by itself because the kernel's stores might alias the tables) — no
    // VALU slot, no v_readlane.  The results are only touched after tabs_ready()'s s_waitcnt.
    auto load_tabs = [&](int t) {
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int k = kb + t * LT + wave * RPT + i;
            if (TAB) {
                asm volatile("s_load_dword %0, %1, %2" : "=s"(zrow[i]) : "s"(p.z_row_index), "s"(k * 4));
                asm volatile("s_load_dword %0, %1, %2" : "=s"(orow[i]) : "s"(p.out_row_index), "s"(k * 4));
            } else {
                zrow[i] = orow[i] = k;
            }
        }
    };
    auto tabs_ready = [&]() {
        if (TAB)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(zrow[0]), "+s"(zrow[1]), "+s"(zrow[2]), "+s"(zrow[3]),
                                                   "+s"(orow[0]), "+s"(orow[1]), "+s"(orow[2]), "+s"(orow[3]));
    };
    auto prologue = [&](int t) {    // this wave's 4 rows of tile t: dt, dt*u -> LDS; D*u -> registers; B / C of the tile -> LDS
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            if constexpr (!DTP) {
                const float uf = f32of(ru[i]);
                Du[i] = Dv * uf;
                float dv = f32of(rd[i]);
                if (SP) {
                    dv += bias;
                    if (sp_on) dv = softplus20(dv);
                }
                *reinterpret_cast<v2f *>(&s_dtdu[wave * RPT + i][lane][0]) = v2f{dv, dv * uf};
            }
        }
        if constexpr (DTP) {
            mfma_f32x4 dacc = {dbias, dbias, dbias, dbias};
            if constexpr (std::is_same<IO, F16>::value) {      // (fp16 models: the same two products on the f16 form of the instruction)
                dacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mfma_f16x8, xa0), __builtin_bit_cast(mfma_f16x8, wdt0), dacc, 0, 0, 0);
                dacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mfma_f16x8, xa1), __builtin_bit_cast(mfma_f16x8, wdt1), dacc, 0, 0, 0);
            } else {
            dacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mfma_bf16x8, xa0), __builtin_bit_cast(mfma_bf16x8, wdt0), dacc, 0, 0, 0);
            // (the SAME opcode for the second half of k: a v_mfma_f32_16x16x16_bf16 chained behind the 16x16x32 read its C operand before the
            // first product had written all of it — two of every four results wrong on the device; hipcc pads that pair with 3 states)
            dacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mfma_bf16x8, xa1), __builtin_bit_cast(mfma_bf16x8, wdt1), dacc, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < RPT; ++i) {       // D[step 4 kq + i][channel n16]
                // softplus with the reference's pass-through above 20; log2(1 + t) directly: below t = 2^-24 the result is 0 instead
                // of t (absolute error < 6e-8 on a step size — the bf16 delta tensor this replaces carried 2^-9 relative)
                const float xv = dacc[i];
                const float tv = xv * kLog2e;
                float dv = xv > 20.f ? tv : fast_log2(1.f + fast_exp2(tv));          // dt' = dt * log2(e)
                // split first pass: the ROUNDED delta the second pass will read.  It is the tensor dt_proj_softplus_kernel used to write, so it takes
                // that kernel's softplus: the direct log2(1 + t) above loses t against 1 (0 below t = 2^-24, 2^-24 / t relative above it), which a
                // WRITTEN 16-bit delta shows as elements off the correctly rounded value (tests/test_gpu_fwd_fuzz.py: 2.1 % in bf16 with 4 of 192
                // channels below -17)
                if constexpr (!LOG2U) dv = to_float<IO>(from_float<IO>(softplus20_r16(xv)));
                *reinterpret_cast<v2f *>(&s_dtdu[4 * kq + i][wave * 16 + n16][0]) = v2f{dv, dv * f32of(up[i])};
#ifdef ZIGMA_DTP_DEBUG
                if (p.checkpoints) {      // debug: (dt, u') of every element, [batch][step][dim][2]
                    float *dbg = p.checkpoints + ((static_cast<int64_t>(b) * L + kb + t * LT + 4 * kq + i) * p.dim + slab * 64 + wave * 16 + n16) * 2;
                    dbg[0] = dv * kLn2;
                    dbg[1] = f32of(up[i]);
                }
#endif
            }
        }
        if constexpr (LOG2U) {    // two plain multiplies by the wave-uniform (SGPR) factor: as one packed multiply the factor takes a VGPR pair this kernel does not have
            const v2f bc2 = unpack2<IO>(rbc);
            *reinterpret_cast<v2f *>(&s_bc[bc_step][bc_is_c][bc_pair * 2]) = v2f{bc2.x * bc_scale, bc2.y * bc_scale};
        } else {
            *reinterpret_cast<v2f *>(&s_bc[bc_step][bc_is_c][bc_pair * 2]) = unpack2<IO>(rbc);
        }
    };

    // ---- pipeline fill ---------------------------------------------------------------------------
    if (MODE != 1) load_tabs(0);
    load_ud(0);
    load_bc(0);
    fence16();
    prologue(0);
    __syncthreads();

#pragma unroll 1
    for (int t = 0; t < n_tiles; ++t) {
        const bool more = t + 1 < n_tiles;
        int orow_c[RPT];
        // (scalar branches, once per tile: the 16-step core below stays switch-free)
        if (MODE == 0 && p.reset_period > 0 && (t * LT) % p.reset_period == 0) {        // start of an independent sequence (video
            hA = v2f{0.f, 0.f};                                                          // temporal layers: batch = k, seqlen = b * t)
            hB = v2f{0.f, 0.f};
        }
        if constexpr (OUT) {
            if (p.checkpoints) {      // the state before the tile, [batch][slab][tile][state][64 lanes] fp32 (scan_bwd.hip reads it back)
                float *ckp = p.checkpoints + ((static_cast<int64_t>(b) * n_slabs + slab) * (L / LT) + t) * p.dstate * 64;
                ckp[(n0 + 0) * 64 + lane] = hA.x;
                ckp[(n0 + 1) * 64 + lane] = hA.y;
                ckp[(n0 + 2) * 64 + lane] = hB.x;
                ckp[(n0 + 3) * 64 + lane] = hB.y;
            }
        }
        if (prio_rot) {
            const int val = (t + kslot) % (R6 ? 6 : 5);
            base_q = val < 3 ? val : 3;
            set_prio_rt(base_q);
        }
        if (MODE != 1) {
            tabs_ready();
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                ld16(rz[i], z_rs, lane_off, zrow[i] * z_ls);
                if constexpr (DTP) ld16(ru[i], u_rs, lane_off, (kb + t * LT + wave * RPT + i) * u_ls);      // for D u in this tile's epilogue
                orow_c[i] = orow[i];
            }
        }
        if (more) {
            if (MODE != 1) load_tabs(t + 1);        // consumed at the top of the next iteration
            load_ud(t + 1);
            load_bc(t + 1);
        }
        // ---- core(t): 16 steps, operands from LDS one step ahead ------------------------------------------
        // operands PD steps ahead (rotating registers): a wave that runs alone — the oldest one, or the last ones of the kernel —
        // is otherwise bound by the LDS round trip of every step (prefetch distance 1: measured ~2 us per tile for the
        // first-dispatched workgroups against 0.64 us of VALU work); the registers are free (LDS caps the CU at 5 workgroups)
        if constexpr (MODE == 1 && DTP) {      // this wave's 4 rows of the tile's delta (already rounded: the conversion is exact), row layout: 128-byte stores
#pragma unroll
            for (int i = 0; i < RPT; ++i)
                buf_st<IO>(from_float<IO>(s_dtdu[wave * RPT + i][lane][0]), d_rs, lane_off, (kb + t * LT + wave * RPT + i) * d_ls);
        }
        constexpr int PD = R6 ? 1 : DTP ? 2 : 3;      // (the in-kernel dt_proj needs ~13 registers: one step less of operand prefetch keeps 5 waves per SIMD; R6: 80 registers)
        const float *bcq = &s_bc[0][0][n0];
        v4f Bq[PD], Cq[PD];
        v2f ddq[PD];
        // timing probes of round 6 (probe builds of tools/scan_idle_probe.py only; results wrong): the core's operands WITHOUT their LDS reads — an opaque
        // register per step (an empty asm DEFINES it: no move, no hoisting of a loop-invariant product), same VALU instruction stream (checked in the ISA)
#if defined(ZIGMA_SCAN_PROBE_NOBC)
#define ZIGMA_OPND_BC(dst_, addr_) asm volatile("" : "=v"(dst_))
#else
#define ZIGMA_OPND_BC(dst_, addr_) dst_ = *reinterpret_cast<const v4f *>(addr_)
#endif
#if defined(ZIGMA_SCAN_PROBE_NODTDU)
#define ZIGMA_OPND_DD(dst_, addr_) asm volatile("" : "=v"(dst_))
#else
#define ZIGMA_OPND_DD(dst_, addr_) dst_ = *reinterpret_cast<const v2f *>(addr_)
#endif
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            ZIGMA_OPND_BC(Bq[i], bcq + i * 32);
            if (MODE != 1) ZIGMA_OPND_BC(Cq[i], bcq + i * 32 + 16);
            ZIGMA_OPND_DD(ddq[i], &s_dtdu[i][lane][0]);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float yg[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const int s = g * 4 + s4;
                const v4f Bc = Bq[s % PD], Cc = Cq[s % PD];
                const v2f dc = ddq[s % PD];
                if (s + PD < LT) {
                    ZIGMA_OPND_BC(Bq[s % PD], bcq + (s + PD) * 32);
                    if (MODE != 1) ZIGMA_OPND_BC(Cq[s % PD], bcq + (s + PD) * 32 + 16);
                    ZIGMA_OPND_DD(ddq[s % PD], &s_dtdu[s + PD][lane][0]);
                }
                if constexpr (MODE == 1) {
                    // state-only pass: one scheduled asm block per step.  Without the y chain nothing holds hipcc's schedule
                    // together: it hoists a tile's LDS reads and products, spills the prefetch registers and serialises every
                    // tile behind its loads (seen in the ISA of the plain C++ form, as in round 1's first-generation kernel)
#ifdef ZIGMA_SCAN_MODE1_PLAIN_ASM      // (the round-2 form: 16 plain instructions per step in one asm block)
                    step_h_plain(dc.x, dc.y, Bc.x, Bc.y, Bc.z, Bc.w, a2s, hs);
#else
                    // round 6: the packed products of the full pass here too (6 packed + 4 exp instead of 12 plain + 4 exp per step); what kept hipcc from
                    // hoisting a tile's reads and products in round 2 — the asm block — is now a compiler-level fence per step (no instruction)
                    {
                        const v2f dtv1 = {dc.x, dc.x}, duv1 = {dc.y, dc.y};
                        const v2f dA1 = a2A * dtv1, dB1 = a2B * dtv1;
                        const v2f eA1 = {fast_exp2(dA1.x), fast_exp2(dA1.y)}, eB1 = {fast_exp2(dB1.x), fast_exp2(dB1.y)};
                        hA = __builtin_elementwise_fma(eA1, hA, v2f{Bc.x, Bc.y} * duv1);
                        hB = __builtin_elementwise_fma(eB1, hB, v2f{Bc.z, Bc.w} * duv1);
                        asm volatile("" : "+v"(hA), "+v"(hB)::"memory");
                    }
#endif
                    cum += dc.x;
                    yg[s4] = 0.f;
                    continue;
                }
                const v2f dtv = {dc.x, dc.x}, duv = {dc.y, dc.y};
                const v2f dA = a2A * dtv, dB = a2B * dtv;
                const v2f eA = {fast_exp2(dA.x), fast_exp2(dA.y)}, eB = {fast_exp2(dB.x), fast_exp2(dB.y)};
                const v2f bA = v2f{Bc.x, Bc.y} * duv, bB = v2f{Bc.z, Bc.w} * duv;
                hA = __builtin_elementwise_fma(eA, hA, bA);
                hB = __builtin_elementwise_fma(eB, hB, bB);
                // y = C . h as a scalar chain: the packed form needs a horizontal add (pk_mul + pk_fma + add = 5.9 ns against
                // 4 plain ops = 5.4 ns per wave-instruction group, tools/ubench2)
                yg[s4] = __builtin_fmaf(Cc.w, hB.y, __builtin_fmaf(Cc.z, hB.x, __builtin_fmaf(Cc.y, hA.y, Cc.x * hA.x)));
                // step s is finished by wave s / 4; every wave hands over its partial through LDS, its own included (a register
                // path for the own rows costs a branch and four moves per group: measured slower in the ISA count).  One 4-byte
                // write per step: collecting a group's 4 steps for a 16-byte write measured 8 % slower in the replica (tools/ubench3)
                if (!noy) s_y[wave][s][lane] = yg[s4];
                else asm volatile("" ::"v"(yg[s4]));          // (probe: the chain stays alive, nothing is written)
            }
        }
        if constexpr (ACC) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                rac[i] = 0;          // (zeroed HERE, not once at kernel start: the low halves must be clear for the d16_hi load, and a register that lives through the core spills the six-resident form)
                ld16(rac[i], oz_rs, lane_off, orow_c[i] * oz_ls);
            }
        }
        if (!nobar) __syncthreads();
        fence16();          // this tile's z rows and the next tile's u / delta rows (issued a whole core phase ago) have landed
        fence_acc();
        if (MODE == 1) {
            if (more) prologue(t + 1);
            __syncthreads();
            continue;
        }
        // ---- epilogue(t): this wave's rows -------------------------------------------------------------------
        // the short phase between the two barriers holds the whole workgroup up: run it ahead of the other workgroups'
        // core phases (the SIMD arbiter is oldest-first; priority outranks age, MI355X_MICROARCH.md)
        __builtin_amdgcn_s_setprio(3);
        {
            // DTP: y = p0 + p1 + p2 + p3 + D u as three packed-pair adds per two rows and one fma per row, u straight from its load register;
            // otherwise D u was formed in the prologue (u is needed there for dt u) and starts the sum
            auto part = [&](int w) {
                v4f pv;
                if (noy) asm volatile("" : "=v"(pv));        // (probe: the sums stay, their LDS reads go)
                else pv = v4f{s_y[w][wave * RPT][lane], s_y[w][wave * RPT + 1][lane], s_y[w][wave * RPT + 2][lane], s_y[w][wave * RPT + 3][lane]};
                return pv;
            };
            v4f y = {0.f, 0.f, 0.f, 0.f};
            if constexpr (DTP) {
                {
                    y = part(0);
#pragma unroll
                    for (int w = 1; w < NW; ++w) y += part(w);
                }
#pragma unroll
                for (int e = 0; e < RPT; ++e) y[e] = __builtin_fmaf(Dv, f32of(ru[e]), y[e]);
            } else {
                y = v4f{Du[0], Du[1], Du[2], Du[3]};
#pragma unroll
                for (int w = 0; w < NW; ++w) y += part(w);
            }
#pragma unroll
            for (int e = 0; e < RPT; ++e) {
                const float zf = f32of(rz[e]);
                if constexpr (OUT) buf_st<IO>(from_float<IO>(y[e]), o_rs, lane_off, orow_c[e] * o_ls);
                if constexpr (ACC) buf_st<IO>(from_float<IO>(__builtin_fmaf(y[e], ZACT ? zf : silu(zf), f32of(rac[e]))), oz_rs, lane_off, orow_c[e] * oz_ls);
                else buf_st<IO>(from_float<IO>(y[e] * (ZACT ? zf : silu(zf))), oz_rs, lane_off, orow_c[e] * oz_ls);
            }
        }
        if (more) prologue(t + 1);
        if (!nobar) __syncthreads();
        if (prio_rot) set_prio_rt(base_q); else __builtin_amdgcn_s_setprio(0);
    }
    if (stamp && tid == 0) {
        reinterpret_cast<uint64_t *>(p.checkpoints)[2 * blockIdx.x + 1] = now();
    }
    if (MODE == 1) {      // chunk-local carry: decay product exp2(A' * sum(dt)) and the state reached from h = 0
        float *xr = reinterpret_cast<float *>(p.x) + ((static_cast<int64_t>(b) * p.dim + c) * n_chunks + chunk) * 2 * p.dstate;
#ifndef ZIGMA_SCAN_MODE1_PLAIN_ASM
        hs[0] = hA.x; hs[1] = hA.y; hs[2] = hB.x; hs[3] = hB.y;
#endif
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            xr[2 * (n0 + jj)] = fast_exp2(cum * a2s[jj]);
            xr[2 * (n0 + jj) + 1] = hs[jj];
        }
    }
}

// forms and switches: plan_scan() (scan_plan.h)
template <typename IO>
static int launch_tok2(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream) {
    const bool split = plan.form == kScanSplit || plan.form == kScanSplitDtp;
    const dim3 grid(static_cast<unsigned>(scan_slabs(p)), split ? plan.n_chunks : 1), block(256);
    auto run = [&](void (*kernel)(zigma_scan_params_t, int), const zigma_scan_params_t &q) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, q, p.dim / 64);
    };
    if (plan.form == kScanDtp) {
        with_flags([&](auto T, auto Z, auto R6, auto A) { run(scan_tok2_kernel<IO, true, T, Z, 0, false, true, R6, A>, p); },
                   plan.tab, plan.zact, plan.r6, plan.acc);
    } else if (!split) {
        if (plan.out) with_flags([&](auto S, auto T) { run(scan_tok2_kernel<IO, S, T, false, 0, true>, p); }, plan.sp, plan.tab);
        else with_flags([&](auto S, auto T, auto Z) { run(scan_tok2_kernel<IO, S, T, Z, 0>, p); }, plan.sp, plan.tab, plan.zact);
    } else {            // chunk-local states (no gate, no tables) -> running prefixes -> the seeded second pass
        zigma_scan_params_t q = p;
        if (plan.form == kScanSplitDtp) {       // the first pass forms delta (MFMA + softplus) and writes it; the second reads it as a plain delta
            run(scan_tok2_kernel<IO, true, false, false, 1, false, true>, p);
            q.dt_x = nullptr; q.dt_w = nullptr; q.delta_bias = nullptr; q.delta_softplus = 0;
        } else {
            with_flags([&](auto S) { run(scan_tok2_kernel<IO, S, false, false, 1>, p); }, plan.sp);
        }
        launch_combine<IO>(p, plan.n_chunks, stream);
        with_flags([&](auto S, auto T, auto Z) { run(scan_tok2_kernel<IO, S, T, Z, 2>, q); }, plan.sp, plan.tab, plan.zact);
    }
    return check_launch();
}

}  // namespace zigma
