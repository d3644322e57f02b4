// Token-major selective-scan kernel (the hot path).  Included by scan_tok_{bf16,f16,f32}.hip, one I/O element
// type per translation unit so the variants compile in parallel.  See selective_scan.hip for the overview.
//
// Work decomposition (gfx950, wave64):
//   workgroup = one sample x one 64-channel slab, NW waves; wave w owns states 4w..4w+3 of all 64 channels;
//   lane = channel; time runs sequentially inside the lane (no scan, no cross-lane combine).
//   Core, per (element, state): v_mul (dt*A) , v_exp , v_mul_dpp (dt*u*B) , v_fma (h) , v_fmac_dpp (y += C*h).
//   B_l / C_l of a 4-step group live in ONE VGPR each (lane -> (step, state), replicated in every 16-lane row)
//   and reach the FMAs as DPP row_newbcast operands.
// Tile pipeline (LT = 16 steps), two barriers per tile, single-buffered LDS (20 KB):
//   core(t)      : recurrence over the tile; each wave's partial y for the OTHER waves' rows -> LDS, for its
//                  own rows -> registers; B/C registers are re-loaded for tile t+1 right after their last use
//   barrier
//   epilogue(t)  : own rows: y = sum of partials + D*u, SiLU gate, store to row out_row_index[k]
//   prologue(t+1): own rows: softplus(delta + bias), delta*u  -> LDS;  D*u -> registers
//   barrier
// Rows (u, delta, z, out) are addressed as  buffer descriptor + fixed per-lane offset + scalar row offset, so
// every piece of row arithmetic — including the zigzag row tables — runs on the scalar unit.
#pragma once
#include <type_traits>

#include "buffer_io.h"
#include "scan_helpers.h"
#include "scan_plan.h"

namespace zigma {

constexpr int kLT = 16;  // steps per tile
constexpr int kFlagInitFromX = 1;  // internal (params copy of pass 2): every chunk starts from x[chunk - 1]

// EVEN: seqlen % 16 == 0 (no bounds logic anywhere).  HAS_Z: gate and write out_z.  HAS_OUT: write ungated out.
// Sequence split (long sequences, few samples): gridDim.z = number of chunks of chunk_len steps, each workgroup
// runs one chunk.  STATE_ONLY (pass 1): recurrence only, from h = 0, writes the chunk-local carry
// (prod a, h_end) to x; zigma_scan_combine_kernel turns the local carries into running prefixes (the reference's x
// tensor); pass 2 (kFlagInitFromX) starts every chunk from x[chunk - 1] and produces the outputs.
template <typename IO, int NW, bool EVEN, bool HAS_Z, bool HAS_OUT, bool STATE_ONLY>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 5 : 4) void scan_tok_kernel(const zigma_scan_params_t p) {
    constexpr int LT = kLT, RPT = LT / NW, NG = LT / 4;
    static_assert(RPT % 4 == 0, "every wave finishes whole 4-step groups");
    using io_t = typename IO::raw;   // B/C share the activation dtype in this path
    constexpr int ES = static_cast<int>(sizeof(io_t));
    __shared__ __attribute__((aligned(16))) float s_spdu[LT / 2][64][4];     // [step pair][channel][dt0, dtu0, dt1, dtu1]
    __shared__ __attribute__((aligned(16))) float s_y[NW - 1][NG][64][4];    // foreign partial y, [slot][group][channel][step]
    __shared__ float s_cum[NW][64];                                          // per-wave sums of dt (carry output only)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int c = blockIdx.x * 64 + lane;
    const int L = p.seqlen;
    const int n0 = wave * 4;
    const bool init_from_x = (p.flags & kFlagInitFromX) != 0;
    const bool HAS_X = p.x != nullptr && !init_from_x;          // pass 2 only reads x
    const int chunk_len = p.chunk_len > 0 ? p.chunk_len : 2048;
    const int n_chunks = (L + chunk_len - 1) / chunk_len;
    const bool split = gridDim.z > 1;
    const int chunk = blockIdx.z;
    const int kb = split ? chunk * chunk_len : 0;                  // first step of this workgroup
    const int k_end = split ? (kb + chunk_len < L ? kb + chunk_len : L) : L;

    float a2[4], h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a2[j] = reinterpret_cast<const float *>(p.A)[c * p.A_d_stride + (n0 + j) * p.A_dstate_stride] * kLog2e;
        h[j] = 0.f;
    }
    if (init_from_x && chunk > 0) {
        const float *xr = reinterpret_cast<const float *>(p.x) + ((static_cast<int64_t>(b) * p.dim + c) * n_chunks + chunk - 1) * 2 * p.dstate;
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = xr[2 * (n0 + j) + 1];
    }
    const float Dv = p.D ? reinterpret_cast<const float *>(p.D)[c] : 0.f;
    const float bias = p.delta_bias ? reinterpret_cast<const float *>(p.delta_bias)[c] : 0.f;
    const bool sp_on = p.delta_softplus != 0;

    const unsigned lane_off = static_cast<unsigned>(c) * ES;
    const int u_ls = static_cast<int>(p.u_l_stride) * ES, d_ls = static_cast<int>(p.delta_l_stride) * ES;
    const int z_ls = static_cast<int>(p.z_l_stride) * ES, o_ls = static_cast<int>(p.out_l_stride) * ES;
    const int oz_ls = static_cast<int>(p.out_z_l_stride) * ES;
    const int B_ls = static_cast<int>(p.B_l_stride) * ES, C_ls = static_cast<int>(p.C_l_stride) * ES;
    const int64_t Lm1 = L - 1, dimb = static_cast<int64_t>(p.dim) * ES;
    const rsrc_t u_rs = make_rsrc(reinterpret_cast<const io_t *>(p.u) + b * p.u_batch_stride, Lm1 * u_ls + dimb);
    const rsrc_t d_rs = make_rsrc(reinterpret_cast<const io_t *>(p.delta) + b * p.delta_batch_stride, Lm1 * d_ls + dimb);
    const rsrc_t z_rs = make_rsrc(reinterpret_cast<const io_t *>(p.z) + b * p.z_batch_stride, HAS_Z ? Lm1 * z_ls + dimb : 0);
    const rsrc_t o_rs = make_rsrc(reinterpret_cast<const io_t *>(p.out) + b * p.out_batch_stride, HAS_OUT ? Lm1 * o_ls + dimb : 0);
    const rsrc_t oz_rs = make_rsrc(reinterpret_cast<const io_t *>(p.out_z) + b * p.out_z_batch_stride, HAS_Z ? Lm1 * oz_ls + dimb : 0);
    const rsrc_t B_rs = make_rsrc(reinterpret_cast<const io_t *>(p.B) + b * p.B_batch_stride,
                                  Lm1 * B_ls + ((p.dstate - 1) * p.B_dstate_stride + 1) * ES);
    const rsrc_t C_rs = make_rsrc(reinterpret_cast<const io_t *>(p.C) + b * p.C_batch_stride,
                                  Lm1 * C_ls + ((p.dstate - 1) * p.C_dstate_stride + 1) * ES);
    // B/C group register: lane -> (step s = (lane & 15) >> 2, state j = lane & 3)
    const int bc_s = (lane & 15) >> 2;
    const unsigned B_lane = static_cast<unsigned>((n0 + (lane & 3)) * static_cast<int>(p.B_dstate_stride) * ES);
    const unsigned C_lane = static_cast<unsigned>((n0 + (lane & 3)) * static_cast<int>(p.C_dstate_stride) * ES);
    const unsigned B_lane_s = B_lane + static_cast<unsigned>(bc_s * B_ls), C_lane_s = C_lane + static_cast<unsigned>(bc_s * C_ls);
    const bool has_ztab = HAS_Z && p.z_row_index != nullptr, has_otab = p.out_row_index != nullptr;
    const int n_tiles = (k_end - kb + LT - 1) / LT;

    io_t ru[RPT], rd[RPT], rz[RPT], rb[NG], rc[NG];   // prefetched operands, RAW (widened where consumed)
    float Du[RPT];                                     // D * u of the rows this wave finishes
    int zi = 0, oi = 0;                                // this wave's entries of the row tables (lane i -> row i)
    float cum = 0.f;

    auto clampk = [&](int k) { return EVEN ? k : (k < L ? k : L - 1); };
    auto load_ud = [&](int t) {                        // u, delta rows of this wave in tile t
        const int r0 = kb + t * LT + wave * RPT;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int kk = clampk(r0 + i);
            ru[i] = buf_ld<IO>(u_rs, lane_off, kk * u_ls);
            rd[i] = buf_ld<IO>(d_rs, lane_off, kk * d_ls);
        }
    };
    auto load_bc_group = [&](int t, int g) {           // B/C of 4-step group g of tile t
        if (EVEN || kb + (t + 1) * LT <= L) {
            const int kg = kb + t * LT + g * 4;
            rb[g] = buf_ld<IO>(B_rs, B_lane_s, kg * B_ls);
            rc[g] = buf_ld<IO>(C_rs, C_lane_s, kg * C_ls);
        } else {                                       // ragged last tile: clamp per lane (those steps carry dt*u = 0)
            const int k = clampk(kb + t * LT + g * 4 + bc_s);
            rb[g] = buf_ld<IO>(B_rs, B_lane + static_cast<unsigned>(k * B_ls), 0);
            rc[g] = buf_ld<IO>(C_rs, C_lane + static_cast<unsigned>(k * C_ls), 0);
        }
    };
    auto load_tab = [&](const int32_t *tab, int t) {   // lane i (mod RPT) <- table entry of this wave's row i in tile t
        const int k = clampk(kb + t * LT + wave * RPT + (lane & (RPT - 1)));
        return tab[k];
    };
    // prologue of tile t: softplus, dt*u -> LDS (one 16-byte write per pair of rows), D*u -> registers
    auto prologue = [&](int t) {
#pragma unroll
        for (int i = 0; i < RPT; i += 2) {
            v4f w;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float uf = to_float<IO>(ru[i + e]);
                float dv = to_float<IO>(rd[i + e]) + bias;
                if (sp_on) dv = softplus20(dv);
                float du = dv * uf;
                if (!EVEN && kb + t * LT + wave * RPT + i + e >= L) { dv = 0.f; du = 0.f; }  // identity step
                Du[i + e] = Dv * uf;
                cum += dv;   // running sum of dt over THIS wave's rows (the carry needs the sum over all rows)
                if (e == 0) { w.x = dv; w.y = du; } else { w.z = dv; w.w = du; }
            }
            *reinterpret_cast<v4f *>(&s_spdu[(wave * RPT + i) >> 1][lane][0]) = w;
        }
    };

#define ZIGMA_STEP(S, dv, du, Bf, Cf, yv)                                        \
    {                                                                            \
        const float e0 = fast_exp2((dv) * a2[0]), e1 = fast_exp2((dv) * a2[1]);  \
        const float e2 = fast_exp2((dv) * a2[2]), e3 = fast_exp2((dv) * a2[3]);  \
        h[0] = __builtin_fmaf(e0, h[0], row_bcast<(S) * 4 + 0>(Bf) * (du));      \
        h[1] = __builtin_fmaf(e1, h[1], row_bcast<(S) * 4 + 1>(Bf) * (du));      \
        h[2] = __builtin_fmaf(e2, h[2], row_bcast<(S) * 4 + 2>(Bf) * (du));      \
        h[3] = __builtin_fmaf(e3, h[3], row_bcast<(S) * 4 + 3>(Bf) * (du));      \
        yv = row_bcast<(S) * 4 + 0>(Cf) * h[0];                                  \
        fmac_bcast<(S) * 4 + 1>(yv, Cf, h[1]);                                   \
        fmac_bcast<(S) * 4 + 2>(yv, Cf, h[2]);                                   \
        fmac_bcast<(S) * 4 + 3>(yv, Cf, h[3]);                                   \
    }

    // ---- pipeline fill ---------------------------------------------------------------------------
    if (!STATE_ONLY && has_ztab) zi = load_tab(p.z_row_index, 0);
    load_ud(0);
#pragma unroll
    for (int g = 0; g < NG; ++g) load_bc_group(0, g);
    prologue(0);
    __syncthreads();

#pragma unroll 1
    for (int t = 0; t < n_tiles; ++t) {
        const bool more = t + 1 < n_tiles;
        // ---- issue this tile's long-latency loads: z rows + out row table of tile t, u / delta of tile t+1 ----
        if (!STATE_ONLY && has_otab) oi = load_tab(p.out_row_index, t);
        if constexpr (HAS_Z && !STATE_ONLY) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int zrow = has_ztab ? __builtin_amdgcn_readlane(zi, i) : clampk(kb + t * LT + wave * RPT + i);
                rz[i] = buf_ld<IO>(z_rs, lane_off, zrow * z_ls);
            }
            if (has_ztab && more) zi = load_tab(p.z_row_index, t + 1);
        }
        if (more) load_ud(t + 1);

        if (p.reset_period > 0 && (kb + t * LT) % p.reset_period == 0) {   // start of an independent sequence
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = 0.f;
        }
        if constexpr (HAS_Z && HAS_OUT && !STATE_ONLY) {     // training forward: state before the tile -> checkpoint buffer
            if (p.checkpoints) {
                const int64_t n_tiles_all = (L + LT - 1) / LT;
                float *ckp = p.checkpoints + ((static_cast<int64_t>(b) * gridDim.x + blockIdx.x) * n_tiles_all + kb / LT + t) * p.dstate * 64;
#pragma unroll
                for (int j = 0; j < 4; ++j) ckp[(n0 + j) * 64 + lane] = h[j];
            }
        }
        // ---- core(t) ----------------------------------------------------------------------------------
        float yown[RPT];
        v4f q0 = *reinterpret_cast<const v4f *>(&s_spdu[0][lane][0]);
        v4f q1 = *reinterpret_cast<const v4f *>(&s_spdu[1][lane][0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            v4f n0v = q0, n1v = q1;
            if (g + 1 < NG) {   // LDS reads of the next group fly under this group's math
                n0v = *reinterpret_cast<const v4f *>(&s_spdu[g * 2 + 2][lane][0]);
                n1v = *reinterpret_cast<const v4f *>(&s_spdu[g * 2 + 3][lane][0]);
            }
            float Bf = to_float<IO>(rb[g]);
            float Cf = to_float<IO>(rc[g]);
            if constexpr (STATE_ONLY) dpp_settle(Bf); else dpp_settle(Cf);
            float y0, y1, y2, y3;
            if constexpr (STATE_ONLY) {
                y0 = y1 = y2 = y3 = 0.f;
                step_h<0>(q0.x, q0.y, Bf, a2, h);
                step_h<1>(q0.z, q0.w, Bf, a2, h);
                step_h<2>(q1.x, q1.y, Bf, a2, h);
                step_h<3>(q1.z, q1.w, Bf, a2, h);
            } else {
            ZIGMA_STEP(0, q0.x, q0.y, Bf, Cf, y0)
            ZIGMA_STEP(1, q0.z, q0.w, Bf, Cf, y1)
            ZIGMA_STEP(2, q1.x, q1.y, Bf, Cf, y2)
            ZIGMA_STEP(3, q1.z, q1.w, Bf, Cf, y3)
            }
            if (more) load_bc_group(t + 1, g);         // the registers are free again: refill for the next tile
            const int owner = (g * 4) / RPT;           // rows 4g..4g+3 are finished by this wave
            if constexpr (STATE_ONLY) {
            } else if (owner == wave) {
                const int o = (g * 4) % RPT;
                yown[o] = y0; yown[o + 1] = y1; yown[o + 2] = y2; yown[o + 3] = y3;
            } else {
                const int slot = wave < owner ? wave : wave - 1;
                *reinterpret_cast<v4f *>(&s_y[slot][g][lane][0]) = v4f{y0, y1, y2, y3};
            }
            q0 = n0v;
            q1 = n1v;
        }
        // carries at chunk ends.  chunk_len is a multiple of LT (dispatcher), so a chunk end is a tile end; the
        // sequence end may fall inside the last tile, whose padded steps are identities.  The product of the
        // decay factors is exp2(A * sum(dt)); each wave holds the dt of its own rows only, so the sum is
        // completed through LDS (s_y is free here only after the barrier -> use a dedicated small buffer).
        bool carry = false;
        int chunk_idx = chunk;
        if (HAS_X) {
            const int k_next = kb + (t + 1) * LT;
            carry = !more || (!split && k_next % chunk_len == 0);
            if (!split) chunk_idx = ((k_next <= L ? k_next : L) - 1) / chunk_len;
            if (carry) s_cum[wave][lane] = cum;
        }
        __syncthreads();
        if (carry) {   // uniform over the workgroup
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) tot += s_cum[w][lane];
            float *xr = reinterpret_cast<float *>(p.x) + ((static_cast<int64_t>(b) * p.dim + c) * n_chunks + chunk_idx) * 2 * p.dstate;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xr[2 * (n0 + j)] = fast_exp2(tot * a2[j]);
                xr[2 * (n0 + j) + 1] = h[j];
            }
        }
        if constexpr (STATE_ONLY) {
            if (more) prologue(t + 1);
            __syncthreads();
            continue;
        }

        // ---- epilogue(t): this wave's rows ---------------------------------------------------------------
#pragma unroll
        for (int i4 = 0; i4 < RPT; i4 += 4) {
            const int gq = (wave * RPT + i4) >> 2;
            v4f y = {yown[i4] + Du[i4], yown[i4 + 1] + Du[i4 + 1], yown[i4 + 2] + Du[i4 + 2], yown[i4 + 3] + Du[i4 + 3]};
#pragma unroll
            for (int w = 0; w < NW - 1; ++w) y += *reinterpret_cast<const v4f *>(&s_y[w][gq][lane][0]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = kb + t * LT + wave * RPT + i4 + e;
                if (EVEN || k < L) {
                    const int orow = has_otab ? __builtin_amdgcn_readlane(oi, i4 + e) : k;
                    if constexpr (HAS_OUT) buf_st<IO>(from_float<IO>(y[e]), o_rs, lane_off, orow * o_ls);
                    if constexpr (HAS_Z) buf_st<IO>(from_float<IO>(y[e] * silu(to_float<IO>(rz[i4 + e]))), oz_rs, lane_off, orow * oz_ls);
                }
            }
        }
        // ---- prologue(t+1) -----------------------------------------------------------------------------------
        if (more) prologue(t + 1);
        __syncthreads();
    }
#undef ZIGMA_STEP
}

// local carries (prod a over the chunk, h_end from h = 0)  ->  running prefixes, in place (the reference's x tensor)
template <typename IO>   // templated only so that every per-dtype TU owns its instance
__global__ void zigma_scan_combine_kernel(float *x, int64_t rows, int n_chunks, int dstate) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;   // (b, d, n)
    if (i >= rows * dstate) return;
    float *xr = x + (i / dstate) * n_chunks * 2 * dstate + 2 * (i % dstate);
    float P = 1.f, H = 0.f;
    for (int c = 0; c < n_chunks; ++c) {
        const float pc = xr[c * 2 * dstate], sc = xr[c * 2 * dstate + 1];
        H = pc * H + sc;
        P *= pc;
        xr[c * 2 * dstate] = P;
        xr[c * 2 * dstate + 1] = H;
    }
}

// calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for the run-time switches b0, b1, ...: one instantiation per combination
template <typename F> static void with_flags(F &&f) { f(); }
template <typename F, typename... R> static void with_flags(F &&f, bool b, R... rest) {
    if (b) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

template <typename IO>
static void launch_combine(const zigma_scan_params_t &p, int n_chunks, hipStream_t stream) {
    const int64_t rows = static_cast<int64_t>(p.batch) * p.dim;
    hipLaunchKernelGGL(zigma_scan_combine_kernel<IO>, dim3(static_cast<unsigned>((rows * p.dstate + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<float *>(p.x), rows, n_chunks, p.dstate);
}

// sequence split: chunk-local carries (pass 1) -> running prefixes -> every chunk from its prefix (pass 2, which writes the outputs)
template <typename IO>
static int launch_tok(const zigma_scan_params_t &p, const ScanPlan &plan, hipStream_t stream) {
    const bool split = plan.form == kScanSplit;
    with_flags([&](auto N4, auto E) {
        constexpr int NW = N4 ? 4 : 2;
        const dim3 grid(p.dim / 64, p.batch, split ? plan.n_chunks : 1), block(64 * NW);
        zigma_scan_params_t q = p;
        if (split) {
            hipLaunchKernelGGL((scan_tok_kernel<IO, NW, E, false, false, true>), grid, block, 0, stream, p);
            launch_combine<IO>(p, plan.n_chunks, stream);
            q.flags |= kFlagInitFromX;
        }
        if (plan.z && plan.out) hipLaunchKernelGGL((scan_tok_kernel<IO, NW, E, true, true, false>), grid, block, 0, stream, q);
        else if (plan.z) hipLaunchKernelGGL((scan_tok_kernel<IO, NW, E, true, false, false>), grid, block, 0, stream, q);
        else hipLaunchKernelGGL((scan_tok_kernel<IO, NW, E, false, true, false>), grid, block, 0, stream, q);
    }, plan.nw == 4, plan.even);
    return check_launch();
}

}  // namespace zigma
