// ntt_mulk.hpp -- poly_mul_ntt_k: k shared NTT-domain rows times a batch,
//   out[b][i] = a_i * y_b (+ add[b][i])  mod (x^n + 1, q),  0 <= i < k,
// one launch (qTESLA's t_i = a_i y + e_i over its public polynomials).
//
// Modelled on the b-hat branch of k_poly_mul (ntt_device.hpp): a work unit
// (one wave for n = 2048, a half-wave per polynomial for n = 1024) loads y
// once, transforms it completely and keeps y-hat, reduced to [0, 2q), in 32
// registers.  Then, per row i: load a_i-hat with the b-hat mapping (pass-2
// register j holds index brv5(j)*S + lane), Montgomery product into a working
// copy, inverse transform, store.  k + 1 transforms of work per y instead of
// the 2k of k poly_mul_ntt calls, y read once, no broadcast copies of a-hat
// (k*n*4 <= 64 KiB, read from global memory by every unit: it stays in L2).
//
// Registers: y-hat (32) + working copy (32) + the row's a-hat loads or its
// addend (32) are live together, past the 128 VGPRs of 4 waves/SIMD; the
// kernel is built for 3 waves/SIMD (<= 168 VGPRs, no spills).  A workgroup
// is 6 waves (48 KiB of transpose buffers + 31.5 KiB of twiddle tables), two
// workgroups per CU: 12 waves/CU = 3 waves/SIMD, and the CU never drains to
// start the next workgroup.
//
// add may equal out (accumulate in place), safe by construction: the words
// out[b][i][.] that a lane stores are exactly the words add[b][i][.] it
// loaded, at the same offsets, and all 32 of those loads are issued before
// the lane's first store of that row; no other lane, wave or row touches
// them.  y and a-hat never overlap out (rejected by the entry point), hence
// __restrict__; add is only read and may overlap them.
//
// Small batches: blockIdx.y strides over the rows (row i = blockIdx.y,
// blockIdx.y + gridDim.y, ...), every y-slice recomputing y-hat; the entry
// point launches gridDim.y = k up to the measured switch batch
// (mulk_split_max) and 1 above it.
#pragma once
#include "ntt_device.hpp"

namespace qntt {

constexpr int MULK_WAVES = 6;
constexpr int MULK_WG = MULK_WAVES * 64;
constexpr int MULK_WAVES_PER_SIMD = 3;
constexpr int MULK_LDS_WORDS = MULK_WAVES * XPOSE_WORDS + 2 * TW2_WORDS;
static_assert(2 * MULK_LDS_WORDS * 4 <= 160 * 1024, "two workgroups per CU (160 KiB LDS)");
static_assert(2 * MULK_WAVES == 4 * MULK_WAVES_PER_SIMD, "two workgroups fill the CU's four SIMDs");
constexpr int MULK_K_MAX = 8;   // NTT_MUL_K_MAX
// Units a wave walks per workgroup, at most (launch_shape's chunk).  A unit is
// k + 1 transforms long, so 4 amortise the table prologue as 16 do in the
// other kernels, and the shorter workgroups leave a smaller idle tail: against
// 16, -10 % (p-III, k = 5) / -12 % (p-I, k = 4) at 2^17 and -2 % at 2^20; 2 is
// another 2-8 % faster from 2^15 to 2^17 but 1-2 % slower than 4 at 2^20
// (poly_mul_ntt_k).
#ifndef MULK_PPW_MAX
#define MULK_PPW_MAX 4
#endif

// Largest batch whose rows are spread over gridDim.y = k (one forward per
// row instead of one per y, but k times the waves); 0: never.  The largest
// batch of a half-octave sweep at which that shape was the faster one; the
// crossover was the same at k = 2, 4, 5 and 8 (poly_mul_ntt_k).
// A/B builds only: MULK_SPLIT_FORCE 0 never splits, 1 always does.
#ifdef MULK_SPLIT_FORCE
constexpr size_t mulk_split_max(int) { return MULK_SPLIT_FORCE ? (size_t)0x7FFFFFFF : 0; }
#else
constexpr size_t kMulkSplitMax[3] = {1448, 1448, 724};   // ref, p-I, p-III
constexpr size_t mulk_split_max(int ps) { return kMulkSplitMax[ps]; }
#endif

template <int PS, bool ADD>
__global__ __launch_bounds__(MULK_WG, MULK_WAVES_PER_SIMD) void k_poly_mul_k(const uint32_t *__restrict__ y,
                                                                             const uint32_t *__restrict__ ahat,
                                                                             const uint32_t *add, uint32_t *out,
                                                                             uint32_t npoly, uint32_t k, uint32_t ppw)
{
    using P = typename PSel<PS>::T;
    using LT = Lane<P>;
    constexpr int SWO = TW2_ENTRIES * 64;   // bit-5 pairs' offset (pairs)
    __shared__ __attribute__((aligned(16))) uint32_t lds[MULK_LDS_WORDS];
    uint2 *ftw2 = reinterpret_cast<uint2 *>(lds + MULK_WAVES * XPOSE_WORDS);
    uint2 *itw2 = ftw2 + TW2_WORDS / 2;
    fill_tw2<PS, false, MULK_WG>(ftw2);
    fill_tw2<PS, true, MULK_WG>(itw2);
    __syncthreads();
    const LT L;
    uint32_t *buf = lds + (threadIdx.x >> 6) * XPOSE_WORDS;

    const uint32_t nunits = (npoly + LT::UPW - 1) / LT::UPW;
    const uint32_t kn = k * P::N;   // words between two polynomials of out / add (<= 2^14)
    uint32_t u = blockIdx.x * (MULK_WAVES * ppw) + wave_id();
#pragma unroll 1
    for (uint32_t it = 0; it < ppw; ++it, u += MULK_WAVES) {   // dispatch-ordered chunk (see chunk_loop)
        if (u >= nunits) break;
        const bool valid = LT::BIG || L.poly(u) < npoly;
        uint32_t yh[32];
        load32(yh, y + LT::unit_base(u) + L.col_load(u, npoly), [](int j) { return LT::S * j; });
        fwd_pass1<PS, P>(yh, L.h, ftw2 + SWO + opaque_zero());
        lds_p1_to_p2<P>(yh, buf, L);
        fwd_pass2<P>(yh, ftw2 + opaque_zero(), L.lane);
#pragma unroll
        for (int j = 0; j < 32; ++j) yh[j] = csub<P::Q2>(yh[j]);   // [0, 4q) -> [0, 2q), once for all rows
        // out / add: the unit's polynomials lie k*n words apart (n = 1024: the
        // two halves of the wave), row i another i*n words in.  Scalar 64-bit
        // base per (unit, row) + 32-bit lane offset.  The second half of an
        // odd batch's last n = 1024 unit loads its addend from the first
        // (valid) polynomial and stores nothing.
        const size_t ubase = (size_t)u * LT::UPW * kn;
        const uint32_t ooff = LT::BIG ? L.brl : L.h * kn + L.brl;
        const uint32_t aoff = valid ? ooff : L.brl;
#pragma unroll 1
        for (uint32_t i = blockIdx.y; i < k; i += gridDim.y) {
            const uint32_t *pa = ahat + (size_t)i * P::N + L.brl;
            uint32_t r[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) r[j] = mont_mul<P>(yh[j], csub<P::Q2>(pa[LT::S * brv5(j)]));   // a-hat < 2q
            inv_pass2<P>(r, itw2 + opaque_zero(), L.lane);
            // n = 2048 with an addend: transpose addresses recomputed from an
            // opaque lane (hoisted out of the row loop they pin ~25 VGPRs: 2 spilled)
            constexpr bool HOIST = !(ADD && LT::BIG);
            lds_p2_to_p1<P>(r, buf, HOIST ? L : LT(opaque_lane()));
            const size_t rbase = ubase + (size_t)i * P::N;
            uint32_t ad[ADD ? 32 : 1];
            if constexpr (ADD) load32(ad, add + rbase + aoff, [](int j) { return LT::S * j; });
            uint32_t *po = out + rbase + ooff;
            // stores interleaved with the last stage (see inv_pass1); with an
            // addend the last stage leaves [0, 2q) and the sum (< 4q) is
            // reduced to canonical form here
            auto emit = [&](int j, uint32_t v) {
                if constexpr (ADD) v = canon4<P>(v + ad[j]);
                if (valid) st_out(po + LT::S * j, v);
            };
            inv_pass1_head<P>(r, L.h, tw_base<PS, true>(), itw2 + SWO + opaque_zero());
            inv_last_scaled<P, !ADD, P::NINV_R, P::C1_R>(r, emit);
        }
    }
}

}  // namespace qntt
