// ntt_mulkl.hpp -- poly_mul_ntt_kl: a k x l matrix of shared NTT-domain
// polynomials times l batches, accumulated in the NTT domain,
//   out[b][i] = sum_{j<l} a_ij * y_j[b] (+ add[b][i])  mod (x^n + 1, q),  0 <= i < k,
// one launch (qTESLA's verification, w_i = a_i z - t_i c: rows [a_i-hat,
// q - t_i-hat], inputs [z, c]).  The NTT is linear, so the l products of a row
// are summed before its one inverse transform: k + l transforms per b.
//
// k_poly_mul_k (ntt_mulk.hpp) with l forward transforms kept in registers:
// the same work unit (a wave per n = 2048 polynomial, a half-wave per
// n = 1024 polynomial), twiddle tables in LDS, row loop, addend handling and
// store order (add == out is safe for the reason given there), chunked walk
// and gridDim.y row split.  Per row the point values are
//   REDC(sum_j y_j-hat * a_ij-hat):
// the l 64-bit products (each < 4q^2) are summed (v_mad_u64_u32) and reduced
// once; l * 4q^2 < 2^64, and (T + m q) / 2^32 < l * 4q^2 / 2^32 + q, which is
// below 2q where 4 l q < 2^32 (ref, p-I) and below 4q otherwise (p-III: one
// conditional subtraction).  So inv_pass2 gets [0, 2q), the range it has in
// every other kernel (DESIGN.md "lazy reduction bounds").
//
// Registers: l x 32 of y-hat + the working copy (32) + the row's a-hat loads
// or its addend are live together: at l = 2 past the 168 VGPRs of 3
// waves/SIMD, so the kernel is built for 2 waves/SIMD (<= 256 VGPRs, no
// spills).  A workgroup is 4 waves (32 KiB of transpose buffers + 31.5 KiB of
// tables), two workgroups per CU: 8 waves/CU = 2 waves/SIMD, and the CU never
// drains to start the next workgroup.
//
// The inputs' base pointers travel by value (MulKLIn): a caller's batches
// are read where they lie.  They may overlap each other and add; none
// overlaps out (rejected by the entry point).
//
// Also here: k_poly_scatter, sparse (position, value) lists -> dense
// polynomials (qTESLA's challenge c).
#pragma once
#include "ntt_mulk.hpp"

namespace qntt {

constexpr int MULKL_L_MAX = 2;   // NTT_MUL_L_MAX
constexpr int MULKL_WAVES = 4;
constexpr int MULKL_WG = MULKL_WAVES * 64;
constexpr int MULKL_WAVES_PER_SIMD = 2;
constexpr int MULKL_LDS_WORDS = MULKL_WAVES * XPOSE_WORDS + 2 * TW2_WORDS;
static_assert(2 * MULKL_LDS_WORDS * 4 <= 160 * 1024, "two workgroups per CU (160 KiB LDS)");
static_assert(2 * MULKL_WAVES == 4 * MULKL_WAVES_PER_SIMD, "two workgroups fill the CU's four SIMDs");
// Units a wave walks per workgroup, at most (see MULK_PPW_MAX: a unit is
// k + l transforms long).
#ifndef MULKL_PPW_MAX
#define MULKL_PPW_MAX 4
#endif

// Largest batch whose rows are spread over gridDim.y = k (l forwards per row
// instead of l per b, but k times the waves); 0: never.  l = 2; the largest
// batch of a half-octave sweep at which that shape was the faster one, at the
// sets' own k (4 / 5) -- n = 1024: the same at k = 8; n = 2048: 512 at k = 2
// (tools/mulk_split_sweep.py --kl, profiles/mulkl/).
// A/B builds only: MULKL_SPLIT_FORCE 0 never splits, 1 always does.
#ifdef MULKL_SPLIT_FORCE
constexpr size_t mulkl_split_max(int) { return MULKL_SPLIT_FORCE ? (size_t)0x7FFFFFFF : 0; }
#else
constexpr size_t kMulklSplitMax[3] = {1024, 1024, 362};   // ref, p-I, p-III
constexpr size_t mulkl_split_max(int ps) { return kMulklSplitMax[ps]; }
#endif

template <int L> struct MulKLIn {
    const uint32_t *y[L];
};

// REDC(sum_t y[t] * a[t]), y[t], a[t] in [0, 2q): the sum times 2^-32 mod q, in [0, 2q)
template <class P, int L>
__device__ __forceinline__ uint32_t mont_dot(const uint32_t (&y)[L], const uint32_t (&a)[L])
{
    static_assert((uint64_t)P::Q2 * P::Q2 <= ~0ull / L, "the sum fits 64 bits");
    static_assert(4ull * L * P::Q < 3ull << 32, "REDC output below 4q");
    uint64_t t = (uint64_t)y[0] * a[0];
#pragma unroll
    for (int i = 1; i < L; ++i) t += (uint64_t)y[i] * a[i];
    const uint32_t lo = (uint32_t)t;
    const uint32_t m = lo * P::QNEG;
    const uint32_t v = (uint32_t)(t >> 32) + __umulhi(m, P::Q) + (lo != 0u ? 1u : 0u);   // < L*4q^2 / 2^32 + q
    return 4ull * L * P::Q < 1ull << 32 ? v : csub<P::Q2>(v);
}

template <int PS, int L, bool ADD>
__global__ __launch_bounds__(MULKL_WG, MULKL_WAVES_PER_SIMD) void k_poly_mul_kl(const MulKLIn<L> in,
                                                                                const uint32_t *__restrict__ ahat,
                                                                                const uint32_t *add, uint32_t *out,
                                                                                uint32_t npoly, uint32_t k, uint32_t ppw)
{
    using P = typename PSel<PS>::T;
    using LT = Lane<P>;
    constexpr int SWO = TW2_ENTRIES * 64;   // bit-5 pairs' offset (pairs)
    __shared__ __attribute__((aligned(16))) uint32_t lds[MULKL_LDS_WORDS];
    uint2 *ftw2 = reinterpret_cast<uint2 *>(lds + MULKL_WAVES * XPOSE_WORDS);
    uint2 *itw2 = ftw2 + TW2_WORDS / 2;
    fill_tw2<PS, false, MULKL_WG>(ftw2);
    fill_tw2<PS, true, MULKL_WG>(itw2);
    __syncthreads();
    const LT Ln;
    uint32_t *buf = lds + (threadIdx.x >> 6) * XPOSE_WORDS;

    const uint32_t nunits = (npoly + LT::UPW - 1) / LT::UPW;
    const uint32_t kn = k * P::N;   // words between two polynomials of out / add (<= 2^14)
    uint32_t u = blockIdx.x * (MULKL_WAVES * ppw) + wave_id();
#pragma unroll 1
    for (uint32_t it = 0; it < ppw; ++it, u += MULKL_WAVES) {   // dispatch-ordered chunk (see chunk_loop)
        if (u >= nunits) break;
        const bool valid = LT::BIG || Ln.poly(u) < npoly;
        uint32_t yh[L][32];
#pragma unroll
        for (int t = 0; t < L; ++t) {
            load32(yh[t], in.y[t] + LT::unit_base(u) + Ln.col_load(u, npoly), [](int j) { return LT::S * j; });
            fwd_pass1<PS, P>(yh[t], Ln.h, ftw2 + SWO + opaque_zero());
            // transpose addresses recomputed from an opaque lane here and in the
            // row loop: kept live across the unit they pin ~25 VGPRs (n = 2048: 7 spilled)
            lds_p1_to_p2<P>(yh[t], buf, LT(opaque_lane()));
            fwd_pass2<P>(yh[t], ftw2 + opaque_zero(), Ln.lane);
#pragma unroll
            for (int j = 0; j < 32; ++j) yh[t][j] = csub<P::Q2>(yh[t][j]);   // [0, 4q) -> [0, 2q), once for all rows
        }
        // out / add addressing as in k_poly_mul_k
        const size_t ubase = (size_t)u * LT::UPW * kn;
        const uint32_t ooff = LT::BIG ? Ln.brl : Ln.h * kn + Ln.brl;
        const uint32_t aoff = valid ? ooff : Ln.brl;
#pragma unroll 1
        for (uint32_t i = blockIdx.y; i < k; i += gridDim.y) {
            const uint32_t *pa = ahat + (size_t)i * (L * P::N) + Ln.brl;   // row i: a_i0-hat .. a_i(L-1)-hat, n words each
            uint32_t r[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                uint32_t yv[L], av[L];
#pragma unroll
                for (int t = 0; t < L; ++t) {
                    yv[t] = yh[t][j];
                    av[t] = csub<P::Q2>(pa[t * P::N + LT::S * brv5(j)]);   // a-hat < 2q
                }
                r[j] = mont_dot<P, L>(yv, av);
            }
            inv_pass2<P>(r, itw2 + opaque_zero(), Ln.lane);
            lds_p2_to_p1<P>(r, buf, LT(opaque_lane()));
            const size_t rbase = ubase + (size_t)i * P::N;
            uint32_t ad[ADD ? 32 : 1];
            if constexpr (ADD) load32(ad, add + rbase + aoff, [](int j) { return LT::S * j; });
            uint32_t *po = out + rbase + ooff;
            // stores interleaved with the last stage; with an addend the last
            // stage leaves [0, 2q) and the sum (< 4q) is reduced here
            auto emit = [&](int j, uint32_t v) {
                if constexpr (ADD) v = canon4<P>(v + ad[j]);
                if (valid) st_out(po + LT::S * j, v);
            };
            inv_pass1_head<P>(r, Ln.h, tw_base<PS, true>(), itw2 + SWO + opaque_zero());
            constexpr uint32_t S0P = cshoup(P::NINV_R, P::Q);
            constexpr TwPair S1S = csigned_tw(P::C1_R, P::Q);
            inv_last_stage<P, !ADD>(r, P::NINV_R, S0P, S1S.x, S1S.y, emit);
        }
    }
}

// poly_scatter: one workgroup per polynomial builds it in LDS -- zero, scatter
// the h (position, value) pairs, store coalesced -- so every word of out is
// written exactly once (a zero fill and a scatter in global memory within one
// launch would race).  Values < 2q are reduced; positions >= n are ignored.
constexpr int SCATTER_WG = 256;
__global__ __launch_bounds__(SCATTER_WG) void k_poly_scatter(const uint32_t *__restrict__ pos,
                                                             const uint32_t *__restrict__ val, uint32_t *__restrict__ out,
                                                             uint32_t n, uint32_t q, uint32_t h)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t spoly[];
    const size_t b = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < n; i += SCATTER_WG) spoly[i] = 0;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < h; j += SCATTER_WG) {
        const uint32_t p = pos[b * h + j], v = val[b * h + j];
        if (p < n) spoly[p] = umin(v, v - q);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += SCATTER_WG) out[b * n + i] = spoly[i];
}

}  // namespace qntt
