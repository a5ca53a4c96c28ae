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
// k_poly_mul_kl_round is the same kernel with poly_round (ntt_round.hpp) as
// its store epilogue: both are ntt_mulkl_body.hpp, which says how.
//
// k_poly_mul_kl_keyed / k_poly_mul_kl_round_keyed are the same two kernels with
// one block of rows per key, ahat [nkeys][k][l][n], and an index per message
// (KeySel): the row base moves by key * (k l n) words and nothing else changes.
//
// Also here: k_poly_scatter, sparse (position, value) lists -> dense
// polynomials (qTESLA's challenge c).
#pragma once
#include "ntt_mulk.hpp"
#include "ntt_round.hpp"

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

// Outputs of the rounding epilogue (poly_mul_ntt_kl_round): hi NULL or
// [npoly][k][n] bytes, norms NULL or [npoly][k] pairs, d as in poly_round.
struct RoundOut {
    uint8_t *hi;
    uint2 *norms;
    uint32_t d;
};

// The keyed kernels' key of each message: message b takes the rows of key
// min(key ? key[b] : b, last), last = nkeys - 1.  The clamp is the definition
// (qtesla_ntt.h): whatever the index, the rows read lie inside ahat.
struct KeySel {
    const uint32_t *key;   // [npoly], or NULL
    uint32_t last;
};

template <int PS, int L, bool ADD>
__global__ __launch_bounds__(MULKL_WG, MULKL_WAVES_PER_SIMD) void k_poly_mul_kl(const MulKLIn<L> in,
                                                                                const uint32_t *__restrict__ ahat,
                                                                                const uint32_t *add, uint32_t *out,
                                                                                uint32_t npoly, uint32_t k, uint32_t ppw)
{
    constexpr bool RND = false;
    constexpr bool KEYED = false;
    const RoundOut ro = {};
    const KeySel ks = {};
#include "ntt_mulkl_body.hpp"
}

// poly_mul_ntt_kl_round: k_poly_mul_kl with poly_round as its store epilogue,
// at the same launch bounds and launch shape.  L = 1 (one y, the signer's
// w_i = v_i - e_i c with the addend v) is the same body.
template <int PS, int L, bool ADD>
__global__ __launch_bounds__(MULKL_WG, MULKL_WAVES_PER_SIMD) void k_poly_mul_kl_round(const MulKLIn<L> in,
                                                                                      const uint32_t *__restrict__ ahat,
                                                                                      const uint32_t *add, const RoundOut ro,
                                                                                      uint32_t npoly, uint32_t k,
                                                                                      uint32_t ppw)
{
    constexpr bool RND = true;
    constexpr bool KEYED = false;
    uint32_t *const out = nullptr;
    const KeySel ks = {};
#include "ntt_mulkl_body.hpp"
}

// poly_mul_ntt_kl_keyed / _kl_round_keyed: the two kernels above with ahat
// [nkeys][k][L][n] and the key of each message (ks), at the same launch bounds
// and launch shape.  L = 1 with ks.key NULL is a key-generation batch's
// t_b = a_b s_b + e_b.
template <int PS, int L, bool ADD>
__global__ __launch_bounds__(MULKL_WG, MULKL_WAVES_PER_SIMD) void k_poly_mul_kl_keyed(const MulKLIn<L> in,
                                                                                      const uint32_t *__restrict__ ahat,
                                                                                      const KeySel ks, const uint32_t *add,
                                                                                      uint32_t *out, uint32_t npoly, uint32_t k,
                                                                                      uint32_t ppw)
{
    constexpr bool RND = false;
    constexpr bool KEYED = true;
    const RoundOut ro = {};
#include "ntt_mulkl_body.hpp"
}

template <int PS, int L, bool ADD>
__global__ __launch_bounds__(MULKL_WG, MULKL_WAVES_PER_SIMD) void k_poly_mul_kl_round_keyed(
    const MulKLIn<L> in, const uint32_t *__restrict__ ahat, const KeySel ks, const uint32_t *add, const RoundOut ro,
    uint32_t npoly, uint32_t k, uint32_t ppw)
{
    constexpr bool RND = true;
    constexpr bool KEYED = true;
    uint32_t *const out = nullptr;
#include "ntt_mulkl_body.hpp"
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
