// ntt_gen_a.hpp -- qTESLA's GenA over a batch (poly_gen_a): seed_a to the k
// public polynomials a_1 .. a_k, sampled directly in the NTT domain, so that a
// verifier holding only public-key bytes and a key-generation batch make their
// rows on the device.  The definition is restated in full in
// include/qtesla_ntt.h; tests/gen_a_model.py is the same statement in Python.
//
// Work split: one seed per lane, one wave per workgroup, keccak_f1600 and
// cshake_simple_prefix of ntt_xof.hpp with the state in registers, as
// k_sample_y.  A draw is one whole 32-bit word of the squeezed block (the
// accepted parameter sets have four-byte draws), word W picked by a
// compile-time index, so the draw index, the block count and the one tail
// predicate (an odd call leaves the last two words of its last block) are
// wave-uniform; only the output index i (draws minus this lane's rejections)
// is per lane.  A call is the prefix block, the seed, and its squeezed blocks:
// the first call (customisation 0, nblocks blocks) and every refill
// (customisation r, one block) run the same code, since at qTESLA's shapes
// half of a launch's permutations are refills.  The loop over calls runs while
// any lane has i < k n, at most refills_max times; a lane that is done stores
// nothing; lanes past the batch hash seed 0 and store nothing.
//
// Stores.  Every block rejects in some lane (a draw is accepted with
// probability 0.64 / 0.80), so the lanes' output indices drift apart at once
// and k_sample_y's flat tile does not apply: each accepted draw is one
// predicated dword store to the lane's own key.  (Staging a lane's accepted
// draws in a wave-private LDS column and writing them out in aligned groups
// of four as 16-byte stores was built as the A/B partner and measured:
// DESIGN.md section 5l.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "ntt_sample.hpp"

namespace qntt {

constexpr int GEN_A_WG = 64;      // one wave a workgroup, as k_sample_y
constexpr int GEN_A_WORDS = 42;   // 32-bit words of a 168-byte block

// what one lane carries through the kernel (everything but i and key is wave-uniform)
struct GenALane {
    uint32_t *key;    // polynomial 0 of this lane's key
    size_t gap;       // pstride - n: the words between two polynomials of a key
    uint32_t lg, kn, q, mask;
    uint32_t i;       // coefficients written so far; k n for a lane past the batch
    // coefficient j of the key, j = polynomial * n + index
    __device__ __forceinline__ uint32_t *at(uint32_t j) const { return key + ((size_t)j + (size_t)(j >> lg) * gap); }
};

// word W of the block: masked, stored when below q and the key is not yet full
template <int W> __device__ __forceinline__ void gen_a_draw(const uint64_t (&s)[25], GenALane &L)
{
    const uint32_t v = keccak_word<W>(s) & L.mask;
    const bool take = v < L.q && L.i < L.kn;
    if (take) *L.at(L.i) = v;
    L.i += take ? 1u : 0u;
}

// the block's 42 words, or its first 40 (`full` is wave-uniform)
template <int... W>
__device__ __forceinline__ void gen_a_block(const uint64_t (&s)[25], GenALane &L, bool full, std::integer_sequence<int, W...>)
{
    (((W < GEN_A_WORDS - 2 || full) ? gen_a_draw<W>(s, L) : (void)0), ...);
}

// a [batch][k] polynomials of n words, pstride words apart; seed [batch][sw] 8-byte words, 1 <= sw <= 20;
// n = 2^lg, mask = 2^qbits - 1 with four-byte draws
__global__ __launch_bounds__(GEN_A_WG) void k_gen_a(uint32_t *__restrict__ a, size_t pstride, const uint64_t *__restrict__ seed,
                                                    uint32_t sw, uint32_t batch, uint32_t k, uint32_t lg, uint32_t q,
                                                    uint32_t mask, uint32_t nblocks, uint32_t refills_max)
{
    constexpr int R = XOF_RATE128;
    const uint32_t b = blockIdx.x * GEN_A_WG + threadIdx.x;
    const bool live = b < batch;          // a tail lane stores nothing and reads nothing beyond the batch
    const uint32_t src = live ? b : 0;
    const uint64_t *sd = seed + (size_t)src * sw;
    const uint32_t kn = k << lg;
    GenALane L = {a + (size_t)src * k * pstride, pstride - ((size_t)1 << lg), lg, kn, q, mask, live ? 0u : kn};
#pragma unroll 1
    for (uint32_t r = 0; r <= refills_max; ++r) {   // r = 0: the first call, nblocks blocks; then one block per refill
        if (!__any(L.i < kn)) break;
        uint64_t s[25] = {};
        s[0] = cshake_simple_prefix<R>(r);          // r <= 65535
        keccak_f1600(s);
        const uint32_t swb = sw + (r >> 16);        // as in k_challenge: keeps the absorb predicates out of the loop's SGPRs
#pragma unroll
        for (int w = 0; w < R; ++w) {
            if ((uint32_t)w < swb) s[w] ^= sd[w];
            if ((uint32_t)w == swb) s[w] ^= 0x04;
        }
        s[R - 1] ^= XOF_PAD_LAST;
        keccak_f1600(s);
        uint32_t left = r == 0 ? nblocks : 1u;      // blocks of this call still to draw from
        const bool even = !(left & 1u);             // an odd call's last block gives 40 draws: draws come in fours
#pragma unroll 1
        for (;;) {
            gen_a_block(s, L, left > 1u || even, std::make_integer_sequence<int, GEN_A_WORDS>{});
            if (--left == 0 || !__any(L.i < kn)) break;
            keccak_f1600(s);
        }
    }
    for (; L.i < kn; ++L.i) *L.at(L.i) = 0;   // the refill bound was reached (not by hash outputs: qtesla_ntt.h)
}

}  // namespace qntt
