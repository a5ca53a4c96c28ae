// ntt_gauss.hpp -- qTESLA's key generation on the device: the CDT Gaussian
// sampler over a batch (poly_sample_gauss) and check_ES's sum of the h largest
// |coefficients| (poly_hsum).  Both definitions are restated in full in
// include/qtesla_ntt.h; tests/gauss_model.py is the same statement in Python.
//
// k_sample_gauss.  Work split: one 512-sample chunk per lane -- the chunks of a
// polynomial are independent cSHAKE calls -- one wave per workgroup,
// keccak_f1600 and cshake_simple_prefix of ntt_xof.hpp with the state in
// registers, as k_sample_y.  Lane g is chunk g % (n / 512) of polynomial
// g / (n / 512), so a wave's 64 chunks are 64 * 512 consecutive words of the
// output.  There is no rejection: every lane makes the same draws from the
// same stream positions, so the sample index, the block count and the one tail
// predicate are wave-uniform.  A sample is `cols` whole 32-bit words of the
// squeezed stream; a block is 42 (rate 168) or 34 (rate 136) words, so samples
// straddle blocks with a period of lcm(words, cols) / words blocks:
//   rate 168   cols 1: 42 a block   2: 21   3: 14   4: 10 + 11 over two blocks
//   rate 136   cols 1: 34 a block   2: 17   3: 11 + 11 + 12 over three   4: 8 + 9 over two
// The chunk loop is unrolled over the period: every word is picked by a
// compile-time index and the one to three words of a straddling sample are
// carried in registers.  Neither the state nor the words go to scratch.
//
// The count.  A block's samples are packed once into the integer R of the
// definition (31-bit limbs, most significant first: 32, 64 or 128 bits), in
// groups of at most 21 samples; then one loop runs over all `rows` table rows:
// row j is read through the scalar cache (j is wave-uniform, the table at most
// 2 KiB), packed the same way on the scalar unit, and compared with every
// sample of the group -- one compare, or for three and four limbs the borrow
// of R - T_j through a carry chain -- each adding 0 or 1 to that sample's
// counter.
//
// Constant time.  The samples, their source words and the counters are
// secret.  No branch, loop bound, memory address or LDS address depends on R,
// m or the sign: the row loop always runs `rows` times, a compare is a flag
// and an add, the sign is applied by a select, and every address below is a
// function of the lane, the block and the sample index alone.  This is
// verified by reading (the kernel's only branches are on wave-uniform public
// values: rows, the samples left, lanes past the batch).
//
// Stores.  out[i] per lane would hit 64 rows per instruction.  A block's D
// samples go to a wave-private LDS tile, lane l's sample J at tile[l * S + J]
// (S odd: conflict-free), and the tile is read back flat, element 64 t + lane
// of instruction t (conflict-free), which is sample e % S of row e / S; a
// store instruction then covers 64 consecutive elements of the tile, at most
// three rows' runs.  Every row's run starts at the same offset (the samples
// done so far), so unlike sample_flush there is no per-row index to fetch.
// Lanes past the last chunk hash message 0's seed and store nothing.
//
// k_hsum.  One wave per polynomial, the n / 64 centred magnitudes of a lane in
// registers (16-byte loads, 64 lanes apart).  The h-th largest magnitude t* is
// found by a fixed bisection over the 30 value bits: each round counts
// |c| >= t with one compare and one add per register and sums the lanes'
// counts with six shuffles.  The sum is then sum_{|c| > t*} |c| + (h - #{|c| > t*}) t*,
// which counts ties as often as they occur.  The 30 rounds, every compare and
// every address are independent of the data (s and e are secret).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "ntt_round.hpp"
#include "ntt_sample.hpp"
#include "ntt_xof.hpp"

namespace qntt {

constexpr int GAUSS_WG = 64;       // one wave: the tile is wave-private
constexpr int GAUSS_CHUNK = 512;   // NTT_GAUSS_CHUNK: samples per cSHAKE call
constexpr uint32_t GAUSS_LIMB = 0x7FFFFFFFu;

// Block P of a period of a chunk's stream at rate R lanes and C words a sample: CW words of its first
// sample came with the block before, D samples complete in it, LEFT words stay over for the next block.
template <int R, int C, int P> struct GaussPhase {
    static constexpr int WORDS = 2 * R;
    static constexpr int CW = (P * WORDS) % C;
    static constexpr int D = (WORDS + CW) / C;
    static constexpr int LEFT = (WORDS + CW) % C;
};
template <int R, int C> struct GaussRate {
    static constexpr int PERIOD = (2 * R) % C == 0 ? 1 : (4 * R) % C == 0 ? 2 : 3;
    static constexpr int STRIDE = ((2 * R + C - 1) / C) | 1;   // tile row, in words: odd, >= every D
    static_assert((PERIOD * 2 * R) % C == 0, "the period ends on a sample");
};

// a sample or a table row as an integer: 31-bit limbs, most significant first (at most 124 bits)
template <int C> struct GaussInt { using T = unsigned __int128; };
template <> struct GaussInt<1> { using T = uint32_t; };
template <> struct GaussInt<2> { using T = uint64_t; };
template <int C> __device__ __forceinline__ typename GaussInt<C>::T gauss_pack(const uint32_t (&w)[C])
{
    typename GaussInt<C>::T v = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) v = (v << 31) | (w[k] & GAUSS_LIMB);
    return v;
}
// r >= t as 0 or 1: one compare, or the borrow of r - t over the words of the integer; a flag and no branch
template <class T> __device__ __forceinline__ uint32_t gauss_ge(T r, T t)
{
    if constexpr (sizeof(T) <= 8) return (uint32_t)(r >= t);
    else {
        T d;
        return (uint32_t)!__builtin_sub_overflow(r, t, &d);
    }
}

// word K of sample J of block P; `carry` holds the CW words that came with the block before
template <int R, int C, int P, int J, int K>
__device__ __forceinline__ uint32_t gauss_word(const uint64_t (&s)[25], const uint32_t (&carry)[3])
{
    constexpr int O = J * C + K - GaussPhase<R, C, P>::CW;
    static_assert(O >= 0 || J == 0, "only the first sample straddles");
    if constexpr (O < 0) return carry[J * C + K];
    else return keccak_word<O>(s);
}
template <int R, int C, int P, int J, int... K>
__device__ __forceinline__ typename GaussInt<C>::T gauss_sample(const uint64_t (&s)[25], const uint32_t (&carry)[3],
                                                                std::integer_sequence<int, K...>)
{
    const uint32_t w[C] = {gauss_word<R, C, P, J, K>(s, carry)...};
    return gauss_pack<C>(w);
}

// what one lane carries through k_sample_gauss (everything but the state is wave-uniform)
struct GaussLane {
    const uint32_t *cdt;   // [rows][C]
    uint32_t rows, q;
    uint32_t *out;         // chunk 0 of the wave
    uint32_t nrows;        // chunks of this wave inside the batch
    uint32_t lane;
    uint32_t done;         // samples of the chunk stored so far
};

// the tile as 64 consecutive elements per store instruction; `width` samples per row are valid
template <int S> __device__ __forceinline__ void gauss_flush(const uint32_t *tile, GaussLane &L, uint32_t width)
{
    __syncthreads();   // one wave: orders the lanes' tile writes before the flat reads
#pragma unroll 1
    for (uint32_t t = 0; t < (uint32_t)S; ++t) {
        const uint32_t e = t * GAUSS_WG + L.lane, r = e / (uint32_t)S, c = e - r * (uint32_t)S;
        const uint32_t v = tile[e];
        if (c < width && r < L.nrows) L.out[(size_t)r * GAUSS_CHUNK + L.done + c] = v;
    }
    // the next block's tile writes follow these reads in program order (same wave, LDS is in order)
    L.done += width;
}

// Samples J0 + J... of block P to the tile: packed once, then counted over all rows.  A block goes in groups of
// at most GAUSS_GROUP samples, which bounds the registers of the row loop whatever the samples per block.
constexpr int GAUSS_GROUP = 21;
template <int R, int C, int P, int J0, int... J>
__device__ __forceinline__ void gauss_group(const uint64_t (&s)[25], const uint32_t (&carry)[3], const GaussLane &L, uint32_t *tile,
                                            std::integer_sequence<int, J...>)
{
    using T = typename GaussInt<C>::T;
    using Limbs = std::make_integer_sequence<int, C>;
    const T v[sizeof...(J)] = {gauss_sample<R, C, P, J0 + J>(s, carry, Limbs{})...};
    uint32_t m[sizeof...(J)] = {};
#pragma unroll 1
    for (uint32_t j = 0; j < L.rows; ++j) {   // all rows, always
        uint32_t tw[C];
#pragma unroll
        for (int k = 0; k < C; ++k) tw[k] = L.cdt[j * C + k];   // wave-uniform: scalar loads
        const T t = gauss_pack<C>(tw);
        ((m[J] += gauss_ge<T>(v[J], t)), ...);
    }
    // (sign && m) ? q - m : m, by a select
    ((tile[L.lane * GaussRate<R, C>::STRIDE + J0 + J] =
          ((gauss_word<R, C, P, J0 + J, 0>(s, carry) >> 31) & (uint32_t)(m[J] != 0)) ? L.q - m[J] : m[J]),
     ...);
}

// Block P of the chunk with `left` samples still to make (wave-uniform; in the last block the samples past
// them are computed from stream words that exist and are not stored); true when it was the last one.
template <int R, int C, int P>
__device__ __forceinline__ bool gauss_phase(uint64_t (&s)[25], uint32_t (&carry)[3], uint32_t &left, GaussLane &L, uint32_t *tile)
{
    using Ph = GaussPhase<R, C, P>;
    constexpr int G0 = Ph::D < GAUSS_GROUP ? Ph::D : GAUSS_GROUP;
    static_assert(Ph::D <= 2 * GAUSS_GROUP, "two groups cover a block");
    gauss_group<R, C, P, 0>(s, carry, L, tile, std::make_integer_sequence<int, G0>{});
    if constexpr (Ph::D > G0) gauss_group<R, C, P, G0>(s, carry, L, tile, std::make_integer_sequence<int, Ph::D - G0>{});
    gauss_flush<GaussRate<R, C>::STRIDE>(tile, L, left < (uint32_t)Ph::D ? left : (uint32_t)Ph::D);
    if (left <= (uint32_t)Ph::D) return true;
    left -= Ph::D;
    if constexpr (Ph::LEFT > 0) carry[0] = keccak_word<Ph::WORDS - Ph::LEFT>(s);
    if constexpr (Ph::LEFT > 1) carry[1] = keccak_word<Ph::WORDS - Ph::LEFT + 1>(s);
    if constexpr (Ph::LEFT > 2) carry[2] = keccak_word<Ph::WORDS - Ph::LEFT + 2>(s);
    keccak_f1600(s);
    return false;
}

// out [batch][n]; seed [batch][sw] 8-byte words, 1 <= sw <= R - 1; nonces NULL or [batch]; cdt [rows][C];
// a polynomial is 2^lcpp chunks of 512 samples
template <int R, int C>
__global__ __launch_bounds__(GAUSS_WG) void k_sample_gauss(uint32_t *__restrict__ out, const uint64_t *__restrict__ seed,
                                                           uint32_t sw, const uint32_t *__restrict__ nonces, uint32_t nonce,
                                                           const uint32_t *__restrict__ cdt, uint32_t rows, uint32_t batch,
                                                           uint32_t lcpp, uint32_t q)
{
    __shared__ uint32_t tile[GAUSS_WG * GaussRate<R, C>::STRIDE];
    const uint32_t lane = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * GAUSS_WG, g = g0 + lane, total = (uint64_t)batch << lcpp;
    const bool live = g < total;          // a tail lane stores nothing and reads nothing beyond the batch
    const uint32_t src = live ? (uint32_t)(g >> lcpp) : 0u, ch = (uint32_t)g & ((1u << lcpp) - 1u);
    const uint64_t *sd = seed + (size_t)src * sw;
    const uint32_t cstm = (((((nonces ? nonces[src] : 0u) + nonce) & 0xFFu) << 8) + ch) & 0xFFFFu;
    GaussLane L = {cdt, rows, q, out + (size_t)g0 * GAUSS_CHUNK,
                   total - g0 < (uint64_t)GAUSS_WG ? (uint32_t)(total - g0) : (uint32_t)GAUSS_WG, lane, 0u};
    uint64_t s[25] = {};
    s[0] = cshake_simple_prefix<R>(cstm);
    keccak_f1600(s);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if ((uint32_t)k < sw) s[k] ^= sd[k];
        if ((uint32_t)k == sw) s[k] ^= 0x04;
    }
    s[R - 1] ^= XOF_PAD_LAST;
    keccak_f1600(s);
    uint32_t left = GAUSS_CHUNK, carry[3] = {0, 0, 0};
#pragma unroll 1
    for (;;) {
        if (gauss_phase<R, C, 0>(s, carry, left, L, tile)) break;
        if constexpr (GaussRate<R, C>::PERIOD >= 2) {
            if (gauss_phase<R, C, 1>(s, carry, left, L, tile)) break;
        }
        if constexpr (GaussRate<R, C>::PERIOD == 3) {
            if (gauss_phase<R, C, 2>(s, carry, left, L, tile)) break;
        }
    }
}

// the sum over the wave's 64 lanes, in every lane
__device__ __forceinline__ uint32_t lanes_sum(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

constexpr int HSUM_WAVES = 4;   // polynomials per workgroup, one wave each (no barrier)

// w [batch][N] with entries < 2q; sum [batch]; 1 <= h <= N
template <int PS>
__global__ __launch_bounds__(HSUM_WAVES * 64) void k_hsum(uint64_t *__restrict__ sum, const uint32_t *__restrict__ w, uint32_t batch,
                                                          uint32_t h)
{
    using P = typename PSel<PS>::T;
    constexpr int VECS = P::N / 256;   // 16-byte loads per lane
    static_assert(P::Q < (1u << 30), "|c| <= (q - 1) / 2 has 29 bits: the bisection's 30 cover it");
    const uint32_t lane = threadIdx.x & 63, b = blockIdx.x * HSUM_WAVES + wave_id();
    if (b >= batch) return;   // wave-uniform
    const round_u32x4 *src = reinterpret_cast<const round_u32x4 *>(w + (size_t)b * P::N) + lane;
    round_u32x4 a[VECS];
#pragma unroll
    for (int c = 0; c < VECS; ++c) a[c] = __builtin_nontemporal_load(src + 64 * c);
#pragma unroll
    for (int c = 0; c < VECS; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t x = csub<P::Q>(a[c][e]);
            a[c][e] = umin(x, P::Q - x);   // |c| of poly_round's centred value
        }
    }
    uint32_t t = 0;   // the largest t with #{|c| >= t} >= h, built from the top bit down
#pragma unroll 1
    for (int bit = 29; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        uint32_t cnt = 0;
#pragma unroll
        for (int c = 0; c < VECS; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) cnt += (uint32_t)(a[c][e] >= cand);
        }
        cnt = lanes_sum(cnt);
        t = cnt >= h ? cand : t;
    }
    uint64_t above = 0;
    uint32_t nabove = 0;
#pragma unroll
    for (int c = 0; c < VECS; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool gt = a[c][e] > t;
            above += gt ? a[c][e] : 0u;
            nabove += (uint32_t)gt;
        }
    }
    nabove = lanes_sum(nabove);
    above = ((uint64_t)lanes_sum((uint32_t)(above >> 32)) << 32) + (uint64_t)lanes_sum((uint32_t)above & 0xFFFFu) +
            ((uint64_t)lanes_sum((uint32_t)above >> 16) << 16);   // 16-bit pieces: 64 of them sum within 32 bits
    if (lane == 0) sum[b] = above + (uint64_t)(h - nabove) * t;
}

}  // namespace qntt
