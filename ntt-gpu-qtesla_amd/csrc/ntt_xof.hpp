// ntt_xof.hpp -- SHAKE128 / SHAKE256 / cSHAKE-simple over a batch (ntt_xof)
// and qTESLA's challenge expansion Enc(c') (poly_challenge): the two hashes at
// the ends of a verification, on the device.
//
// keccak_f1600 is the one statement of the permutation; both kernels call it.
// The state is 25 lanes of uint64_t held in registers (50 VGPRs): every index
// into it is a compile-time constant -- theta, rho/pi and chi are expanded over
// integer sequences, absorb and squeeze are fully unrolled loops over the rate
// (a template argument: 21 lanes for SHAKE128, 17 for SHAKE256) whose
// run-time bounds are wave-uniform predicates, never subscripts -- so nothing
// of it lives in scratch.  The 24 rounds stay a rolled loop; the round
// constants are a constexpr table read through the scalar cache (they are
// wave-uniform).  A 64-bit rotate by a constant is two v_alignbit_b32.
//
// Work split: one message (one seed) per lane.  Absorbing is serial per
// message -- 76 permutations for p-III's H -- so the throughput comes from the
// batch; a small batch pays the whole serial chain on a handful of lanes
// (DESIGN.md section 5i).
//
// k_xof: message b is in0[b][0 .. 8 w0) || in1[b][0 .. 8 w1), two buffers used
// where they lie.  Message word t (8 bytes) is in0's for t < w0 and in1's
// otherwise; the boundary may fall anywhere in a rate block, so every word
// picks its segment by a wave-uniform compare.  Each lane reads its own
// stream with 8-byte loads (a row is only 8-byte aligned), a whole rate block
// in flight before its permutation; consecutive blocks of a lane share cache
// lines (staging each wave's 64 rate blocks through LDS with coalesced loads
// was built and measured 24 - 28 % slower at 2^20: DESIGN.md section 5i).
// Lengths are whole lanes, so the domain byte always lands on byte 0
// of lane `rem` and there is no byte-wise absorb.  Each lane writes its own
// out[b] with 8-byte vector stores, every word once.  Lanes past the batch
// return at once: there is no barrier in this kernel.
//
// k_challenge: one wave per workgroup, one seed per lane.  Per squeeze block:
// the cSHAKE prefix block (customisation = block counter), one permutation,
// the seed (at most 20 lanes, one absorb block), one permutation, then 56
// three-byte draws out of the 168 bytes, every byte picked by a constant
// index.  The set of taken positions is an n-bit map per lane in LDS, word w
// of lane l at [w * 64 + l]: the 32 lanes that an LDS access serves together
// always lie on 32 different banks whichever words they touch, and a lane only
// ever touches its own words (no barrier, no padding).  Positions and signs go
// out as they are accepted.  The block loop is bounded; whatever is left after
// the bound gets pos = 0xFFFFFFFF (ignored by poly_scatter), val = 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

namespace qntt {

constexpr int XOF_RATE128 = 21;   // SHAKE128: 168 bytes
constexpr int XOF_RATE256 = 17;   // SHAKE256: 136 bytes
constexpr int XOF_WG = 256;
constexpr int CHALLENGE_WG = 64;  // one wave: the bit map is wave-private
constexpr int CHALLENGE_DRAWS = 56;   // 168 / 3

// x rotated left by the constant N: ({a, b} >> s) twice
template <int N> __device__ __forceinline__ uint64_t rotl64(uint64_t x)
{
    static_assert(N >= 0 && N < 64, "rotation count");
    if constexpr (N == 0) return x;
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if constexpr (N == 32) return ((uint64_t)lo << 32) | hi;
    uint32_t nl, nh;
    if constexpr (N < 32) {
        nh = __builtin_amdgcn_alignbit(hi, lo, 32 - N);
        nl = __builtin_amdgcn_alignbit(lo, hi, 32 - N);
    } else {
        nh = __builtin_amdgcn_alignbit(lo, hi, 64 - N);
        nl = __builtin_amdgcn_alignbit(hi, lo, 64 - N);
    }
    return ((uint64_t)nh << 32) | nl;
}

// rho offsets of lane x + 5 y
struct KeccakRho {
    static constexpr int R[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                  25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
};

using KeccakLanes = std::make_integer_sequence<int, 25>;
using KeccakCols = std::make_integer_sequence<int, 5>;

template <int... X> __device__ __forceinline__ void keccak_theta(uint64_t (&a)[25], std::integer_sequence<int, X...>)
{
    const uint64_t c[5] = {(a[X] ^ a[X + 5] ^ a[X + 10] ^ a[X + 15] ^ a[X + 20])...};
    const uint64_t d[5] = {(c[(X + 4) % 5] ^ rotl64<1>(c[(X + 1) % 5]))...};
    ((a[X] ^= d[X], a[X + 5] ^= d[X], a[X + 10] ^= d[X], a[X + 15] ^= d[X], a[X + 20] ^= d[X]), ...);
}
// b[y + 5 ((2x + 3y) mod 5)] = rotl(a[x + 5y], rho[x + 5y])
template <int... I>
__device__ __forceinline__ void keccak_rho_pi(const uint64_t (&a)[25], uint64_t (&b)[25], std::integer_sequence<int, I...>)
{
    ((b[I / 5 + 5 * ((2 * (I % 5) + 3 * (I / 5)) % 5)] = rotl64<KeccakRho::R[I]>(a[I])), ...);
}
template <int... I>
__device__ __forceinline__ void keccak_chi(uint64_t (&a)[25], const uint64_t (&b)[25], std::integer_sequence<int, I...>)
{
    ((a[I] = b[I] ^ (~b[(I % 5 + 1) % 5 + 5 * (I / 5)] & b[(I % 5 + 2) % 5 + 5 * (I / 5)])), ...);
}

__device__ __forceinline__ void keccak_f1600(uint64_t (&a)[25])
{
    static constexpr uint64_t RC[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
        0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
        0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
        0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
        0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        uint64_t b[25];
        keccak_theta(a, KeccakCols{});
        keccak_rho_pi(a, b, KeccakLanes{});
        keccak_chi(a, b, KeccakLanes{});
        a[0] ^= RC[r];
    }
}

// The first lane of cSHAKE's prefix block for an empty function name and the
// two-byte customisation string `cstm` (little-endian), bytepad'ed to the rate:
// 01 <rate> 01 00 01 10 lo hi, every other byte of the block zero.
template <int R> __device__ __forceinline__ uint64_t cshake_simple_prefix(uint32_t cstm)
{
    return 0x0000100100010001ull | ((uint64_t)(R * 8) << 8) | ((uint64_t)(cstm & 0xFFFFu) << 48);
}

constexpr uint64_t XOF_PAD_LAST = 0x8000000000000000ull;   // 0x80 in the rate's last byte

// out [batch][ow], in0 [batch][w0], in1 [batch][w1], all in 8-byte words;
// cstm < 0: SHAKE (domain byte 0x1F), else cSHAKE-simple (prefix block, 0x04)
template <int R>
__global__ __launch_bounds__(XOF_WG) void k_xof(uint64_t *__restrict__ out, uint32_t ow, const uint64_t *__restrict__ in0,
                                                uint32_t w0, const uint64_t *__restrict__ in1, uint32_t w1, uint32_t batch,
                                                int cstm)
{
    const uint32_t b = blockIdx.x * XOF_WG + threadIdx.x;
    if (b >= batch) return;
    const uint64_t *p0 = in0 + (size_t)b * w0;
    const uint64_t *p1 = in1 + (size_t)b * w1;
    auto word = [&](uint32_t t) { return t < w0 ? p0[t] : p1[t - w0]; };   // t < w0 is wave-uniform
    uint64_t s[25] = {};
    uint64_t dom = 0x1F;
    if (cstm >= 0) {
        s[0] = cshake_simple_prefix<R>((uint32_t)cstm);
        keccak_f1600(s);
        dom = 0x04;
    }
    const uint32_t words = w0 + w1;
    uint32_t t = 0;
#pragma unroll 1
    for (; words - t >= (uint32_t)R; t += R) {
#pragma unroll
        for (int i = 0; i < R; ++i) s[i] ^= word(t + i);
        keccak_f1600(s);
    }
    const uint32_t rem = words - t;   // < R: the last block holds rem words, then the padding
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if ((uint32_t)i < rem) s[i] ^= word(t + i);
        if ((uint32_t)i == rem) s[i] ^= dom;
    }
    s[R - 1] ^= XOF_PAD_LAST;
    keccak_f1600(s);
    uint64_t *o = out + (size_t)b * ow;
    uint32_t left = ow;
#pragma unroll 1
    for (;;) {
#pragma unroll
        for (int i = 0; i < R; ++i)
            if ((uint32_t)i < left) o[i] = s[i];
        if (left <= (uint32_t)R) break;
        left -= R;
        o += R;
        keccak_f1600(s);
    }
}

// byte K of a squeezed block
template <int K> __device__ __forceinline__ uint32_t keccak_byte(const uint64_t (&s)[25])
{
    return (uint32_t)(s[K / 8] >> (8 * (K % 8))) & 0xFFu;
}

// draw J of a block: its three bytes against this lane's map; accepted draws go out at once
template <int J>
__device__ __forceinline__ void challenge_draw(const uint64_t (&s)[25], uint32_t *taken, uint32_t lane, uint32_t nmask,
                                               uint32_t q, uint32_t h, uint32_t &i, uint32_t *op, uint32_t *ov)
{
    // one flat predicate per draw (a finished lane still reads its map: the slot is always its own)
    const uint32_t p = ((keccak_byte<3 * J>(s) << 8) | keccak_byte<3 * J + 1>(s)) & nmask;
    const uint32_t slot = (p >> 5) * CHALLENGE_WG + lane, bit = 1u << (p & 31);
    const uint32_t w = taken[slot];
    const bool take = i < h && !(w & bit);
    if (take) {
        taken[slot] = w | bit;
        op[i] = p;
        ov[i] = (keccak_byte<3 * J + 2>(s) & 1u) ? q - 1 : 1u;
    }
    i += take ? 1u : 0u;
}
template <int... J>
__device__ __forceinline__ void challenge_draws(const uint64_t (&s)[25], uint32_t *taken, uint32_t lane, uint32_t nmask,
                                                uint32_t q, uint32_t h, uint32_t &i, uint32_t *op, uint32_t *ov,
                                                std::integer_sequence<int, J...>)
{
    (challenge_draw<J>(s, taken, lane, nmask, q, h, i, op, ov), ...);
}

// pos, val [batch][h]; seed [batch][sw] 8-byte words, 1 <= sw <= 20; n a power
// of two, n / 32 * 64 words of dynamic LDS
__global__ __launch_bounds__(CHALLENGE_WG) void k_challenge(uint32_t *__restrict__ pos, uint32_t *__restrict__ val,
                                                            const uint64_t *__restrict__ seed, uint32_t sw, uint32_t batch,
                                                            uint32_t h, uint32_t n, uint32_t q, uint32_t blocks_max)
{
    constexpr int R = XOF_RATE128;
    extern __shared__ uint32_t taken[];   // word w of lane l at [w * 64 + l]
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x * CHALLENGE_WG + lane;
    const bool live = b < batch;          // a tail lane draws nothing and stores nothing
    for (uint32_t w = 0; w < n / 32; ++w) taken[w * CHALLENGE_WG + lane] = 0;
    const uint64_t *sd = seed + (size_t)(live ? b : 0) * sw;
    uint32_t *op = pos + (size_t)(live ? b : 0) * h, *ov = val + (size_t)(live ? b : 0) * h;
    uint32_t i = live ? 0 : h;
#pragma unroll 1
    for (uint32_t dmsp = 0; dmsp < blocks_max; ++dmsp) {
        if (!__any(i < h)) break;
        uint64_t s[25] = {};
        s[0] = cshake_simple_prefix<R>(dmsp);
        keccak_f1600(s);
        // sw again per block (dmsp < 2^16, the term is 0): computed once before the loop, the
        // 41 wave-uniform predicates below would stay in SGPRs across both permutations and spill
        const uint32_t swb = sw + (dmsp >> 16);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if ((uint32_t)k < swb) s[k] ^= sd[k];
            if ((uint32_t)k == swb) s[k] ^= 0x04;
        }
        s[R - 1] ^= XOF_PAD_LAST;
        keccak_f1600(s);
        challenge_draws(s, taken, lane, n - 1, q, h, i, op, ov, std::make_integer_sequence<int, CHALLENGE_DRAWS>{});
    }
    for (; i < h; ++i) {   // the block bound was reached (not by hash outputs: qtesla_ntt.h)
        op[i] = 0xFFFFFFFFu;
        ov[i] = 0;
    }
}

}  // namespace qntt
