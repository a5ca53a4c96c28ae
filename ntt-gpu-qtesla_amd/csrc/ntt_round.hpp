// ntt_round.hpp -- poly_round: qTESLA's rounding [.]_M and the two norm
// maxima its signer tests, per polynomial.  For a coefficient x < 2q and a
// bit count d (an argument: the library keeps no scheme constants),
//   x' = x mod q
//   c  = x' > (q-1)/2 ? x' - q : x'                centred
//   lo = c mod+- 2^d  in (-2^(d-1), 2^(d-1)]
//   hi = (c - lo) >> d = (c + 2^(d-1) - 1) >> d    (arithmetic shift)
// and a polynomial's outputs are hi as n two's-complement bytes and the pair
// { max |c|, max |lo| }.  round_coeff is the one statement of it on the
// device: k_poly_round below and the rounding epilogue of k_poly_mul_kl_round
// (ntt_mulkl.hpp) both call it.
//
// k_poly_round is memory-bound (4 B read, 1 B written per coefficient).  Work
// split: a thread takes 16 coefficients as four 16-byte loads, 64 lanes
// apart, so every load instruction of a wave covers 1 KiB contiguous and the
// four are in flight together; its 4 bytes per load go out as one dword, a
// wave's store 256 B contiguous.  A wave therefore rounds 1024 consecutive
// coefficients whatever n is, and a polynomial is n / 1024 waves that always
// lie in one workgroup:
//   n = 1024   one wave per polynomial, 4 polynomials per 256-thread workgroup;
//              the maxima are reduced across lanes, lane 0 stores the pair
//   n = 2048   two waves,  2 polynomials per workgroup
//   n = 4096   four waves, the whole 256-thread workgroup
//   n = 8192   eight waves, a 512-thread workgroup
// With more than one wave per polynomial each wave's pair goes through LDS and
// the polynomial's first wave combines them after one barrier.  So batch 1 at
// n = 8192 is 512 threads with four loads each, not one wave walking 8192
// coefficients, and the large-batch shape is the same code: no second kernel
// and no threshold.  A workgroup walks up to ROUND_TILES_MAX consecutive
// tiles (the batch kernels' dispatch-ordered chunk, see chunk_loop); the LDS
// slots alternate between iterations, one barrier each.  Every output word is
// written once by a plain vector store: no atomics, no accumulators in memory.
#pragma once
#include "ntt_device.hpp"

namespace qntt {

// x canonical in [0, q): hi, |c| and |lo| of the definition above; 1 <= d <= 30
template <class P>
__device__ __forceinline__ void round_coeff(uint32_t x, uint32_t d, int32_t &hi, uint32_t &abs_c, uint32_t &abs_lo)
{
    static_assert(P::Q < (1u << 30), "c + 2^(d-1) - 1 fits int32 for d <= 30");
    constexpr uint32_t H = (P::Q - 1) / 2;
    const int32_t c = (int32_t)(x > H ? x - P::Q : x);
    const uint32_t two_d = 1u << d;
    const uint32_t t = (uint32_t)c & (two_d - 1);   // lo = t <= 2^(d-1) ? t : t - 2^d
    hi = (c + (int32_t)(two_d / 2 - 1)) >> d;
    abs_c = umin(x, P::Q - x);
    abs_lo = umin(t, two_d - t);
}

// max over the lanes that differ from this one in the bits below 2^LOGW
template <int LOGW>
__device__ __forceinline__ uint32_t lanes_max(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < (1 << LOGW); m <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}

typedef uint32_t round_u32x4 __attribute__((ext_vector_type(4)));

#ifndef ROUND_TILES_MAX
#define ROUND_TILES_MAX 4
#endif

template <int PS> struct RoundGeom {
    using P = typename PSel<PS>::T;
    static constexpr int WAVE_COEFFS = 1024;                  // 64 lanes x 4 loads x 4 words
    static constexpr int WPP = P::N / WAVE_COEFFS;            // waves per polynomial
    static constexpr int WAVES = WPP > 4 ? WPP : 4;           // waves per workgroup, a multiple of WPP
    static constexpr int WG = WAVES * 64;
    static_assert(P::N % WAVE_COEFFS == 0 && WAVES % WPP == 0, "a polynomial's waves share a workgroup");
};

// w: nwaves * 1024 words, entries < 2q; hi (HI): one byte per word; norms
// (NORMS): one pair per nwaves / WPP polynomials.  Workgroup b owns tiles
// [b * tiles, (b + 1) * tiles), a tile being WAVES consecutive waves' worth.
template <int PS, bool HI, bool NORMS>
__global__ __launch_bounds__(RoundGeom<PS>::WG) void k_poly_round(const uint32_t *__restrict__ w, uint32_t *__restrict__ hi,
                                                                  uint2 *__restrict__ norms, size_t nwaves, uint32_t d,
                                                                  uint32_t tiles)
{
    using G = RoundGeom<PS>;
    using P = typename G::P;
    __shared__ uint2 red[2][G::WAVES];
    const uint32_t lane = threadIdx.x & 63, wv = wave_id();
    size_t gw = (size_t)blockIdx.x * (G::WAVES * tiles) + wv;
#pragma unroll 1
    for (uint32_t it = 0; it < tiles; ++it, gw += G::WAVES) {
        if (gw - wv >= nwaves) break;     // the whole tile lies past the end (workgroup-uniform)
        const bool active = gw < nwaves;  // wave-uniform; a tile's tail waves only meet the barrier
        uint32_t mc = 0, ml = 0;
        if (active) {
            const size_t base = gw * (G::WAVE_COEFFS / 4) + lane;   // in 16-byte units of w, dwords of hi
            const round_u32x4 *src = reinterpret_cast<const round_u32x4 *>(w) + base;
            round_u32x4 v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = __builtin_nontemporal_load(src + 64 * c);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint32_t word = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int32_t h;
                    uint32_t ac, al;
                    round_coeff<P>(csub<P::Q>(v[c][e]), d, h, ac, al);
                    word |= ((uint32_t)h & 0xFFu) << (8 * e);
                    mc = max(mc, ac);
                    ml = max(ml, al);
                }
                if constexpr (HI) __builtin_nontemporal_store(word, hi + base + 64 * c);
            }
        }
        if constexpr (NORMS) {
            mc = lanes_max<6>(mc);
            ml = lanes_max<6>(ml);
            if constexpr (G::WPP == 1) {
                if (active && lane == 0) norms[gw] = make_uint2(mc, ml);
            } else {
                if (lane == 0) red[it & 1][wv] = make_uint2(mc, ml);
                __syncthreads();
                if (active && wv % G::WPP == 0 && lane == 0) {
#pragma unroll
                    for (int o = 1; o < G::WPP; ++o) {
                        const uint2 r = red[it & 1][wv + o];
                        mc = max(mc, r.x);
                        ml = max(ml, r.y);
                    }
                    norms[gw / G::WPP] = make_uint2(mc, ml);
                }
            }
        }
    }
}

}  // namespace qntt
