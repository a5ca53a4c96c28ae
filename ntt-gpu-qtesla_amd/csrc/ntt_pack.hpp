// ntt_pack.hpp -- poly_pack / poly_unpack: qTESLA's wire formats (signature
// z, public key t) between bit-packed rows and [batch][k][n] coefficients.
// The definition is restated in full in include/qtesla_ntt.h;
// tests/pack_model.py is the same statement in numpy.
//
// Both kernels are memory-bound (4 B on the coefficient side, b / 8 on the
// byte side per coefficient) and have k_poly_round's shape (ntt_round.hpp): a
// wave owns 1024 consecutive coefficients, which are 128 b packed bytes (whole
// 128-byte lines for every b); a lane owns four groups of 4 coefficients, 64
// lanes apart, so every coefficient-side instruction of a wave is a 16-byte
// access covering 1 KiB contiguous; a polynomial is n / 1024 waves of one
// workgroup, the maxima go through lanes_max and the LDS combine, and a
// workgroup walks its dispatch-ordered chunk of tiles.  q, n's row geometry,
// b and the signedness are kernel arguments; only the waves per polynomial
// (the workgroup's size and the combine) are a template argument.
//
// Byte side of unpack.  Group g's four fields are bits [4 g b, 4 g b + 4 b) of
// the wave's span: they start at dword (g b) >> 3, bit ((g b) & 7) * 4, and
// span at most 5 dwords, which the lane loads straight from global memory (a
// wave instruction's addresses are monotone and dense over 32 b bytes, so
// every line comes from memory once and the cache serves the repeats).  A
// dword past the wave's span is never needed; its index is clamped to the
// span's last dword, so nothing outside [row, row + k n b / 8) is read.  The
// window is funnel-shifted down to the group's first bit and then by b per
// field (v_alignbit_b32), every register index a compile-time constant.
//
// Byte side of pack.  The wave's 1024 fields, masked to b bits, go to its own
// 4 KiB of LDS in coefficient order (one 16-byte write per group); lane l then
// assembles the whole output dwords l + 64 t.  Dword o holds bits
// [32 o, 32 o + 32): its first field is i0 = floor(32 o / b) (one multiply-high
// by a host-computed reciprocal, exact for every o < 32 b), shifted right by
// 32 o - i0 b; with b >= 8 at most four more fields follow, shifted left.  A
// wave's store instruction is 256 contiguous bytes, every output dword is
// written once by a plain vector store and the gap bytes of a row are not
// touched.
#pragma once
#include "ntt_device.hpp"
#include "ntt_round.hpp"

namespace qntt {

constexpr int PACK_WAVE_COEFFS = 1024;   // 64 lanes x 4 groups x 4 fields

template <int WPP> struct PackGeom {
    static constexpr int WAVES = WPP > 4 ? WPP : 4;   // waves per workgroup, a multiple of WPP
    static constexpr int WG = WAVES * 64;
    static_assert(WPP >= 1 && (WPP & (WPP - 1)) == 0 && WAVES % WPP == 0, "a polynomial's waves share a workgroup");
};

// the byte side and the field, as the kernels take them
struct PackRows {
    size_t stride;    // bytes from row to row
    uint32_t k;       // polynomials per row
    uint32_t b;       // bits per field, 8 .. 30
    uint32_t sbit;    // signed: 2^(b-1); unsigned: 0
    uint32_t q;
    uint32_t b_inv;   // floor(2^32 / b) + 1: floor(x / b) = mulhi(x, b_inv) for x < 2^32 / b
    // dword offset of wave gw's span (polynomial gw / WPP = row * k + ki)
    template <int WPP> __device__ __forceinline__ size_t span(size_t gw) const
    {
        const uint32_t p = (uint32_t)(gw / WPP), wq = (uint32_t)(gw % WPP), row = p / k, ki = p - row * k;
        return (size_t)row * (stride / 4) + ((size_t)ki * WPP + wq) * (32u * b);
    }
};

// in [batch rows of R.stride bytes], w [nwaves * 1024] canonical, mx (MAX): one word per nwaves / WPP polynomials
template <int WPP, bool MAX>
__global__ __launch_bounds__(PackGeom<WPP>::WG) void k_poly_unpack(uint32_t *__restrict__ w, uint32_t *__restrict__ mx,
                                                                   const uint32_t *__restrict__ in, PackRows R, size_t nwaves,
                                                                   uint32_t tiles)
{
    using G = PackGeom<WPP>;
    __shared__ uint32_t red[2][G::WAVES];
    const uint32_t lane = threadIdx.x & 63, wv = wave_id();
    const uint32_t b = R.b, mask = (1u << b) - 1u, last = 32u * b - 1u;
    size_t gw = (size_t)blockIdx.x * (G::WAVES * tiles) + wv;
#pragma unroll 1
    for (uint32_t it = 0; it < tiles; ++it, gw += G::WAVES) {
        if (gw - wv >= nwaves) break;     // the whole tile lies past the end (workgroup-uniform)
        const bool active = gw < nwaves;  // wave-uniform; a tile's tail waves only meet the barrier
        uint32_t m = 0;
        if (active) {
            const uint32_t *src = in + R.template span<WPP>(gw);
            round_u32x4 *dst = reinterpret_cast<round_u32x4 *>(w) + gw * (PACK_WAVE_COEFFS / 4) + lane;
            uint32_t d[4][5];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t first = ((lane + 64 * c) * b) >> 3;
#pragma unroll
                for (int j = 0; j < 5; ++j) d[c][j] = src[umin(first + j, last)];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t off = (((lane + 64 * c) * b) & 7u) * 4u;
                uint32_t r[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_alignbit(d[c][j + 1], d[c][j], off);
                round_u32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int32_t s = (int32_t)((r[0] & mask) ^ R.sbit) - (int32_t)R.sbit;   // sign-extended when signed
                    const uint32_t u = (uint32_t)s + (s < 0 ? R.q : 0u);
                    v[e] = umin(u, u - R.q);                                                 // unsigned fields in [q, 2q)
                    m = max(m, (uint32_t)(s < 0 ? -s : s));
#pragma unroll
                    for (int j = 0; j < 3; ++j) r[j] = __builtin_amdgcn_alignbit(r[j + 1], r[j], b);
                    r[3] >>= b;
                }
                __builtin_nontemporal_store(v, dst + 64 * c);
            }
        }
        if constexpr (MAX) {
            m = lanes_max<6>(m);
            if constexpr (WPP == 1) {
                if (active && lane == 0) mx[gw] = m;
            } else {
                if (lane == 0) red[it & 1][wv] = m;
                __syncthreads();
                if (active && wv % WPP == 0 && lane == 0) {
#pragma unroll
                    for (int o = 1; o < WPP; ++o) m = max(m, red[it & 1][wv + o]);
                    mx[gw / WPP] = m;
                }
            }
        }
    }
}

// w [nwaves * 1024] entries < 2q; out [batch rows of R.stride bytes]
template <int WPP>
__global__ __launch_bounds__(PackGeom<WPP>::WG) void k_poly_pack(uint32_t *__restrict__ out, const uint32_t *__restrict__ w,
                                                                 PackRows R, size_t nwaves, uint32_t tiles)
{
    using G = PackGeom<WPP>;
    __shared__ round_u32x4 fields[G::WAVES][PACK_WAVE_COEFFS / 4];
    const uint32_t lane = threadIdx.x & 63, wv = wave_id();
    const uint32_t b = R.b, mask = (1u << b) - 1u, ndw = 32u * b;
    const uint32_t centre = R.sbit ? (R.q - 1) / 2 : 0xFFFFFFFFu;   // x' above it packs as x' - q
    const uint32_t *f = reinterpret_cast<const uint32_t *>(fields[wv]);
    size_t gw = (size_t)blockIdx.x * (G::WAVES * tiles) + wv;
#pragma unroll 1
    for (uint32_t it = 0; it < tiles; ++it, gw += G::WAVES) {
        if (gw - wv >= nwaves) break;     // the whole tile lies past the end (workgroup-uniform)
        const bool active = gw < nwaves;  // wave-uniform; a tile's tail waves only meet the barrier
        if (active) {
            const round_u32x4 *src = reinterpret_cast<const round_u32x4 *>(w) + gw * (PACK_WAVE_COEFFS / 4) + lane;
            round_u32x4 v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = __builtin_nontemporal_load(src + 64 * c);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t x = umin(v[c][e], v[c][e] - R.q);   // [0, 2q) -> [0, q)
                    v[c][e] = (x > centre ? x - R.q : x) & mask;
                }
                fields[wv][lane + 64 * c] = v[c];
            }
        }
        __syncthreads();   // the wave's fields are in LDS
        if (active) {
            uint32_t *dst = out + R.template span<WPP>(gw);
#pragma unroll 1
            for (uint32_t o = lane; o < ndw; o += 64) {
                const uint32_t i0 = __umulhi(32u * o, R.b_inv);   // floor(32 o / b)
                const uint32_t down = 32u * o - i0 * b;             // < b: the first field's bits below the dword
                uint32_t word = f[i0] >> down;
#pragma unroll
                for (uint32_t j = 1; j < 5; ++j) {
                    const uint32_t up = j * b - down;               // > 0
                    const uint32_t x = f[umin(i0 + j, (uint32_t)PACK_WAVE_COEFFS - 1u)];
                    word |= up < 32u ? x << up : 0u;
                }
                __builtin_nontemporal_store(word, dst + o);
            }
        }
        // no second barrier: the fields are wave-private, and a wave's next writes follow its own reads in LDS order
    }
}

}  // namespace qntt
