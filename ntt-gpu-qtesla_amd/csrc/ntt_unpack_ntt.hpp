// ntt_unpack_ntt.hpp -- poly_unpack_ntt: bit-packed rows (a public key's t, a
// signer's s and e_i) straight to NTT-domain polynomials, optionally negated
// and pstride words apart, so that slot 1 of the [k][2][n] verification rows,
// q - t-hat, is one launch from the key's bytes.  The definition is restated
// in full in include/qtesla_ntt.h; tests/unpack_ntt_model.py is the same
// statement in numpy.
//
// The kernel is k_ntt_fwd<PS, false> (ntt_device.hpp) with a load stage and a
// store stage of its own: the workgroup, the LDS budget, the wave-private
// transpose, the chunk walk and fwd_pass1 / lds_p1_to_p2 / fwd_pass2 are that
// kernel's.  A wave unit is one n = 2048 polynomial or two n = 1024 ones, one
// per half-wave; the two may lie in different rows of the byte side.
//
// Load.  In the pass-1 layout register j of a lane is coefficient
// i = brl + S j of its polynomial (S = 64 / 32).  Field i starts at bit i b of
// the polynomial's span (PackRows::span).  S j b is a whole number of dwords,
// (S / 32) b j, so the field's first dword is ((brl b) >> 5) + (S / 32) b j
// and its shift (brl b) & 31 is the same for all 32 registers of a lane.  With
// b <= 30 the field lies in that dword and the next: one v_alignbit_b32 and a
// mask.  The second index can pass the span's end only for j = 31 (the last
// field ends with the span); it is clamped to the span's last dword there, as
// k_poly_unpack clamps, so nothing outside [row, row + k n b / 8) is read.  A
// wave instruction covers 64 b contiguous bits (n = 2048) or two runs of 32 b
// (n = 1024), and the 32 instructions of a unit are dense over the span: every
// line comes from memory once and the cache serves the second dword.  (Bringing
// the span in coalesced through the wave's transpose buffer and extracting from
// LDS was built as the A/B partner and measured: DESIGN.md section 5o.)
//
// Value and maximum are k_poly_unpack's.  Signed fields are sign-extended and
// made canonical as there.  An unsigned field goes to the transform as it is:
// it is < 2^b <= 2q, the transform takes entries < 2q and gives the exact
// canonical result of their residues, so the result is bit-identical to
// poly_unpack's f - q followed by poly_ntt and two instructions a coefficient
// are saved.  The two forms are the two sides of a wave-uniform branch on the
// caller's sgn.  A polynomial belongs to one wave (or half-wave): its maximum
// is one lanes_max and a store by its first lane, no LDS combine and no barrier.
//
// Store.  canon4, then the negation (q - x, with q -> 0) on one side of a
// wave-uniform branch on the caller's neg, to out + poly pstride + brv5(j) S + lane: the
// lane-contiguous 128 / 256-byte runs of k_ntt_fwd.  The pstride - n words
// after a polynomial are not touched.
//
// Secret input (sgn = 1, a signer's key).  No branch, loop bound, global or LDS
// address depends on a field's value: the load addresses are functions of the
// lane, j, b and the unit; the sign extension, the + q and the maximum are
// selects; the two branches are on sgn and neg, which are the caller's; the
// transform and the transpose are data-independent.
#pragma once
#include "ntt_device.hpp"
#include "ntt_pack.hpp"

namespace qntt {

// in [batch rows of R.stride bytes]; out: polynomial p at p * pstride, n words, canonical; mx (MAX): one word per polynomial
template <int PS, bool MAX>
__global__ __launch_bounds__(NTT_WG, NTT_WAVES_PER_SIMD) void k_unpack_ntt(uint32_t *__restrict__ out, size_t pstride,
                                                                           uint32_t *__restrict__ mx,
                                                                           const uint32_t *__restrict__ in, PackRows R,
                                                                           uint32_t neg, uint32_t npoly, uint32_t ppw)
{
    using P = typename PSel<PS>::T;
    using LT = Lane<P>;
    constexpr int WPP = P::N / PACK_WAVE_COEFFS;   // PackRows::span counts in 1024-coefficient pieces
    __shared__ __attribute__((aligned(16))) uint32_t lds[NTT_LDS_WORDS];
    uint2 *tw2 = reinterpret_cast<uint2 *>(lds + NTT_WAVES * XPOSE_WORDS);
    auto prologue = [&]() {
        fill_tw2<PS, false, NTT_WG>(tw2);
        __syncthreads();
    };
    const LT L;
    uint32_t *buf = lds + (threadIdx.x >> 6) * XPOSE_WORDS;
    const uint32_t nunits = (npoly + LT::UPW - 1) / LT::UPW;
    const uint32_t b = R.b, mask = (1u << b) - 1u;
    const uint32_t last = (P::N / 32) * b - 1u;    // the span's last dword
    const uint32_t first = (L.brl * b) >> 5, sh = (L.brl * b) & 31u;

    // r[2 j], r[2 j + 1]: the two dwords of field brl + S j
    auto load = [&](uint32_t (&r)[64], uint32_t u) {
        // dwords between a lane's consecutive fields; opaque, so that its 32 multiples are made here, per unit, and
        // not kept in scalar registers across the whole walk
        const uint32_t step = (LT::S / 32) * (b + opaque_zero());
        const uint32_t p0 = u * LT::UPW;
        size_t off = R.template span<WPP>((size_t)p0 * WPP);
        if constexpr (!LT::BIG) {   // the second half-wave's polynomial, or the first again (Lane::load_poly)
            const size_t off1 = R.template span<WPP>((size_t)(p0 + 1 < npoly ? p0 + 1 : p0) * WPP);
            off = L.h ? off1 : off;
        }
        const uint32_t *src = in + off;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            r[2 * j] = ld_in(src + (first + step * j));
            r[2 * j + 1] = ld_in(src + (j < 31 ? first + step * j + 1 : umin(first + step * j + 1, last)));
        }
    };
    auto process = [&](uint32_t (&r)[64], uint32_t u) {
        uint32_t x[32], m = 0;
        if (R.sbit) {   // wave-uniform: the signedness is the caller's, not the data's
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const uint32_t f = __builtin_amdgcn_alignbit(r[2 * j + 1], r[2 * j], sh) & mask;
                const int32_t s = (int32_t)(f ^ R.sbit) - (int32_t)R.sbit;   // sign-extended
                x[j] = (uint32_t)s + (s < 0 ? P::Q : 0u);                    // canonical: 2^(b-1) <= (q-1)/2
                m = max(m, (uint32_t)(s < 0 ? -s : s));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                // the raw field, < 2^b <= 2q: the transform takes entries < 2q and gives the exact canonical result
                // of their residues, so poly_unpack's f - q is left to it
                x[j] = __builtin_amdgcn_alignbit(r[2 * j + 1], r[2 * j], sh) & mask;
                m = max(m, x[j]);
            }
        }
        const uint32_t poly = L.poly(u);
        const bool valid = LT::BIG || poly < npoly;
        if constexpr (MAX) {
            m = lanes_max<LT::BIG ? 6 : 5>(m);
            if (valid && L.brl == 0) mx[poly] = m;
        }
        fwd_pass1<PS, P>(x, L.h, tw2 + TW2_ENTRIES * 64 + opaque_zero());
        lds_p1_to_p2<P>(x, buf, L);
        fwd_pass2<P>(x, tw2 + opaque_zero(), L.lane);
        if (valid) {   // natural order from the bit-reversed pass-2 registers: brv5(j) * S + lane
            uint32_t *dst = out + (size_t)poly * pstride + L.brl;
            if (neg) {   // wave-uniform
#pragma unroll
                for (int j = 0; j < 32; ++j) st_out(dst + brv5(j) * LT::S, csub<P::Q>(P::Q - canon4<P>(x[j])));   // q - 0 -> 0
            } else {
#pragma unroll
                for (int j = 0; j < 32; ++j) st_out(dst + brv5(j) * LT::S, canon4<P>(x[j]));
            }
        }
    };
    chunk_loop<NTT_WAVES, 64>(nunits, ppw, prologue, load, process);
}

}  // namespace qntt
