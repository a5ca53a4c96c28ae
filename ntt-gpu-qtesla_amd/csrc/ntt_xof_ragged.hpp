// ntt_xof_ragged.hpp -- SHAKE128 / SHAKE256 / cSHAKE-simple over messages of
// any byte length, back to back in one buffer behind CSR-style offsets
// (ntt_xof_ragged): qTESLA's G(m) on the device.
//
// k_xof_ragged is k_xof (ntt_xof.hpp) with three things per lane instead of
// per launch: the length, the byte the padding lands on and the byte address
// the message starts at.  The work split and the state are k_xof's: one
// message per lane, 256-thread workgroups, no LDS, no barrier, lanes past the
// batch return at once; the 25 lanes of the state are indexed by compile-time
// constants only -- absorb, tail and squeeze are fully unrolled loops over the
// rate whose per-lane predicates are selects, never subscripts -- so nothing
// of it lives in scratch.  It calls ntt_xof.hpp's keccak_f1600,
// cshake_simple_prefix and XOF_PAD_LAST.
//
// Message b is msg[begin, end) with begin = min(off[b], msg_bytes) and end =
// min(max(off[b + 1], begin), msg_bytes): the clamps are the definition
// (qtesla_ntt.h), and with them no offset makes the kernel read outside msg.
// Offsets and lengths are 64-bit throughout.
//
// Realignment.  The message starts at byte a = begin & 7 of aligned word
// W = begin / 8.  Only aligned 8-byte loads are issued: message word t is bytes
// a .. a + 7 of the aligned pair (W + t, W + t + 1), taken with two
// v_alignbyte_b32 after one select per dword on a's bit 2 (a = 0 is the shift
// count 0 of that instruction, not a shift by 64).  The last aligned word of a
// rate block is carried into the next, so the first block costs R + 1 loads
// and every further one R.
//
// Which words are read.  Aligned word W + t + 1 holds a byte of the message iff
// 8 (t + 1) - a < L.  In a full rate block that holds for every word but, at
// a = 0 and a message that ends with the block, the last; that one load takes
// the word before it instead (its value is never used: at a = 0 the high word
// of a pair contributes no byte).  The last, partial block holds
// nv = ceil((r + a) / 8) - 1 such words (r = bytes left); a lane with nv = 0
// loads nothing, the others load word min(i, nv - 1) for i < R -- a whole block
// in flight under one branch, no branch per load -- and what such a load
// brings beyond the message is cut off by the tail mask.  A message of length
// 0 loads nothing at all, so with msg_bytes = 0 msg is never looked at.
//
// Different lengths per lane.  The block loop is divergent: a lane leaves it
// when fewer than `rate` bytes of its message remain and waits, its state
// untouched, until the longest message of its wave is through; then all lanes
// finalise together.  A wave therefore costs its longest message's chain of
// permutations.
//
// Tail.  With r = L mod rate bytes left: words below r / 8 whole, word r / 8
// masked to r & 7 bytes and XORed with the domain byte at bit 8 (r & 7), the
// words above it nothing; 0x80 into the rate's last byte as in k_xof (at
// r = rate - 1 both meet in one byte: 0x9F / 0x84).
#pragma once
#include "ntt_xof.hpp"

namespace qntt {

// bytes a .. a + 7 of the 16 bytes lo || hi (little-endian), 0 <= a <= 7
__device__ __forceinline__ uint64_t xof_align_bytes(uint64_t lo, uint64_t hi, uint32_t a)
{
    const bool up = (a & 4u) != 0;   // v_alignbyte_b32 takes a & 3
    const uint32_t d0 = (uint32_t)lo, d1 = (uint32_t)(lo >> 32), d2 = (uint32_t)hi, d3 = (uint32_t)(hi >> 32);
    const uint32_t e0 = up ? d1 : d0, e1 = up ? d2 : d1, e2 = up ? d3 : d2;
    return ((uint64_t)__builtin_amdgcn_alignbyte(e2, e1, a) << 32) | __builtin_amdgcn_alignbyte(e1, e0, a);
}

// out [batch][ow] 8-byte words; msg [msg_bytes / 8] aligned words, off [batch + 1];
// cstm < 0: SHAKE (domain byte 0x1F), else cSHAKE-simple (prefix block, 0x04)
template <int R>
__global__ __launch_bounds__(XOF_WG) void k_xof_ragged(uint64_t *__restrict__ out, uint32_t ow,
                                                       const uint64_t *__restrict__ msg, uint64_t msg_bytes,
                                                       const uint64_t *__restrict__ off, uint32_t batch, int cstm)
{
    constexpr uint64_t RATE = 8 * R;
    const uint32_t b = blockIdx.x * XOF_WG + threadIdx.x;
    if (b >= batch) return;
    const uint64_t o0 = off[b], o1 = off[b + 1];
    const uint64_t begin = o0 < msg_bytes ? o0 : msg_bytes;
    const uint64_t lim = o1 > begin ? o1 : begin;
    const uint64_t end = lim < msg_bytes ? lim : msg_bytes;
    const uint32_t a = (uint32_t)begin & 7u;
    uint64_t left = end - begin;             // bytes of the message not yet absorbed
    const uint64_t *p = msg + (begin >> 3);  // the aligned word the next block's first byte lies in
    uint64_t s[25] = {};
    uint64_t dom = 0x1F;
    if (cstm >= 0) {
        s[0] = cshake_simple_prefix<R>((uint32_t)cstm);
        keccak_f1600(s);
        dom = 0x04;
    }
    uint64_t carry = 0;
    if (left) carry = p[0];
#pragma unroll 1
    while (left >= RATE) {
        // word R of the block's R + 1 holds a byte of the message unless a = 0 and the message ends here
        const int last = (a || left > RATE) ? R : R - 1;
        uint64_t h[R];
#pragma unroll
        for (int i = 0; i < R - 1; ++i) h[i] = p[i + 1];
        h[R - 1] = p[last];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            s[i] ^= xof_align_bytes(carry, h[i], a);
            carry = h[i];
        }
        keccak_f1600(s);
        p += R;
        left -= RATE;
    }
    // the last block: r = left < RATE bytes, then the padding
    const uint32_t r = (uint32_t)left;
    const uint32_t rw = r >> 3, rb8 = (r & 7u) * 8;
    const uint32_t nv = (r + a + 7) / 8;   // aligned words from p on with a byte of the message: p[0] is `carry`
    uint64_t h[R] = {};
    if (nv > 1) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const uint32_t j = (uint32_t)i + 1 < nv ? (uint32_t)i + 1 : nv - 1;
            h[i] = p[j];
        }
    }
    const uint64_t tail = ((uint64_t)1 << rb8) - 1, domw = dom << rb8;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const uint64_t w = xof_align_bytes(carry, h[i], a);
        carry = h[i];
        s[i] ^= (uint32_t)i < rw ? w : ((uint32_t)i == rw ? (w & tail) ^ domw : 0);
    }
    s[R - 1] ^= XOF_PAD_LAST;
    keccak_f1600(s);
    uint64_t *o = out + (size_t)b * ow;
    uint32_t wl = ow;
#pragma unroll 1
    for (;;) {
#pragma unroll
        for (int i = 0; i < R; ++i)
            if ((uint32_t)i < wl) o[i] = s[i];
        if (wl <= (uint32_t)R) break;
        wl -= R;
        o += R;
        keccak_f1600(s);
    }
}

}  // namespace qntt
