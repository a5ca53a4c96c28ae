// ntt_sample.hpp -- qTESLA's masking-polynomial sampler sample_y over a batch
// (poly_sample_y): the signer's first step on the device.  The definition is
// restated in full in include/qtesla_ntt.h; tests/sample_model.py is the same
// statement in Python.
//
// Work split: one seed per lane, one wave per workgroup, keccak_f1600 of
// ntt_xof.hpp with the state in registers.  The first call squeezes 3 n bytes:
// draw d of it is the same three stream bytes for every lane, so the draw
// index, the block count and every tail predicate are wave-uniform; only the
// output index i (draws minus this lane's rejections) is per lane.  At rate
// 168 a block is 56 whole draws.  At rate 136 draws straddle blocks with a
// period of three blocks (408 bytes = 136 draws: 45, 45 and 46 draws complete
// in them), so the first call is unrolled over the period: every byte is
// picked by a compile-time index and the one or two bytes of a straddling
// draw are carried in a register.  Neither the state nor the bytes go to
// scratch.
//
// Stores.  With a row per lane, y[i++] = v writes 64 lanes x 4 bytes into 64
// different rows per instruction.  So while no lane of the wave rejects in a
// block, the block's draws go through a wave-private LDS tile instead: lane l
// writes draw J to tile[l * S + J] (S odd: conflict-free), and the tile is
// read back flat, element e = 64 t + lane of instruction t (conflict-free, a
// constant offset), which is draw e mod S of row e / S.  A store instruction
// then covers 64 consecutive elements of the tile: at most three rows, in runs
// that continue where the previous instruction stopped (S - D <= 2 elements
// per row are padding and store nothing).  Row r's run starts at that lane's
// own i, fetched with a wave shuffle; the stores are single dwords, so an i
// that an earlier rejection moved off a 16-byte boundary costs nothing extra.
// In a block in which any lane rejects (0.3 % of them at qTESLA's bits) each
// lane takes its own draws back from the tile and stores them one by one;
// a refill block, where the lanes need different numbers of draws, is drawn
// from the state with per-lane stores and does not touch the tile.
// Lanes past the batch hash message 0's seed, never reject, store nothing.
// (Per-lane stores for every block were built as the A/B partner and measured:
// DESIGN.md section 5j.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "ntt_xof.hpp"

namespace qntt {

constexpr int SAMPLE_WG = 64;   // one wave: the tile is wave-private

// the 32-bit word W of a squeezed block
template <int W> __device__ __forceinline__ uint32_t keccak_word(const uint64_t (&s)[25])
{
    return (uint32_t)(s[W / 2] >> (32 * (W % 2)));
}
// bytes O, O + 1, O + 2 of a squeezed block in bits 0 .. 23 (little-endian); the bits above are not defined
template <int O> __device__ __forceinline__ uint32_t keccak_le24(const uint64_t (&s)[25])
{
    constexpr int W = O / 4, SH = 8 * (O % 4);
    if constexpr (SH == 0) return keccak_word<W>(s);
    else if constexpr (SH == 8) return keccak_word<W>(s) >> 8;
    else return __builtin_amdgcn_alignbit(keccak_word<W + 1>(s), keccak_word<W>(s), SH);
}

// Block P of a period of the first call's stream at rate R lanes: CB bytes of its first draw came
// with the block before, D draws complete in it, LEFT bytes stay over for the next block.
template <int R, int P> struct SamplePhase {
    static constexpr int CB = (P * 8 * R) % 3;
    static constexpr int D = (8 * R + CB) / 3;
    static constexpr int LEFT = (8 * R + CB) % 3;
};
template <int R> struct SampleRate {
    static constexpr int PERIOD = (8 * R) % 3 ? 3 : 1;
    static constexpr int STRIDE = ((8 * R + 2) / 3) | 1;   // tile row, in words: odd, >= every D (57 / 47)
    static_assert(STRIDE > 32 && STRIDE < 64, "sample_flush steps rows by one or two per instruction");
};

// draw J of block P; `carry` holds the CB bytes that came with the block before
template <int R, int P, int J> __device__ __forceinline__ uint32_t sample_draw(const uint64_t (&s)[25], uint32_t carry)
{
    constexpr int CB = SamplePhase<R, P>::CB, O = 3 * J - CB;
    static_assert(O >= 0 || J == 0, "only the first draw straddles");
    if constexpr (O < 0) return carry | (keccak_le24<0>(s) << (8 * CB));
    else return keccak_le24<O>(s);
}

// what one lane carries through the kernel (everything but i and row is wave-uniform)
struct SampleLane {
    uint32_t *row;    // this lane's y[b]
    uint32_t *rows;   // y[b] of the wave's lane 0
    uint32_t nrows;   // rows of this wave inside the batch
    uint32_t n, q, mask, B;
    uint32_t lane;
    bool live;
    uint32_t i;       // coefficients written so far; n for a lane past the batch
    __device__ __forceinline__ uint32_t value(uint32_t v) const   // (v - B) mod q
    {
        const int32_t t = (int32_t)v - (int32_t)B;
        return (uint32_t)(t + ((t >> 31) & (int32_t)q));
    }
};

// the tile as 64 consecutive elements per store instruction; `width` draws per row are valid
template <int S> __device__ __forceinline__ void sample_flush(const uint32_t *tile, SampleLane &L, uint32_t width)
{
    __syncthreads();   // one wave: orders the lanes' tile writes before the flat reads
    uint32_t r = L.lane >= (uint32_t)S ? 1u : 0u, c = L.lane - r * S;
    // rolled in steps of four: unrolled to the end, the compiler hoists all S rows' addresses and
    // predicates (they depend on the lane alone) out of the kernel's loops, into 170 more registers
#pragma unroll 1
    for (int t0 = 0; t0 < S; t0 += 4) {
#pragma unroll
        for (int t = t0; t < t0 + 4; ++t) {
            if (t < S) {
                const uint32_t v = tile[t * SAMPLE_WG + L.lane];
                const uint32_t ir = __shfl(L.i, (int)r);
                if (c < width && r < L.nrows) L.rows[(size_t)r * L.n + ir + c] = L.value(v);
            }
            c += SAMPLE_WG - S;
            r += 1;
            if (c >= (uint32_t)S) {
                c -= S;
                r += 1;
            }
        }
    }
    // the next block's tile writes follow these reads in program order (same wave, LDS is in order)
    L.i += L.live ? width : 0u;
}

// one draw's masked value to this lane's row, unless it is the rejected one or the row is full
__device__ __forceinline__ void sample_store(uint32_t v, SampleLane &L)
{
    const bool take = v != L.mask && L.i < L.n;
    if (take) L.row[L.i] = L.value(v);
    L.i += take ? 1u : 0u;
}
template <int R, int P, int J>
__device__ __forceinline__ void sample_stage(const uint64_t (&s)[25], uint32_t carry, const SampleLane &L, uint32_t *tile,
                                             uint32_t &top)
{
    const uint32_t v = sample_draw<R, P, J>(s, carry) & L.mask;
    top = v > top ? v : top;
    tile[L.lane * SampleRate<R>::STRIDE + J] = v;
}

// The first min(limit, D) draws of block P (limit is wave-uniform).  TILE: through the tile, flat unless a lane
// rejects (the first call, where every live lane has room for all of them); otherwise straight from the state.
template <int R, int P, bool TILE, int... J>
__device__ __forceinline__ void sample_block(const uint64_t (&s)[25], uint32_t carry, uint32_t limit, SampleLane &L,
                                             uint32_t *tile, std::integer_sequence<int, J...>)
{
    constexpr int D = SamplePhase<R, P>::D;
    if constexpr (TILE) {
        uint32_t top = 0;
        (void)(((uint32_t)J < limit && (sample_stage<R, P, J>(s, carry, L, tile, top), true)) && ...);
        if (!__any(L.live && top == L.mask)) {
            sample_flush<SampleRate<R>::STRIDE>(tile, L, limit < (uint32_t)D ? limit : (uint32_t)D);
        } else {   // each lane takes its own draws back from the tile (its own writes: no barrier)
#pragma unroll 1
            for (uint32_t j = 0; j < (uint32_t)D && j < limit; ++j) sample_store(tile[L.lane * SampleRate<R>::STRIDE + j], L);
        }
    } else {
        (void)(((uint32_t)J < limit && (sample_store(sample_draw<R, P, J>(s, carry) & L.mask, L), true)) && ...);
    }
}

// Block P of the first call with `left` draws still to make; true when it was the last one.
template <int R, int P>
__device__ __forceinline__ bool sample_phase(uint64_t (&s)[25], uint32_t &carry, uint32_t &left, SampleLane &L, uint32_t *tile)
{
    using Ph = SamplePhase<R, P>;
    sample_block<R, P, true>(s, carry, left, L, tile, std::make_integer_sequence<int, Ph::D>{});
    if (left <= (uint32_t)Ph::D) return true;
    left -= Ph::D;
    if constexpr (Ph::LEFT > 0) carry = (uint32_t)(s[R - 1] >> (64 - 8 * Ph::LEFT));
    keccak_f1600(s);
    return false;
}

// y [batch][n]; seed [batch][sw] 8-byte words, 1 <= sw <= R - 1; nonces NULL or [batch]
template <int R>
__global__ __launch_bounds__(SAMPLE_WG) void k_sample_y(uint32_t *__restrict__ y, const uint64_t *__restrict__ seed, uint32_t sw,
                                                        const uint32_t *__restrict__ nonces, uint32_t nonce, uint32_t batch,
                                                        uint32_t n, uint32_t q, uint32_t bits, uint32_t refills_max)
{
    __shared__ uint32_t tile[SAMPLE_WG * SampleRate<R>::STRIDE];
    const uint32_t lane = threadIdx.x, b0 = blockIdx.x * SAMPLE_WG, b = b0 + lane;
    const bool live = b < batch;          // a tail lane stores nothing and reads nothing beyond the batch
    const uint32_t src = live ? b : 0;
    const uint64_t *sd = seed + (size_t)src * sw;
    const uint32_t cstm = ((((nonces ? nonces[src] : 0u) + nonce) & 0xFFu) << 8);
    SampleLane L = {y + (size_t)src * n, y + (size_t)b0 * n, batch - b0 < (uint32_t)SAMPLE_WG ? batch - b0 : (uint32_t)SAMPLE_WG,
                    n, q, (1u << bits) - 1u, (1u << (bits - 1)) - 1u, lane, live, live ? 0u : n};
#pragma unroll 1
    for (uint32_t r = 0; r <= refills_max; ++r) {   // r = 0: the first call, 3 n bytes; then one block per refill
        if (!__any(L.i < n)) break;
        uint64_t s[25] = {};
        s[0] = cshake_simple_prefix<R>(cstm + r);   // r <= 255 stays inside this nonce's range
        keccak_f1600(s);
        const uint32_t swb = sw + (r >> 16);        // as in k_challenge: keeps the absorb predicates out of the loop's SGPRs
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if ((uint32_t)k < swb) s[k] ^= sd[k];
            if ((uint32_t)k == swb) s[k] ^= 0x04;
        }
        s[R - 1] ^= XOF_PAD_LAST;
        keccak_f1600(s);
        if (r == 0) {
            uint32_t left = n, carry = 0;
#pragma unroll 1
            for (;;) {
                if (sample_phase<R, 0>(s, carry, left, L, tile)) break;
                if constexpr (SampleRate<R>::PERIOD == 3) {
                    if (sample_phase<R, 1>(s, carry, left, L, tile)) break;
                    if (sample_phase<R, 2>(s, carry, left, L, tile)) break;
                }
            }
        } else {
            constexpr int D = SamplePhase<R, 0>::D;   // 56 draws; 45 draws, byte 135 unused
            sample_block<R, 0, false>(s, 0u, (uint32_t)D, L, tile, std::make_integer_sequence<int, D>{});
        }
    }
    for (; L.i < n; ++L.i) L.row[L.i] = 0;   // the refill bound was reached (not by hash outputs: qtesla_ntt.h)
}

}  // namespace qntt
