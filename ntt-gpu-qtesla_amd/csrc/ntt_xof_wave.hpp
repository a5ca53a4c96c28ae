// ntt_xof_wave.hpp -- SHAKE128 / SHAKE256 / cSHAKE-simple for small batches:
// the Keccak state spread over the lanes of a wave, two messages per wave
// (k_xof_wave, k_xof_ragged_wave).
//
// k_xof / k_xof_ragged keep one message's 25 words in one lane and walk about
// 6 240 dependent VALU instructions per permutation, whatever the batch.  Here
// word i = x + 5 y of a message is one uint64_t (2 VGPRs) of one lane of a
// 32-lane half of the wave, and messages 2 w and 2 w + 1 share wave w.  A round
// in gather form, g(v, j) meaning "every lane reads v of the lane that holds
// word j":
//
//   s1 = a ^ g(a, (i + 5) % 25)
//   C  = s1 ^ g(s1, (i + 10) % 25) ^ g(a, (i + 20) % 25)      column parity, in every lane of the column
//   D  = g(C, (x + 4) % 5 + 5 y) ^ rotl1(g(C, (x + 1) % 5 + 5 y))
//   r  = rotl(a ^ D, rho[i])                                  per-lane count
//   b  = g(r, src(i))                                         pi, inverted: src(j) = (j % 5 + 3 (j / 5)) % 5 + 5 (j % 5)
//   a  = b ^ (~g(b, (x + 1) % 5 + 5 y) & g(b, (x + 2) % 5 + 5 y))
//   word 0: a ^= RC[round]
//
// tests/keccak_wave_model.py is the same text in Python.
//
// Placement.  Word i sits in lane i + (i >= 15) of its half: rows y = 0, 1, 2
// in lanes 0 .. 14, rows 3 and 4 in lanes 16 .. 25, so that no row of five
// straddles a 16-lane DPP row.  Lanes 15 and 26 .. 31 are passengers: their
// gather addresses point at themselves and their content is never used.  The
// gathers down a column and pi's are ds_bpermute_b32 (the LDS crossbar, no LDS
// allocation): three dependent levels per round.  The gathers along a row --
// x - 1 and x + 1 of C, x + 1 and x + 2 of b -- are DPP row shifts: word
// (x + k) % 5 of the row is lane + k where x + k < 5 and lane + k - 5 otherwise,
// two v_mov_b32_dpp and a select per dword, no trip through the crossbar.
//
// A gather from an inactive lane returns 0, so all 64 lanes stay active
// through every permutation: there is no early return for a half without a
// message (an odd batch's last wave) and no divergent branch round a
// permutation; loads and stores are predicated instead.  In the ragged kernel
// the two messages of a wave may differ in length: the block loop runs to the
// longer one, and the half that has finished absorbing keeps its state across
// the other's permutations by a select.
//
// The per-lane rotate count is a run-time value: rotl by n is a right rotation
// by (64 - n) & 63 = 32 s + k, a swap of the dwords if s, then two
// v_alignbit_b32 by k -- k = 0 is that instruction's shift count 0, so the
// counts 0 and 32 need no case of their own.  The round constants are a
// constexpr table read through the scalar cache, as in keccak_f1600.  That
// table and ntt_xof_ragged.hpp's xof_align_bytes are copies here, not shared:
// the one is local to its function, and a second caller of the other changes
// the code the compiler makes for k_xof_ragged, which stays as it is.
//
// Absorb: the lane of word j < R loads message word t + j, so a rate block is
// one contiguous 136 / 168-byte read per half; the next block's words are
// loaded before the permutation of the current one and waited for after it.
// Squeeze: the lanes of words j < R store word j, every output word once.
#pragma once
#include "ntt_xof.hpp"

namespace qntt {

constexpr int XOF_WAVE_WG = 64;   // one wave, two messages, per workgroup
static_assert(XOF_WAVE_WG % 64 == 0, "whole waves");

// rho offsets packed six bits apiece, ten to a word: word k holds lanes 10 k .. 10 k + 9
constexpr uint64_t keccak_rho_pack(int k)
{
    uint64_t w = 0;
    for (int j = 0; j < 10; ++j)
        if (10 * k + j < 25) w |= (uint64_t)KeccakRho::R[10 * k + j] << (6 * j);
    return w;
}

constexpr uint32_t KECCAK_WAVE_IDLE = 31;   // `word` of a passenger lane: above every rate

// what a lane knows of its place in the state: the gather addresses (byte
// addresses, lane * 4, of ds_bpermute_b32) and its rotation, computed once
struct KeccakWaveLane {
    int up5, up10, up20;   // rows y + 1, y + 2, y + 4 of the column
    int pi;                // src(i)
    uint32_t rot;          // right rotation (64 - rho[i]) & 63
    uint32_t word;         // i = x + 5 y, KECCAK_WAVE_IDLE for a passenger
    uint32_t x;            // i % 5
    uint32_t half;         // 0 / 1: which message of the wave
};

__device__ __forceinline__ KeccakWaveLane keccak_wave_lane(uint32_t lane)
{
    const uint32_t base = lane & 32u, l = lane & 31u;
    const bool st = l != 15 && l < 26;
    const uint32_t i = st ? l - (l > 15) : 0;
    const uint32_t x = i % 5;
    auto at = [&](uint32_t j) { return (int)(((st ? j + (j >= 15) : l) + base) * 4); };   // the lane of word j
    const uint64_t pack = i < 10 ? keccak_rho_pack(0) : (i < 20 ? keccak_rho_pack(1) : keccak_rho_pack(2));
    const uint32_t rho = (uint32_t)(pack >> (6 * (i % 10))) & 63u;
    KeccakWaveLane L;
    L.up5 = at((i + 5) % 25);
    L.up10 = at((i + 10) % 25);
    L.up20 = at((i + 20) % 25);
    L.pi = at((x + 3 * (i / 5)) % 5 + 5 * x);
    L.rot = (64u - rho) & 63u;
    L.word = st ? i : KECCAK_WAVE_IDLE;
    L.x = x;
    L.half = lane >> 5;
    return L;
}

// every lane reads v of the lane at byte address `addr`
__device__ __forceinline__ uint64_t keccak_gather(uint64_t v, int addr)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

constexpr int DPP_ROW_SHL = 0x100, DPP_ROW_SHR = 0x110;   // lane + n, lane - n of the 16-lane row (0 from outside it)

template <int CTRL> __device__ __forceinline__ uint64_t keccak_dpp(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, true);
    return ((uint64_t)hi << 32) | lo;
}

// every lane reads v of word (x + K) % 5 of its row: lane + K, or lane + K - 5 where the row wraps
template <int K> __device__ __forceinline__ uint64_t keccak_row(uint64_t v, uint32_t x)
{
    static_assert(K >= 1 && K <= 4, "row step");
    const uint64_t ahead = keccak_dpp<DPP_ROW_SHL + K>(v), behind = keccak_dpp<DPP_ROW_SHR + 5 - K>(v);
    return x + K >= 5 ? behind : ahead;
}

// v rotated right by the per-lane count n, 0 <= n < 64
__device__ __forceinline__ uint64_t rotr64_var(uint64_t v, uint32_t n)
{
    const bool swap = (n & 32u) != 0;
    const uint32_t l = (uint32_t)v, h = (uint32_t)(v >> 32);
    const uint32_t lo = swap ? h : l, hi = swap ? l : h;   // v_alignbit_b32 takes n & 31
    return ((uint64_t)__builtin_amdgcn_alignbit(lo, hi, n) << 32) | __builtin_amdgcn_alignbit(hi, lo, n);
}

// Keccak-f[1600] of the wave's two states; every lane of the wave must be active
__device__ __forceinline__ uint64_t keccak_f1600_wave(uint64_t a, const KeccakWaveLane &L)
{
    static constexpr uint64_t RC[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
        0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
        0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
        0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
        0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    const uint64_t first = L.word == 0 ? ~(uint64_t)0 : 0;   // a mask, not a select: the constant is loaded by every lane, at the top of the round
#pragma unroll 1
    for (int r = 0; r < 24; ++r) {
        const uint64_t rc = RC[r];
        const uint64_t s1 = a ^ keccak_gather(a, L.up5);
        const uint64_t c = s1 ^ keccak_gather(s1, L.up10) ^ keccak_gather(a, L.up20);
        const uint64_t d = keccak_row<4>(c, L.x) ^ rotl64<1>(keccak_row<1>(c, L.x));
        const uint64_t b = keccak_gather(rotr64_var(a ^ d, L.rot), L.pi);
        a = b ^ (~keccak_row<1>(b, L.x) & keccak_row<2>(b, L.x));
        a ^= rc & first;
    }
    return a;
}

// The wave's index in the grid, as a scalar.  batch goes up to 2^31 - 1, so
// there are up to 2^30 waves and 64 times as many threads: 32 bits hold neither
// a thread index nor the threads of one grid dimension (a launch is cut to
// 2^32 - 1 threads per dimension).  The grid is therefore rows of
// XOF_WAVE_GRID_X workgroups, and the index is made from workgroup indices.
constexpr uint32_t XOF_WAVE_GRID_X = 1u << 20;
__device__ __forceinline__ uint32_t xof_wave_index()
{
    const uint32_t wg = blockIdx.y * XOF_WAVE_GRID_X + blockIdx.x;
    return __builtin_amdgcn_readfirstlane(wg * (uint32_t)(XOF_WAVE_WG / 64) + (threadIdx.x >> 6));
}

// squeeze ow words per message: lanes j < R of a live half store word j of each block
template <int R>
__device__ __forceinline__ void xof_wave_squeeze(uint64_t a, const KeccakWaveLane &L, uint64_t *o, uint32_t ow, bool live)
{
    uint32_t left = ow;
#pragma unroll 1
    for (;;) {
        if (live && L.word < (uint32_t)R && L.word < left) o[L.word] = a;
        if (left <= (uint32_t)R) break;
        left -= R;
        o += R;
        a = keccak_f1600_wave(a, L);
    }
}

// k_xof's arguments and result, two messages per wave; launched with ceil(batch / 2) waves
template <int R>
__global__ __launch_bounds__(XOF_WAVE_WG) void k_xof_wave(uint64_t *__restrict__ out, uint32_t ow,
                                                          const uint64_t *__restrict__ in0, uint32_t w0,
                                                          const uint64_t *__restrict__ in1, uint32_t w1, uint32_t batch,
                                                          int cstm)
{
    const uint32_t wave = xof_wave_index();
    if (2 * wave >= batch) return;   // the whole wave: the grid is rounded up to workgroups and rows
    const KeccakWaveLane L = keccak_wave_lane(threadIdx.x & 63u);
    const uint32_t b = 2 * wave + L.half;
    const bool live = b < batch;
    const uint64_t *p0 = in0 + (size_t)b * w0;
    const uint64_t *p1 = in1 + (size_t)b * w1;
    const uint32_t words = w0 + w1;
    // message word t + lane of a block, 0 where the lane has none
    auto word = [&](uint32_t t) -> uint64_t {
        const uint32_t k = t + L.word;
        if (!live || L.word >= (uint32_t)R || k >= words) return 0;
        return k < w0 ? p0[k] : p1[k - w0];
    };
    uint64_t a = 0;
    uint64_t dom = 0x1F;
    if (cstm >= 0) {
        a = L.word == 0 ? cshake_simple_prefix<R>((uint32_t)cstm) : 0;
        a = keccak_f1600_wave(a, L);
        dom = 0x04;
    }
    uint32_t t = 0;
    uint64_t m = word(0);
#pragma unroll 1
    for (; words - t >= (uint32_t)R; t += R) {
        a ^= m;
        m = word(t + R);   // in flight across the permutation
        a = keccak_f1600_wave(a, L);
    }
    const uint32_t rem = words - t;   // < R: the last block holds rem words, then the padding
    a ^= m;
    a ^= L.word == rem ? dom : 0;
    a ^= L.word == (uint32_t)R - 1 ? XOF_PAD_LAST : 0;
    a = keccak_f1600_wave(a, L);
    xof_wave_squeeze<R>(a, L, out + (size_t)b * ow, ow, live);
}

// bytes a .. a + 7 of the 16 bytes lo || hi (little-endian), 0 <= a <= 7: ntt_xof_ragged.hpp's xof_align_bytes
__device__ __forceinline__ uint64_t xof_wave_align_bytes(uint64_t lo, uint64_t hi, uint32_t a)
{
    const bool up = (a & 4u) != 0;   // v_alignbyte_b32 takes a & 3
    const uint32_t d0 = (uint32_t)lo, d1 = (uint32_t)(lo >> 32), d2 = (uint32_t)hi, d3 = (uint32_t)(hi >> 32);
    const uint32_t e0 = up ? d1 : d0, e1 = up ? d2 : d1, e2 = up ? d3 : d2;
    return ((uint64_t)__builtin_amdgcn_alignbyte(e2, e1, a) << 32) | __builtin_amdgcn_alignbyte(e1, e0, a);
}

// one half's message in k_xof_ragged_wave: where it starts and how long it is
struct XofRaggedSpan {
    const uint64_t *p;   // the aligned word the message's first byte lies in
    uint32_t a;          // that byte's place in it
    uint64_t len;        // bytes
};

// The lane's word of the rate block that starts at message byte `pos`: raw
// aligned words first (`load`), cut and padded after the permutation (`cook`).
// Aligned word k of the span holds a byte of the message iff 8 k < a + len (and
// len > 0); nothing else is loaded.
struct XofRaggedRaw {
    uint64_t lo, hi;
};

template <int R>
__device__ __forceinline__ XofRaggedRaw xof_ragged_wave_load(const XofRaggedSpan &s, const KeccakWaveLane &L, uint64_t pos)
{
    XofRaggedRaw w = {0, 0};
    const uint64_t nw = s.len ? (s.a + s.len + 7) >> 3 : 0;   // aligned words with a byte of the message
    const uint64_t k = (pos >> 3) + L.word;
    if (L.word < (uint32_t)R) {
        if (k < nw) w.lo = s.p[k];
        if (k + 1 < nw) w.hi = s.p[k + 1];
    }
    return w;
}

// the bytes of the message in that word, then the domain byte at byte len and 0x80 in the rate's last byte
template <int R>
__device__ __forceinline__ uint64_t xof_ragged_wave_cook(const XofRaggedRaw &w, const XofRaggedSpan &s, const KeccakWaveLane &L,
                                                         uint64_t pos, uint64_t dom)
{
    const uint64_t at = pos + 8 * (uint64_t)L.word;   // the message byte this lane's word starts at
    if (L.word >= (uint32_t)R) return 0;
    uint64_t v = xof_wave_align_bytes(w.lo, w.hi, s.a);
    if (at >= s.len) {
        v = 0;
    } else if (s.len - at < 8) {
        v &= ((uint64_t)1 << (8 * (uint32_t)(s.len - at))) - 1;
    }
    if (s.len - pos < (uint64_t)(8 * R)) {   // the message ends in this block (pos <= len always)
        if (at <= s.len && s.len - at < 8) v ^= dom << (8 * (uint32_t)(s.len - at));
        if (L.word == (uint32_t)R - 1) v ^= XOF_PAD_LAST;
    }
    return v;
}

// k_xof_ragged's arguments and result, two messages per wave; launched with ceil(batch / 2) waves
template <int R>
__global__ __launch_bounds__(XOF_WAVE_WG) void k_xof_ragged_wave(uint64_t *__restrict__ out, uint32_t ow,
                                                                 const uint64_t *__restrict__ msg, uint64_t msg_bytes,
                                                                 const uint64_t *__restrict__ off, uint32_t batch, int cstm)
{
    constexpr uint64_t RATE = 8 * R;
    const uint32_t wave = xof_wave_index();
    if (2 * wave >= batch) return;   // the whole wave: the grid is rounded up to workgroups and rows
    const KeccakWaveLane L = keccak_wave_lane(threadIdx.x & 63u);
    // both messages' spans in every lane (scalar loads): the loop bound below is wave-uniform
    const uint32_t b0 = 2 * wave;
    const bool two = b0 + 1 < batch;
    const uint64_t o[3] = {off[b0], off[b0 + 1], off[two ? b0 + 2 : b0 + 1]};
    uint64_t begin[2], len[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        begin[h] = o[h] < msg_bytes ? o[h] : msg_bytes;
        const uint64_t lim = o[h + 1] > begin[h] ? o[h + 1] : begin[h];
        len[h] = (lim < msg_bytes ? lim : msg_bytes) - begin[h];
    }
    if (!two) len[1] = 0;
    const bool live = L.half == 0 || two;
    const uint64_t mybegin = L.half ? begin[1] : begin[0];
    const XofRaggedSpan s = {msg + (mybegin >> 3), (uint32_t)mybegin & 7u, L.half ? len[1] : len[0]};
    const uint64_t myblocks = s.len / RATE + 1;   // the last one holds the padding
    const uint64_t longer = len[0] > len[1] ? len[0] : len[1];
    const uint64_t blocks = longer / RATE + 1;
    uint64_t a = 0;
    uint64_t dom = 0x1F;
    if (cstm >= 0) {
        a = L.word == 0 ? cshake_simple_prefix<R>((uint32_t)cstm) : 0;
        a = keccak_f1600_wave(a, L);
        dom = 0x04;
    }
    XofRaggedRaw w = xof_ragged_wave_load<R>(s, L, 0);
#pragma unroll 1
    for (uint64_t blk = 0; blk < blocks; ++blk) {
        const bool mine = blk < myblocks;
        const uint64_t pos = blk * RATE;
        const uint64_t before = a;
        a ^= mine ? xof_ragged_wave_cook<R>(w, s, L, pos, dom) : 0;
        if (blk + 1 < myblocks) w = xof_ragged_wave_load<R>(s, L, pos + RATE);   // in flight across the permutation
        a = keccak_f1600_wave(a, L);
        a = mine ? a : before;   // a finished half waits for the longer message
    }
    xof_wave_squeeze<R>(a, L, out + (size_t)(b0 + L.half) * ow, ow, live);
}

}  // namespace qntt
