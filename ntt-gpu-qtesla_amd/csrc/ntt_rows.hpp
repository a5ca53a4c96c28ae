// ntt_rows.hpp -- the logic between the steps of a chain, on the device: row
// tests (ntt_rows_over, ntt_rows_differ), flags to an ascending index list
// (ntt_select) and row moves by index (ntt_rows_move).  Nothing here knows a
// parameter set or a scheme: widths, strides and counts are arguments, indices
// and counts are data, and no value of either makes a kernel read or write
// outside the extents the host was given (qtesla_ntt.h states them).
//
// Every output word is written by a plain vector store of the one thread that
// owns it; there is no atomic, no scratch buffer, and no workgroup waits on
// another.  The three grid kernels stride over their rows (a capped grid, as
// k_pointwise), so a batch of 2^31 - 1 rows needs no second grid dimension.
//
// k_rows_over     a thread per row of m values; the m bounds travel by value.
// k_rows_differ   2^llpr lanes per row (the host takes the smallest power of
//                 two that covers the row's dwords, at most a wave): each ORs
//                 the XOR of its dwords, a butterfly of __shfl_xor below the
//                 group width joins them, lane 0 of the group stores.  The
//                 groups of a wave leave the row loop at different times; a
//                 shuffle never crosses a group, and a group is active or not
//                 as a whole.
// k_select        ONE workgroup of SELECT_WG threads walks the flags in tiles
//                 of SELECT_TILE = SELECT_SUB * SELECT_WG, sub-tile j of a tile
//                 being its flags [j SELECT_WG, (j + 1) SELECT_WG): thread t
//                 holds flag j SELECT_WG + t of each, so its loads are
//                 coalesced and index order is (sub-tile, wave, lane).  Per
//                 sub-tile a __ballot gives the wave's count (popcount) and the
//                 lane's rank below it (popcount under the lane's mask); the
//                 SELECT_SUB * SELECT_WAVES = 64 counts go to LDS, and after one
//                 barrier every wave scans all 64 itself -- one count per lane,
//                 six __shfl_up steps -- and reads its own offsets and the
//                 tile's total out of the scan.  The running offset is a
//                 register every thread carries.  The counts are double
//                 buffered, so a tile costs one barrier, and the next tile's
//                 flags are loaded before the current one's are ranked.
// k_rows_move     2^llpr lanes per row (at most the workgroup) copy it in
//                 16-byte or 4-byte units; the device count trims the host's,
//                 an index at or past its side's row count skips the row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qntt {

constexpr int ROWS_WG = 256;
constexpr int ROWS_M_MAX = 16;   // NTT_ROWS_M_MAX

struct RowBounds {
    uint64_t b[ROWS_M_MAX];
};

// flag [batch]; vals [batch][m] of T (uint32_t / uint64_t); a bound at or above T's maximum never flags
template <class T>
__global__ __launch_bounds__(ROWS_WG) void k_rows_over(uint32_t *__restrict__ flag, const T *__restrict__ vals, uint32_t m,
                                                       RowBounds bounds, uint32_t accumulate, uint32_t batch)
{
    const uint32_t step = gridDim.x * ROWS_WG;
#pragma unroll 1
    for (size_t b = (size_t)blockIdx.x * ROWS_WG + threadIdx.x; b < batch; b += step) {
        const T *row = vals + b * m;
        uint32_t f = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < m; ++j) f |= (uint32_t)((uint64_t)row[j] > bounds.b[j]);
        flag[b] = accumulate ? (flag[b] | f) : f;
    }
}

// flag [batch]; rows of `words` dwords at a + b a_words_stride and b + b b_words_stride (strides in dwords)
__global__ __launch_bounds__(ROWS_WG) void k_rows_differ(uint32_t *__restrict__ flag, const uint32_t *a, size_t a_stride,
                                                         const uint32_t *b, size_t b_stride, size_t words,
                                                         uint32_t accumulate, uint32_t batch, uint32_t llpr)
{
    const uint32_t lpr = 1u << llpr, sub = threadIdx.x & (lpr - 1);
    const size_t step = (size_t)gridDim.x * (ROWS_WG >> llpr);
#pragma unroll 1
    for (size_t r = (size_t)blockIdx.x * (ROWS_WG >> llpr) + (threadIdx.x >> llpr); r < batch; r += step) {
        const uint32_t *pa = a + r * a_stride, *pb = b + r * b_stride;
        uint32_t x = 0;
#pragma unroll 1
        for (size_t u = sub; u < words; u += lpr) x |= pa[u] ^ pb[u];
#pragma unroll 1
        for (uint32_t s = 1; s < lpr; s <<= 1) x |= (uint32_t)__shfl_xor((int)x, (int)s, 64);
        if (sub == 0) {
            const uint32_t f = x != 0;
            flag[r] = accumulate ? (flag[r] | f) : f;
        }
    }
}

constexpr int SELECT_WAVES = 16;
constexpr int SELECT_WG = SELECT_WAVES * 64;
constexpr int SELECT_SUB = 4;
constexpr int SELECT_TILE = SELECT_SUB * SELECT_WG;
static_assert(SELECT_SUB * SELECT_WAVES == 64, "a wave scans the tile's counts, one per lane");

// idx [batch] (words idx[count ..) untouched), count [1], flag [batch], bump NULL or [batch]; one workgroup
__global__ __launch_bounds__(SELECT_WG) void k_select(uint32_t *__restrict__ idx, uint32_t *__restrict__ count,
                                                      const uint32_t *__restrict__ flag, uint32_t want,
                                                      uint32_t *__restrict__ bump, uint32_t batch)
{
    __shared__ uint32_t s_cnt[2][64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t below = ((uint64_t)1 << lane) - 1;   // the lanes before this one
    uint32_t base = 0;                                  // selected so far, the same in every thread
    uint32_t nxt[SELECT_SUB];
#pragma unroll
    for (int j = 0; j < SELECT_SUB; ++j) {
        const uint32_t i = (uint32_t)j * SELECT_WG + tid;
        nxt[j] = i < batch ? flag[i] : 0;
    }
    uint32_t buf = 0;
#pragma unroll 1
    for (uint32_t t0 = 0; t0 < batch; t0 += SELECT_TILE, buf ^= 1) {   // batch <= 2^31 - 1: t0 + SELECT_TILE fits
        bool sel[SELECT_SUB];
        uint32_t rank[SELECT_SUB];
#pragma unroll
        for (int j = 0; j < SELECT_SUB; ++j) {
            const uint32_t i = t0 + (uint32_t)j * SELECT_WG + tid;
            sel[j] = i < batch && (uint32_t)(nxt[j] != 0) == want;
            const uint64_t mask = __ballot(sel[j]);
            rank[j] = (uint32_t)__popcll(mask & below);
            if (lane == 0) s_cnt[buf][j * SELECT_WAVES + wv] = (uint32_t)__popcll(mask);
        }
#pragma unroll
        for (int j = 0; j < SELECT_SUB; ++j) {
            const uint32_t i = t0 + SELECT_TILE + (uint32_t)j * SELECT_WG + tid;
            nxt[j] = i < batch ? flag[i] : 0;
        }
        __syncthreads();
        // inclusive scan of the tile's 64 counts, one per lane, in every wave
        uint32_t incl = s_cnt[buf][lane];
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, s, 64);
            incl += lane >= (uint32_t)s ? up : 0;
        }
#pragma unroll
        for (int j = 0; j < SELECT_SUB; ++j) {
            const uint32_t e = (uint32_t)j * SELECT_WAVES + wv;   // wave-uniform
            const uint32_t before = e ? (uint32_t)__shfl((int)incl, (int)e - 1, 64) : 0;
            if (sel[j]) {
                const uint32_t i = t0 + (uint32_t)j * SELECT_WG + tid;
                idx[base + before + rank[j]] = i;
                if (bump) bump[i] += 1;
            }
        }
        base += (uint32_t)__shfl((int)incl, 63, 64);
    }
    if (tid == 0) count[0] = base;
}

// rows of `units` V (uint4 / uint32_t) each; strides in bytes, multiples of sizeof(V); dcount NULL or [1]
template <class V>
__global__ __launch_bounds__(ROWS_WG) void k_rows_move(uint8_t *__restrict__ dst, size_t dst_stride,
                                                       const uint32_t *__restrict__ dst_idx, size_t dst_rows,
                                                       const uint8_t *__restrict__ src, size_t src_stride,
                                                       const uint32_t *__restrict__ src_idx, size_t src_rows, size_t units,
                                                       const uint32_t *__restrict__ dcount, uint32_t count, uint32_t llpr)
{
    const uint32_t lpr = 1u << llpr, sub = threadIdx.x & (lpr - 1);
    const size_t step = (size_t)gridDim.x * (ROWS_WG >> llpr);
    uint32_t lim = count;
    if (dcount) {
        const uint32_t dc = dcount[0];
        lim = dc < lim ? dc : lim;
    }
#pragma unroll 1
    for (size_t i = (size_t)blockIdx.x * (ROWS_WG >> llpr) + (threadIdx.x >> llpr); i < lim; i += step) {
        const size_t si = src_idx ? (size_t)src_idx[i] : i, di = dst_idx ? (size_t)dst_idx[i] : i;
        if (si >= src_rows || di >= dst_rows) continue;   // the definition: such a row is skipped
        const V *s = reinterpret_cast<const V *>(src + si * src_stride);
        V *d = reinterpret_cast<V *>(dst + di * dst_stride);
#pragma unroll 1
        for (size_t u = sub; u < units; u += lpr) d[u] = s[u];
    }
}

}  // namespace qntt
