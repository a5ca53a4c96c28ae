// family_probe.hip -- test-only library (lib/libqtesla_ntt_family.so, `make
// testlibs`): every transform and product kernel that csrc/ntt_kernels.hip
// compiles, launched by the family the caller names instead of the family the
// measured switch table (kLatTier, csrc/ntt_lat.hpp) selects for the batch,
// and the batch kernels at a chunk length the caller names instead of the one
// the device's CU count gives.  tests/test_gpu_family_probe.py runs all of
// them against the CPU oracle; the product reaches only the kernels its
// current table routes to.  The product headers are included unchanged;
// nothing here is linked into the product library and csrc/ is not touched,
// so the product's src= hash does not depend on this file.
//
//   family 2 / 3 / 4   the radix-4 / 8 / 16 one-polynomial-per-workgroup
//                      kernels (k_ntt_lat, k_poly_mul_lat; k_ntt_latr<.., 3 / 4>)
//   family 0           the batch kernels: k_ntt_fwd / k_ntt_inv / k_bitrev /
//                      k_poly_mul (n <= 2048); k_ntt_fwd_big / k_ntt_inv_big /
//                      k_bitrev_large, k_poly_mul_big (n = 4096) and
//                      k_poly_mul_large (n = 8192)
//
// The chunk is the only launch parameter a caller chooses: 0 is the product's
// rule (batch_shape / large_shape of ntt_kernels.hip restated over
// launch_shape(); tests bind the restatement to the product), 1 ..
// NTT_PPW_MAX the chunk itself, with the grid ceil_div(items, per * chunk)
// that the product launches on a device whose CU count gives that chunk.
// Grid and block are always computed here from the kernels' own constants, so
// no caller can hand a kernel a shape its bounds checks were not written for.
// (k_bitrev_large strides over the batch by its grid instead of walking a
// chunk: there `chunk` polynomials per workgroup means the grid
// ceil_div(batch, chunk).)
//
// The launch lines are those of LXform<PS>::run and LMul<PS>::run.
// NTT_MIN_WG_PER_CU and NTT_PPW_MAX live in ntt_kernels.hip, not in a header:
// they are restated below and the GPU test compares them with what
// ntt_build_info() reports ("ppw<=16 min_wg/cu=4").
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <type_traits>

#include "../../include/qtesla_ntt.h"
#include "../csrc/dev_tables.hpp"
#include "../csrc/launch_shape.hpp"
#include "../csrc/ntt_device.hpp"
#include "../csrc/ntt_large.hpp"
#include "../csrc/ntt_big.hpp"
#include "../csrc/ntt_lat.hpp"
#include "../csrc/ntt_latr.hpp"

#ifndef NTT_MIN_WG_PER_CU
#define NTT_MIN_WG_PER_CU 4
#endif
#ifndef NTT_PPW_MAX
#define NTT_PPW_MAX 16
#endif

namespace qntt {
namespace {

// kind of family_probe_xform; op of family_probe_shape = kind, or OP_MUL / OP_MUL_NTT
enum Op { OP_FWD, OP_INV, OP_FWD_BR, OP_INV_BR, OP_BITREV, OP_MUL, OP_MUL_NTT, NOPS };
static_assert((int)OP_FWD == (int)LAT_FWD && (int)OP_INV == (int)LAT_INV && (int)OP_FWD_BR == (int)LAT_FWD_BR &&
                  (int)OP_INV_BR == (int)LAT_INV_BR,
              "the product's transform kinds");

constexpr int kMaxDev = 64;
std::mutex g_mutex;
bool g_ready[kMaxDev];
int g_cus[kMaxDev];
int g_test_cus = 0;   // family_probe_set_cus: the CU count of shape queries (0: the device's)

// CU count of the current device; with_tables: this library's own copy of the
// device tables uploaded too (once per device)
int device_ready(int *cus, bool with_tables)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return NTT_ERR_HIP;
    std::lock_guard<std::mutex> lk(g_mutex);
    if (!g_cus[dev]) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return NTT_ERR_HIP;
        g_cus[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    if (with_tables && !g_ready[dev]) {
        Tables tabs[NPARAM_SETS];
        for (int i = 0; i < NPARAM_SETS; i++) make_tables(*param_set(i), tabs[i]);
        if (upload_device_tables(tabs) != hipSuccess) return NTT_ERR_HIP;
        g_ready[dev] = true;
    }
    *cus = g_cus[dev];
    return NTT_OK;
}

struct Shape {
    size_t grid;   // checked against the launch limit before it becomes a dim3
    uint32_t block, chunk, per;
};

// a chunked kernel: the product's rule (chunk 0) or the named chunk
Shape chunked(size_t items, int per, int block, size_t per_cu, int chunk, int cus)
{
    if (chunk == 0) {
        const LaunchShape l = launch_shape(items, per, cus, per_cu, NTT_PPW_MAX);
        return {l.grid, (uint32_t)block, l.chunk, (uint32_t)per};
    }
    return {ceil_div(items, (size_t)per * chunk), (uint32_t)block, (uint32_t)chunk, (uint32_t)per};
}

// the (family, op, parameter set, chunk) combinations that name a compiled kernel
bool valid(int family, int op, int ps, int chunk)
{
    const ParamSet *p = param_set(ps);
    if (!p || op < 0 || op >= NOPS || chunk < 0 || chunk > NTT_PPW_MAX) return false;
    if (family == 0) return true;
    if (chunk != 0) return false;                                                  // one polynomial per workgroup: no chunk
    if (family == 2) return op <= OP_INV_BR || (op >= OP_MUL && p->n <= 4096);    // k_poly_mul_lat: n <= 4096
    if (family == 3 || family == 4) return op <= OP_INV_BR;
    return false;
}

// Launch shape of a valid combination.  cus is read for family 0 with chunk 0 only.
template <int PS>
Shape shape_of(int family, int op, size_t batch, int chunk, int cus)
{
    using P = typename PSel<PS>::T;
    constexpr int L = P::LOGN;
    if (family == 2) return {batch, (uint32_t)LatGeo<L>::T, 1, 1};
    if (family == 3) return {batch, (uint32_t)LatRGeo<L, 3>::T, 1, 1};
    if (family == 4) return {batch, (uint32_t)LatRGeo<L, 4>::T, 1, 1};
    const bool bhat = op == OP_MUL_NTT;
    if constexpr (PS < LARGE_PS0) {
        // batch_shape: a unit is one n = 2048 polynomial or two n = 1024 polynomials
        const size_t units = ceil_div(batch, Lane<P>::UPW);
        if (op <= OP_BITREV) return chunked(units, NTT_WG / 64, NTT_WG, NTT_MIN_WG_PER_CU, chunk, cus);
        const int wg = bhat ? mul_wg<true>() : mul_wg<false>();
        return chunked(units, wg / 64, wg, NTT_MIN_WG_PER_CU, chunk, cus);
    } else {
        // large_shape: >= 2 workgroups per CU
        if (op <= OP_INV_BR) return chunked(batch, Big<PS>::WAVES, Big<PS>::NT, 2, chunk, cus);
        if (op == OP_BITREV) {   // one polynomial per workgroup step, the grid its stride
            const size_t g = chunk == 0 ? capped_grid(batch, 1, cus, 64) : ceil_div(batch, (size_t)chunk);
            return {g, 512, (uint32_t)(g ? ceil_div(batch, g) : 1), 1};
        }
        if constexpr (P::N == 4096) {
            const int waves = bhat ? big_mul_waves<true>() : big_mul_waves<false>();
            return chunked(batch, waves, waves * 64, 2, chunk, cus);
        } else {
            if (bhat) return chunked(batch, LargeMul<PS, true>::SLOTS, LargeMul<PS, true>::NT, 2, chunk, cus);
            return chunked(batch, LargeMul<PS, false>::SLOTS, LargeMul<PS, false>::NT, 2, chunk, cus);
        }
    }
}

template <class F> int with_ps(int ps, F &&f)
{
    switch (ps) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return NTT_ERR_PARAM;
    }
}

// the four transforms as template arguments: f(inverse, bit-reversed order)
template <class F> void with_xform(int k, F &&f)
{
    switch (k) {
    case OP_FWD: f(std::false_type{}, std::false_type{}); break;
    case OP_INV: f(std::true_type{}, std::false_type{}); break;
    case OP_FWD_BR: f(std::false_type{}, std::true_type{}); break;
    case OP_INV_BR: f(std::true_type{}, std::true_type{}); break;
    default: break;   // BITREV: a kernel of its own
    }
}
template <class F> void with_flag(bool v, F &&f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

// batch and launch size: batch <= 2^31 - 1, grid x block <= 2^32 - 1
bool launchable(size_t batch, const Shape &sh) { return batch <= (size_t)0x7FFFFFFF && sh.grid * sh.block <= (size_t)0xFFFFFFFFu; }

bool partial_overlap(const void *x, const void *y, size_t bytes)
{
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    if (a == b) return false;
    return a < b + bytes && b < a + bytes;
}

template <int PS>
void launch_xform(int family, int kind, const uint32_t *in, uint32_t *out, uint32_t nb, const Shape &sh, hipStream_t s)
{
    const dim3 g((uint32_t)sh.grid), b(sh.block);
    if (family == 2) {
        with_xform(kind, [&](auto inv, auto br) {
            hipLaunchKernelGGL((k_ntt_lat<PS, decltype(inv)::value, decltype(br)::value>), g, b, 0, s, in, out);
        });
    } else if (family == 3) {
        with_xform(kind, [&](auto inv, auto br) {
            hipLaunchKernelGGL((k_ntt_latr<PS, decltype(inv)::value, decltype(br)::value, 3>), g, b, 0, s, in, out);
        });
    } else if (family == 4) {
        with_xform(kind, [&](auto inv, auto br) {
            hipLaunchKernelGGL((k_ntt_latr<PS, decltype(inv)::value, decltype(br)::value, 4>), g, b, 0, s, in, out);
        });
    } else if constexpr (PS >= LARGE_PS0) {
        with_xform(kind, [&](auto inv, auto br) {
            constexpr bool BR = decltype(br)::value;
            if constexpr (decltype(inv)::value) hipLaunchKernelGGL((k_ntt_inv_big<PS, BR>), g, b, 0, s, in, out, nb, sh.chunk);
            else hipLaunchKernelGGL((k_ntt_fwd_big<PS, BR>), g, b, 0, s, in, out, nb, sh.chunk);
        });
        if (kind == OP_BITREV) hipLaunchKernelGGL(k_bitrev_large<PS>, g, b, 0, s, in, out, nb);
    } else {
        with_xform(kind, [&](auto inv, auto br) {
            constexpr bool BR = decltype(br)::value;
            if constexpr (decltype(inv)::value) hipLaunchKernelGGL((k_ntt_inv<PS, BR>), g, b, 0, s, in, out, nb, sh.chunk);
            else hipLaunchKernelGGL((k_ntt_fwd<PS, BR>), g, b, 0, s, in, out, nb, sh.chunk);
        });
        if (kind == OP_BITREV) hipLaunchKernelGGL(k_bitrev<PS>, g, b, 0, s, in, out, nb, sh.chunk);
    }
}

template <int PS>
void launch_mul(int family, bool bhat, const uint32_t *a, const uint32_t *b, uint32_t *c, uint32_t nb, const Shape &sh,
                hipStream_t s)
{
    constexpr int N = PSel<PS>::T::N;
    const dim3 g((uint32_t)sh.grid), blk(sh.block);
    if (family == 2) {
        if constexpr (N <= 4096)
            with_flag(bhat, [&](auto bh) {
                hipLaunchKernelGGL((k_poly_mul_lat<PS, decltype(bh)::value>), g, blk, 0, s, a, b, c);
            });
        return;
    }
    with_flag(bhat, [&](auto bh) {
        constexpr bool BHAT = decltype(bh)::value;
        if constexpr (PS >= LARGE_PS0 && N == 4096) hipLaunchKernelGGL((k_poly_mul_big<PS, BHAT>), g, blk, 0, s, a, b, c, nb, sh.chunk);
        else if constexpr (PS >= LARGE_PS0) hipLaunchKernelGGL((k_poly_mul_large<PS, BHAT>), g, blk, 0, s, a, b, c, nb, sh.chunk);
        else hipLaunchKernelGGL((k_poly_mul<PS, BHAT>), g, blk, 0, s, a, b, c, nb, sh.chunk);
    });
}

// Every check of a launch, in the ABI's order, then the device and the shape.
// ptrs: the operands, the output last.  NTT_OK with *go = false: an empty batch.
int prepare(int family, int op, int ps, const void *const *ptrs, int nptrs, size_t batch, int chunk, Shape *sh, bool *go)
{
    *go = false;
    if (!valid(family, op, ps, chunk)) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    for (int i = 0; i < nptrs; i++)
        if (!ptrs[i]) return NTT_ERR_NULL;
    for (int i = 0; i < nptrs; i++)
        if (((uintptr_t)ptrs[i]) & 3u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    // a named chunk (and every one-polynomial family) fixes the shape without the device
    const bool need_cus = family == 0 && chunk == 0;
    if (!need_cus) {
        with_ps(ps, [&](auto PSI) { return *sh = shape_of<decltype(PSI)::value>(family, op, batch, chunk, 0), 0; });
        if (!launchable(batch, *sh)) return NTT_ERR_SIZE;
    }
    const size_t bytes = batch * param_set(ps)->n * 4;
    for (int i = 0; i + 1 < nptrs; i++)
        if (partial_overlap(ptrs[i], ptrs[nptrs - 1], bytes)) return NTT_ERR_ALIAS;
    int cus = 0;
    const int rc = device_ready(&cus, true);
    if (rc != NTT_OK) return rc;
    if (need_cus) {
        with_ps(ps, [&](auto PSI) { return *sh = shape_of<decltype(PSI)::value>(family, op, batch, chunk, cus), 0; });
        if (!launchable(batch, *sh)) return NTT_ERR_SIZE;
    }
    *go = true;
    return NTT_OK;
}

}  // namespace
}  // namespace qntt

using namespace qntt;

// d_out = transform `kind` (0 FWD, 1 INV, 2 FWD_BR, 3 INV_BR; 4 BITREV, family 0
// only) of d_in by the kernels of `family`; d_out == d_in is in place.
extern "C" int family_probe_xform(int family, int kind, int ps, uint32_t *d_out, const uint32_t *d_in, size_t batch, int chunk,
                                  void *stream)
{
    if (kind < 0 || kind > OP_BITREV) return NTT_ERR_PARAM;
    const void *ptrs[2] = {d_in, d_out};
    Shape sh{};
    bool go;
    const int rc = prepare(family, kind, ps, ptrs, 2, batch, chunk, &sh, &go);
    if (rc != NTT_OK || !go) return rc;
    return with_ps(ps, [&](auto PSI) {
        launch_xform<decltype(PSI)::value>(family, kind, d_in, d_out, (uint32_t)batch, sh, (hipStream_t)stream);
        return hipGetLastError() == hipSuccess ? (int)NTT_OK : (int)NTT_ERR_HIP;
    });
}

// d_c = d_a d_b mod (x^n + 1, q) (bhat: d_b is poly_ntt's natural-order output)
// by the kernels of `family` (0, or 2 for n <= 4096); d_c may equal d_a or d_b.
extern "C" int family_probe_mul(int family, int bhat, int ps, uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b,
                                size_t batch, int chunk, void *stream)
{
    if (bhat < 0 || bhat > 1) return NTT_ERR_PARAM;
    const void *ptrs[3] = {d_a, d_b, d_c};
    Shape sh{};
    bool go;
    const int rc = prepare(family, bhat ? OP_MUL_NTT : OP_MUL, ps, ptrs, 3, batch, chunk, &sh, &go);
    if (rc != NTT_OK || !go) return rc;
    return with_ps(ps, [&](auto PSI) {
        launch_mul<decltype(PSI)::value>(family, bhat != 0, d_a, d_b, d_c, (uint32_t)batch, sh, (hipStream_t)stream);
        return hipGetLastError() == hipSuccess ? (int)NTT_OK : (int)NTT_ERR_HIP;
    });
}

// The shape family_probe_xform / _mul launch for (family, op, ps, batch,
// chunk): op = the transform kind, or 5 mul / 6 mul_ntt.  *per: work units
// (polynomials; pairs of polynomials at n = 1024) a workgroup takes per pass;
// *chunk_out: passes per workgroup.  An empty batch has grid 0.
extern "C" int family_probe_shape(int family, int op, int ps, size_t batch, int chunk, uint32_t *grid, uint32_t *block,
                                  uint32_t *chunk_out, uint32_t *per)
{
    if (!valid(family, op, ps, chunk)) return NTT_ERR_PARAM;
    if (!grid || !block || !chunk_out || !per) return NTT_ERR_NULL;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    int cus = g_test_cus;
    if (family == 0 && chunk == 0 && !cus) {
        const int rc = device_ready(&cus, false);
        if (rc != NTT_OK) return rc;
    }
    Shape sh{};
    with_ps(ps, [&](auto PSI) { return sh = shape_of<decltype(PSI)::value>(family, op, batch, chunk, cus), 0; });
    if (!launchable(batch, sh)) return NTT_ERR_SIZE;
    *grid = (uint32_t)sh.grid;
    *block = sh.block;
    *chunk_out = sh.chunk;
    *per = sh.per;
    return NTT_OK;
}

// Test argument of family_probe_shape only: the CU count its chunk-0 rule
// takes (1 .. 65536; 0: the current device's again).  Launches always use the
// device's.
extern "C" int family_probe_set_cus(int cus)
{
    if (cus < 0 || cus > 65536) return NTT_ERR_PARAM;
    g_test_cus = cus;
    return NTT_OK;
}

// The restated constants of ntt_kernels.hip: out[0] = NTT_MIN_WG_PER_CU, out[1] = NTT_PPW_MAX.
extern "C" int family_probe_consts(uint32_t *out)
{
    if (!out) return NTT_ERR_NULL;
    out[0] = NTT_MIN_WG_PER_CU;
    out[1] = NTT_PPW_MAX;
    return NTT_OK;
}

// this library's own copy of the n = 8192 slot-barrier expiry counter
extern "C" int family_probe_sync_expiries(uint32_t *count)
{
    if (!count) return NTT_ERR_NULL;
    return hipMemcpyFromSymbol(count, HIP_SYMBOL(g_slot_sync_expired), sizeof(uint32_t), 0, hipMemcpyDeviceToHost) != hipSuccess
               ? NTT_ERR_HIP
               : NTT_OK;
}
