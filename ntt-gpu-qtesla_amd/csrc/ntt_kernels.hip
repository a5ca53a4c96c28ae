// ntt_kernels.hip -- host side of the gfx950 batched negacyclic NTT library:
// per-device table upload, launch shapes, argument checks and the C ABI of
// include/qtesla_ntt.h.  The kernels themselves are in ntt_device.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <type_traits>

#include "../../include/qtesla_ntt.h"
#include "dev_tables.hpp"
#include "launch_shape.hpp"
#include "ntt_device.hpp"
#include "ntt_large.hpp"
#include "ntt_big.hpp"
#include "ntt_lat.hpp"
#include "ntt_latr.hpp"
#include "ntt_mulk.hpp"
#include "ntt_mulkl.hpp"
#include "ntt_pack.hpp"
#include "ntt_round.hpp"
#include "ntt_rows.hpp"
#include "ntt_gauss.hpp"
#include "ntt_gen_a.hpp"
#include "ntt_sample.hpp"
#include "ntt_unpack_ntt.hpp"
#include "ntt_xof.hpp"
#include "ntt_xof_ragged.hpp"
#include "ntt_xof_wave.hpp"
#include "ntt_internal.h"
#include "params.hpp"
#include "pset.hpp"

#ifndef QNTT_SRC_HASH
#define QNTT_SRC_HASH "unknown"   // set by the Makefile: sha256 of the library sources
#endif
#define QNTT_STR2(x) #x
#define QNTT_STR(x) QNTT_STR2(x)

namespace qntt {
namespace {

thread_local int t_last_hip = 0;

int hip_err(hipError_t e)
{
    t_last_hip = (int)e;
    return NTT_ERR_HIP;
}

constexpr int kMaxDev = 64;

std::once_flag g_cpu_tables_once;
Tables g_cpu_tables[NPARAM_SETS];

const Tables &cpu_tables(int ps)
{
    std::call_once(g_cpu_tables_once, [] {
        for (int i = 0; i < NPARAM_SETS; i++) make_tables(*param_set(i), g_cpu_tables[i]);
    });
    return g_cpu_tables[ps];
}

// Per-device state: tables uploaded (retried after a failed attempt, e.g. a
// first call made while another stream was being captured) and the launch
// geometry of the device.  `ready` is published with release order once both
// are done, so every later call on that device -- from any host thread, on
// any stream -- takes the lock-free acquire-load path; only a device's first
// calls serialise on g_dev_mutex (a thread-per-GPU host never contends after
// its device's first call).
struct DevInfo {
    std::atomic<bool> ready{false};
    int cus = 256;
};
std::mutex g_dev_mutex;
DevInfo g_dev[kMaxDev];

// Current device, checked, with tables uploaded and geometry known.
int device_ready(DevInfo **out)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e);
    if (dev < 0 || dev >= kMaxDev) return hip_err(hipErrorInvalidDevice);
    DevInfo &d = g_dev[dev];
    if (!d.ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lk(g_dev_mutex);
        if (!d.ready.load(std::memory_order_relaxed)) {
            hipDeviceProp_t prop;
            if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return hip_err(e);
            d.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            if ((e = upload_device_tables(&cpu_tables(0))) != hipSuccess) return hip_err(e);
            d.ready.store(true, std::memory_order_release);
        }
    }
    *out = &d;
    return NTT_OK;
}

// Launch shapes, all by the one rule of launch_shape.hpp.  The n <= 2048 batch
// kernels: one workgroup per `ppw * waves` consecutive work units (a unit is
// one n = 2048 polynomial or two n = 1024 polynomials); ppw grows with the
// batch (amortising the 16 KiB LDS-table prologue) but never beyond what keeps
// >= NTT_MIN_WG_PER_CU workgroups per CU in flight.
#ifndef NTT_MIN_WG_PER_CU
#define NTT_MIN_WG_PER_CU 4   // ppw 4 instead of 8 at 65 536 n=1024 polys: 3-4 % faster (profiles/r02/s4/ab_launch_ppw_p1_65536.log); 2^20 keeps ppw 16
#endif
#ifndef NTT_PPW_MAX
#define NTT_PPW_MAX 16
#endif
template <int PS>
LaunchShape batch_shape(size_t npoly, int waves, const DevInfo &d, size_t ppw_max = NTT_PPW_MAX)
{
    const size_t units = ceil_div(npoly, PSel<PS>::T::LOGN == 11 ? 1 : 2);
    return launch_shape(units, waves, d.cus, NTT_MIN_WG_PER_CU, ppw_max);
}
// n = 4096 / 8192: `per_wg` polynomials per workgroup step, >= 2 workgroups per CU
LaunchShape large_shape(size_t npoly, int per_wg, const DevInfo &d)
{
    return launch_shape(npoly, per_wg, d.cus, 2, NTT_PPW_MAX);
}

// A runtime choice as a template argument: f(std::bool_constant<v>{})
template <class F> void with_flag(bool v, F &&f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

int check_common(int ps, const void *p, size_t batch)
{
    if (!param_set(ps)) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!p) return NTT_ERR_NULL;
    if (((uintptr_t)p) & 3u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    return NTT_OK;
}

bool partial_overlap(const void *x, const void *y, size_t bytes)
{
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    if (a == b) return false;
    return a < b + bytes && b < a + bytes;
}

bool ranges_overlap(const void *x, size_t xbytes, const void *y, size_t ybytes)
{
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + ybytes && b < a + xbytes;
}

// The operands (a, b, c) of poly_mul / poly_mul_ntt / poly_pointwise /
// poly_mul_nussbaumer, each checked in turn (a's NULL, alignment and size
// before anything of b), then the alignment `mask` the kernel needs beyond a
// word and c against a and b (equal is in place, a partial overlap is not).
// An empty batch is NTT_OK: the caller returns on `rc != NTT_OK || batch == 0`.
int check_abc(int ps, const uint32_t *a, const uint32_t *b, const uint32_t *c, size_t batch, uintptr_t mask = 3u)
{
    int rc;
    if ((rc = check_common(ps, a, batch)) != NTT_OK || batch == 0) return rc;
    if ((rc = check_common(ps, b, batch)) != NTT_OK) return rc;
    if ((rc = check_common(ps, c, batch)) != NTT_OK) return rc;
    if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & mask) return NTT_ERR_ALIGN;
    const size_t bytes = batch * param_set(ps)->n * 4;
    if (partial_overlap(a, c, bytes) || partial_overlap(b, c, bytes)) return NTT_ERR_ALIAS;
    return NTT_OK;
}

// The inputs (y_0 .. y_{l-1}, ahat, add) of poly_mul_ntt_k / _kl / _kl_round:
// l batches of polynomials, the k x l shared rows and the optional addend.
// The keyed entry points add key (NULL or [batch] indices) and nkeys, the
// number of [k][l][n] blocks in ahat (1 in the unkeyed ones).
struct RowOps {
    const uint32_t *const *y;
    int l;
    const uint32_t *ahat, *add;
    const uint32_t *key = nullptr;
    size_t nkeys = 1;
    bool null() const
    {
        if (!y || !ahat) return true;
        for (int j = 0; j < l; j++)
            if (!y[j]) return true;
        return false;
    }
    uintptr_t bits() const   // every address ORed, for the alignment test; after null()
    {
        uintptr_t b = ((uintptr_t)ahat) | ((uintptr_t)add) | ((uintptr_t)key);
        for (int j = 0; j < l; j++) b |= (uintptr_t)y[j];
        return b;
    }
    bool too_large(size_t batch) const { return batch > (size_t)0x7FFFFFFF || nkeys > (size_t)NTT_MUL_KEYS_MAX; }
    // [x, x + bytes) against every y_j, all of ahat and the batch's key indices
    // (the addend has its own rule per entry point)
    bool overlap(const void *x, size_t bytes, size_t batch, int k, size_t row) const
    {
        for (int j = 0; j < l; j++)
            if (ranges_overlap(x, bytes, y[j], batch * row)) return true;
        if (key && ranges_overlap(x, bytes, key, batch * 4)) return true;
        return ranges_overlap(x, bytes, ahat, nkeys * k * l * row);
    }
};
// their parameter set (n = 1024 / 2048, the sets qTESLA defines), k, l and the
// number of keys; NULL: NTT_ERR_PARAM
const ParamSet *row_param_set(int ps, int k, int l, size_t nkeys = 1)
{
    const ParamSet *p = param_set(ps);
    return p && p->n <= 2048 && k >= 1 && k <= NTT_MUL_K_MAX && l >= 1 && l <= NTT_MUL_L_MAX && nkeys >= 1 ? p : nullptr;
}
// poly_mul_ntt_k / _kl / _kl_keyed: PARAM, empty batch (NTT_OK, as check_abc), NULL, ALIGN, SIZE, ALIAS
int check_mul_kl(const uint32_t *out, const RowOps &o, size_t batch, int k, int ps)
{
    const ParamSet *p = row_param_set(ps, k, o.l, o.nkeys);
    if (!p) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!out || o.null()) return NTT_ERR_NULL;
    if ((((uintptr_t)out) | o.bits()) & 3u) return NTT_ERR_ALIGN;
    if (o.too_large(batch)) return NTT_ERR_SIZE;
    const size_t row = (size_t)p->n * 4, obytes = batch * k * row;
    if (o.overlap(out, obytes, batch, k, row)) return NTT_ERR_ALIAS;
    if (o.add && partial_overlap(o.add, out, obytes)) return NTT_ERR_ALIAS;
    return NTT_OK;
}

int finish_launch()
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_err(e);
    return NTT_OK;
}

// Launcher<ps>::run(args...) for 0 <= ps < NSETS, NTT_ERR_PARAM otherwise
template <template <int> class Launcher, int NSETS, int PS = 0, class... Args>
int dispatch(int ps, Args &...args)
{
    if constexpr (PS < NSETS) return ps == PS ? Launcher<PS>::run(args...) : dispatch<Launcher, NSETS, PS + 1>(ps, args...);
    else return NTT_ERR_PARAM;
}
// ... on the current device, made ready first and passed as run's last
// argument.  NSETS = LARGE_PS0: the entry points that exist for n <= 2048 only
// (poly_mul_ntt_k and its kin).
template <template <int> class Launcher, int NSETS = NPARAM_SETS, class... Args>
int launch(int ps, Args &&...args)
{
    DevInfo *d = nullptr;
    const int rc = device_ready(&d);
    return rc != NTT_OK ? rc : dispatch<Launcher, NSETS>(ps, args..., *d);
}

// transform kind: forward / inverse with natural or bit-reversed NTT-domain
// order, or the plain bit-reversal permutation
enum Xform { FWD, INV, FWD_BR, INV_BR, BITREV };
static_assert((int)FWD == (int)LAT_FWD && (int)INV == (int)LAT_INV && (int)FWD_BR == (int)LAT_FWD_BR &&
                  (int)INV_BR == (int)LAT_INV_BR,
              "switch table order");
static_assert(MULK_K_MAX == NTT_MUL_K_MAX, "ABI row limit");
static_assert(ROWS_M_MAX == NTT_ROWS_M_MAX, "ABI column limit of ntt_rows_over");
static_assert(XOF_RATE128 * 8 == 168 && XOF_RATE256 * 8 == 136 && NTT_XOF_OUT_MAX % 8 == 0, "ABI rates and output limit");
static_assert(NTT_CHALLENGE_BLOCKS_MAX * CHALLENGE_DRAWS >= 8 * NTT_CHALLENGE_H_MAX, "block bound far above h / (7/8) draws");
static_assert(MULKL_L_MAX == NTT_MUL_L_MAX && NTT_MUL_L_MAX == 2, "ABI column limit (poly_mul_ntt_kl launches l = 2)");
static_assert(LAT_FWD == NTT_OP_FWD && LAT_INV == NTT_OP_INV && LAT_FWD_BR == NTT_OP_FWD_BR &&
                  LAT_INV_BR == NTT_OP_INV_BR && LAT_MUL == NTT_OP_MUL && LAT_MUL_NTT == NTT_OP_MUL_NTT &&
                  LAT_FWD_OOP == NTT_OP_FWD_OOP && LAT_INV_OOP == NTT_OP_INV_OOP,
              "ABI op codes");
// the four transforms as template arguments: f(inverse, bit-reversed order)
template <class F> void with_xform(Xform k, F &&f)
{
    switch (k) {
    case FWD: f(std::false_type{}, std::false_type{}); break;
    case INV: f(std::true_type{}, std::false_type{}); break;
    case FWD_BR: f(std::false_type{}, std::true_type{}); break;
    case INV_BR: f(std::true_type{}, std::true_type{}); break;
    case BITREV: break;   // a kernel of its own, where there is one
    }
}

template <int PS> struct LXform {
    template <int RB>
    static void launch_latr(Xform k, const uint32_t *in, uint32_t *out, size_t batch, hipStream_t s)
    {
        with_xform(k, [&](auto inv, auto br) {
            hipLaunchKernelGGL((k_ntt_latr<PS, decltype(inv)::value, decltype(br)::value, RB>), dim3((uint32_t)batch),
                               dim3(LatRGeo<PSel<PS>::T::LOGN, RB>::T), 0, s, in, out);
        });
    }
    static int run(Xform k, const uint32_t *in, uint32_t *out, size_t batch, hipStream_t s, const DevInfo &d)
    {
        // FWD / INV: in place or out of place (LAT_FWD_OOP / LAT_INV_OOP)
        const int sop = (k == FWD || k == INV) && in != out ? (k == FWD ? LAT_FWD_OOP : LAT_INV_OOP) : (int)k;
        const int rb = k == BITREV ? 0 : lat_radix(PS, sop, batch);
        const uint32_t nb = (uint32_t)batch;
        if (rb == 2) {
            // small batches: radix-4 passes, one polynomial per n/4-thread workgroup (ntt_lat.hpp)
            with_xform(k, [&](auto inv, auto br) {
                hipLaunchKernelGGL((k_ntt_lat<PS, decltype(inv)::value, decltype(br)::value>), dim3(nb),
                                   dim3(LatGeo<PSel<PS>::T::LOGN>::T), 0, s, in, out);
            });
        } else if (rb == 3) {
            launch_latr<3>(k, in, out, batch, s);   // radix-8 passes, n/8 threads (ntt_latr.hpp)
        } else if (rb == 4) {
            launch_latr<4>(k, in, out, batch, s);   // radix-16 passes, n/16 threads
        } else if constexpr (PS >= LARGE_PS0) {
            // n = 4096 / 8192: one wave per polynomial (ntt_big.hpp); the
            // bit-reversed orders are one launch too (an extra LDS transpose per chunk)
            const LaunchShape l = large_shape(batch, Big<PS>::WAVES, d);
            const dim3 g(l.grid), b(Big<PS>::NT);
            with_xform(k, [&](auto inv, auto br) {
                constexpr bool BR = decltype(br)::value;
                if constexpr (decltype(inv)::value) hipLaunchKernelGGL((k_ntt_inv_big<PS, BR>), g, b, 0, s, in, out, nb, l.chunk);
                else hipLaunchKernelGGL((k_ntt_fwd_big<PS, BR>), g, b, 0, s, in, out, nb, l.chunk);
            });
            if (k == BITREV)
                hipLaunchKernelGGL(k_bitrev_large<PS>, dim3(capped_grid(batch, 1, d.cus, 64)), dim3(512), 0, s, in, out, nb);
        } else {
            const LaunchShape l = batch_shape<PS>(batch, NTT_WG / 64, d);
            const dim3 g(l.grid), b(NTT_WG);
            with_xform(k, [&](auto inv, auto br) {
                constexpr bool BR = decltype(br)::value;
                if constexpr (decltype(inv)::value) hipLaunchKernelGGL((k_ntt_inv<PS, BR>), g, b, 0, s, in, out, nb, l.chunk);
                else hipLaunchKernelGGL((k_ntt_fwd<PS, BR>), g, b, 0, s, in, out, nb, l.chunk);
            });
            if (k == BITREV) hipLaunchKernelGGL(k_bitrev<PS>, g, b, 0, s, in, out, nb, l.chunk);
        }
        return finish_launch();
    }
};
template <int PS> struct LMul {
    static int run(const uint32_t *a, const uint32_t *b, uint32_t *c, size_t batch, hipStream_t s, bool bhat,
                   const DevInfo &d)
    {
        constexpr int N = PSel<PS>::T::N;
        const uint32_t nb = (uint32_t)batch;
        if constexpr (N <= 4096) {
            if (batch <= lat_max_batch(PS, bhat ? LAT_MUL_NTT : LAT_MUL)) {
                // small batches: one product per workgroup (ntt_lat.hpp)
                with_flag(bhat, [&](auto bh) {
                    hipLaunchKernelGGL((k_poly_mul_lat<PS, decltype(bh)::value>), dim3(nb), dim3(LatGeo<PSel<PS>::T::LOGN>::T),
                                       0, s, a, b, c);
                });
                return finish_launch();
            }
        }
        with_flag(bhat, [&](auto bh) {
            constexpr bool BHAT = decltype(bh)::value;
            if constexpr (PS >= LARGE_PS0 && N == 4096) {
                // one wave per product (ntt_big.hpp)
                constexpr int waves = big_mul_waves<BHAT>();
                const LaunchShape l = large_shape(batch, waves, d);
                hipLaunchKernelGGL((k_poly_mul_big<PS, BHAT>), dim3(l.grid), dim3(waves * 64), 0, s, a, b, c, nb, l.chunk);
            } else if constexpr (PS >= LARGE_PS0) {
                using LG = LargeMul<PS, BHAT>;
                const LaunchShape l = large_shape(batch, LG::SLOTS, d);
                hipLaunchKernelGGL((k_poly_mul_large<PS, BHAT>), dim3(l.grid), dim3(LG::NT), 0, s, a, b, c, nb, l.chunk);
            } else {
                constexpr int wg = mul_wg<BHAT>();
                const LaunchShape l = batch_shape<PS>(batch, wg / 64, d);
                hipLaunchKernelGGL((k_poly_mul<PS, BHAT>), dim3(l.grid), dim3(wg), 0, s, a, b, c, nb, l.chunk);
            }
        });
        return finish_launch();
    }
};
template <int PS> struct LPw {
    static int run(const uint32_t *a, const uint32_t *b, uint32_t *c, size_t count4, hipStream_t s, const DevInfo &d)
    {
        hipLaunchKernelGGL(k_pointwise<PS>, dim3(capped_grid(count4, WG, d.cus, 8)), dim3(WG), 0, s, (const uint4 *)a,
                           (const uint4 *)b, (uint4 *)c, count4);
        return finish_launch();
    }
};

// poly_mul_ntt_k and its kin: the batch kernels' launch shape
// with the kernel's own waves and chunk maximum; up to its measured switch
// batch `split_max` the k rows are spread over gridDim.y
struct RowShape {
    dim3 grid;
    uint32_t ppw;
};
template <int PS>
RowShape row_shape(size_t batch, int k, int waves, size_t ppw_max, size_t split_max, const DevInfo &d)
{
    const LaunchShape l = batch_shape<PS>(batch, waves, d, ppw_max);
    return {dim3(l.grid, batch <= split_max ? (uint32_t)k : 1u), l.chunk};
}

// poly_mul_ntt_k (ntt_mulk.hpp)
template <int PS> struct LMulK {
    static int run(const uint32_t *y, const uint32_t *ahat, const uint32_t *add, uint32_t *out, size_t batch, int k,
                   hipStream_t s, const DevInfo &d)
    {
        const RowShape r = row_shape<PS>(batch, k, MULK_WAVES, MULK_PPW_MAX, mulk_split_max(PS), d);
        with_flag(add != nullptr, [&](auto ad) {
            hipLaunchKernelGGL((k_poly_mul_k<PS, decltype(ad)::value>), r.grid, dim3(MULK_WG), 0, s, y, ahat, add, out,
                               (uint32_t)batch, (uint32_t)k, r.ppw);
        });
        return finish_launch();
    }
};

// poly_mul_ntt_kl, l = 2 (ntt_mulkl.hpp): that kernel's workgroup and its own
// measured switch batch
template <int PS> struct LMulKL {
    static int run(const uint32_t *const *y, const uint32_t *ahat, const uint32_t *add, uint32_t *out, size_t batch, int k,
                   hipStream_t s, const DevInfo &d)
    {
        const RowShape r = row_shape<PS>(batch, k, MULKL_WAVES, MULKL_PPW_MAX, mulkl_split_max(PS), d);
        const MulKLIn<2> in = {{y[0], y[1]}};
        with_flag(add != nullptr, [&](auto ad) {
            hipLaunchKernelGGL((k_poly_mul_kl<PS, 2, decltype(ad)::value>), r.grid, dim3(MULKL_WG), 0, s, in, ahat, add, out,
                               (uint32_t)batch, (uint32_t)k, r.ppw);
        });
        return finish_launch();
    }
};

// poly_mul_ntt_kl_round (ntt_mulkl.hpp): LMulKL's launch shape -- workgroup,
// chunk length and split threshold are poly_mul_ntt_kl's at l = 2, not swept
// again -- for l = 2 and for l = 1, which runs the same kernel with one y
template <int PS> struct LMulKLRound {
    template <int L>
    static void launch(const MulKLIn<L> &in, const uint32_t *ahat, const uint32_t *add, const RoundOut &ro, size_t batch,
                       int k, hipStream_t s, const RowShape &r)
    {
        with_flag(add != nullptr, [&](auto ad) {
            hipLaunchKernelGGL((k_poly_mul_kl_round<PS, L, decltype(ad)::value>), r.grid, dim3(MULKL_WG), 0, s, in, ahat, add, ro,
                               (uint32_t)batch, (uint32_t)k, r.ppw);
        });
    }
    static int run(const uint32_t *const *y, int l, const uint32_t *ahat, const uint32_t *add, const RoundOut &ro, size_t batch,
                   int k, hipStream_t s, const DevInfo &d)
    {
        const RowShape r = row_shape<PS>(batch, k, MULKL_WAVES, MULKL_PPW_MAX, mulkl_split_max(PS), d);
        if (l == 1) launch<1>(MulKLIn<1>{{y[0]}}, ahat, add, ro, batch, k, s, r);
        else launch<2>(MulKLIn<2>{{y[0], y[1]}}, ahat, add, ro, batch, k, s, r);
        return finish_launch();
    }
};

// poly_mul_ntt_kl_keyed (ro NULL) and poly_mul_ntt_kl_round_keyed (out NULL):
// the keyed kernels of ntt_mulkl.hpp, in LMulKLRound's launch shape -- the
// split threshold is poly_mul_ntt_kl's at l = 2, not swept again -- for both l
template <int PS> struct LMulKLKeyed {
    template <int L>
    static void launch(const MulKLIn<L> &in, const uint32_t *ahat, const KeySel &ks, const uint32_t *add, uint32_t *out,
                       const RoundOut *ro, size_t batch, int k, hipStream_t s, const RowShape &r)
    {
        with_flag(add != nullptr, [&](auto ad) {
            constexpr bool ADD = decltype(ad)::value;
            if (ro)
                hipLaunchKernelGGL((k_poly_mul_kl_round_keyed<PS, L, ADD>), r.grid, dim3(MULKL_WG), 0, s, in, ahat, ks, add, *ro,
                                   (uint32_t)batch, (uint32_t)k, r.ppw);
            else
                hipLaunchKernelGGL((k_poly_mul_kl_keyed<PS, L, ADD>), r.grid, dim3(MULKL_WG), 0, s, in, ahat, ks, add, out,
                                   (uint32_t)batch, (uint32_t)k, r.ppw);
        });
    }
    static int run(const RowOps &o, uint32_t *out, const RoundOut *ro, size_t batch, int k, hipStream_t s, const DevInfo &d)
    {
        const RowShape r = row_shape<PS>(batch, k, MULKL_WAVES, MULKL_PPW_MAX, mulkl_split_max(PS), d);
        const KeySel ks = {o.key, (uint32_t)(o.nkeys - 1)};
        if (o.l == 1) launch<1>(MulKLIn<1>{{o.y[0]}}, o.ahat, ks, o.add, out, ro, batch, k, s, r);
        else launch<2>(MulKLIn<2>{{o.y[0], o.y[1]}}, o.ahat, ks, o.add, out, ro, batch, k, s, r);
        return finish_launch();
    }
};

// poly_round (ntt_round.hpp): a workgroup per tile of RoundGeom's WAVES
// kilo-coefficients, up to ROUND_TILES_MAX consecutive tiles each once there
// are 8 workgroups per CU
template <int PS> struct LRound {
    template <bool HI, bool NORMS>
    static void launch(const uint32_t *w, uint8_t *hi, uint32_t *norms, size_t nwaves, int dbits, hipStream_t s, const DevInfo &d)
    {
        using G = RoundGeom<PS>;
        const LaunchShape l = launch_shape(ceil_div(nwaves, G::WAVES), 1, d.cus, 8, ROUND_TILES_MAX);
        hipLaunchKernelGGL((k_poly_round<PS, HI, NORMS>), dim3(l.grid), dim3(G::WG), 0, s, w, (uint32_t *)hi, (uint2 *)norms,
                           nwaves, (uint32_t)dbits, l.chunk);
    }
    static int run(const uint32_t *w, uint8_t *hi, uint32_t *norms, size_t batch, int dbits, hipStream_t s, const DevInfo &d)
    {
        const size_t nwaves = batch * RoundGeom<PS>::WPP;
        if (hi && norms) launch<true, true>(w, hi, norms, nwaves, dbits, s, d);
        else if (hi) launch<true, false>(w, hi, norms, nwaves, dbits, s, d);
        else launch<false, true>(w, hi, norms, nwaves, dbits, s, d);
        return finish_launch();
    }
};

// poly_pack / poly_unpack (ntt_pack.hpp): poly_round's launch shape, a wave per
// 1024 coefficients; the kernels are shared by the sets of equal n
template <int PS> struct LPack {
    static int run(uint32_t *bytes, uint32_t *w, uint32_t *mx, bool unpack, const PackRows &R, size_t npoly, hipStream_t s,
                   const DevInfo &d)
    {
        constexpr int WPP = RoundGeom<PS>::WPP;
        using G = PackGeom<WPP>;
        const size_t nwaves = npoly * WPP;
        const LaunchShape l = launch_shape(ceil_div(nwaves, G::WAVES), 1, d.cus, 8, ROUND_TILES_MAX);
        const dim3 grid(l.grid), wg(G::WG);
        if (!unpack) hipLaunchKernelGGL((k_poly_pack<WPP>), grid, wg, 0, s, bytes, (const uint32_t *)w, R, nwaves, l.chunk);
        else if (mx) hipLaunchKernelGGL((k_poly_unpack<WPP, true>), grid, wg, 0, s, w, mx, (const uint32_t *)bytes, R, nwaves, l.chunk);
        else hipLaunchKernelGGL((k_poly_unpack<WPP, false>), grid, wg, 0, s, w, mx, (const uint32_t *)bytes, R, nwaves, l.chunk);
        return finish_launch();
    }
};

// The checks of poly_pack / poly_unpack in the header's order, then the launch.
// bytes: the packed rows; w: the coefficients; mx: poly_unpack's maxima or NULL.
int pack_common(const void *bytes, const void *w, const void *mx, bool unpack, size_t stride, size_t batch, int k, int bits,
                int sgn, int ps, void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p || k < 1 || k > NTT_MUL_K_MAX || (sgn != 0 && sgn != 1)) return NTT_ERR_PARAM;
    int qbits = 0;
    while (p->q >> qbits) ++qbits;
    if (bits < 8 || bits > qbits - sgn) return NTT_ERR_PARAM;
    const size_t packed = (size_t)k * p->n * (size_t)bits / 8;
    if ((stride & 15u) || stride < packed) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!bytes || !w) return NTT_ERR_NULL;
    if (((((uintptr_t)bytes) | ((uintptr_t)w)) & 15u) || (((uintptr_t)mx) & 3u)) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF / (size_t)k) return NTT_ERR_SIZE;
    const size_t bbytes = (batch - 1) * stride + packed, wbytes = batch * k * p->n * 4, mbytes = batch * k * 4;
    if (ranges_overlap(bytes, bbytes, w, wbytes)) return NTT_ERR_ALIAS;
    if (mx && (ranges_overlap(mx, mbytes, bytes, bbytes) || ranges_overlap(mx, mbytes, w, wbytes))) return NTT_ERR_ALIAS;
    const PackRows R = {stride, (uint32_t)k, (uint32_t)bits, sgn ? 1u << (bits - 1) : 0u, p->q,
                        (uint32_t)(((uint64_t)1 << 32) / (uint32_t)bits) + 1u};
    return launch<LPack>(ps, (uint32_t *)bytes, (uint32_t *)w, (uint32_t *)mx, unpack, R, batch * k, (hipStream_t)stream);
}

// poly_unpack_ntt (ntt_unpack_ntt.hpp): k_ntt_fwd's workgroup and launch shape, one kernel for every batch
template <int PS> struct LUnpackNtt {
    static int run(uint32_t *out, size_t pstride, uint32_t *mx, const uint32_t *bytes, const PackRows &R, bool neg, size_t npoly,
                   hipStream_t s, const DevInfo &d)
    {
        const LaunchShape l = batch_shape<PS>(npoly, NTT_WG / 64, d);
        with_flag(mx != nullptr, [&](auto m) {
            hipLaunchKernelGGL((k_unpack_ntt<PS, decltype(m)::value>), dim3(l.grid), dim3(NTT_WG), 0, s, out, pstride, mx, bytes, R,
                               neg ? 1u : 0u, (uint32_t)npoly, l.chunk);
        });
        return finish_launch();
    }
};

// largest hi of poly_round: it fits a signed byte iff this is <= 127
uint32_t round_hmax(uint32_t q, int d) { return ((q - 1) / 2 + (1u << (d - 1)) - 1) >> d; }

// poly_round's checks of d and its two outputs (hbytes / nbytes: their sizes);
// the caller has checked the parameter set and batch > 0
int check_round_out(const ParamSet *p, const uint8_t *d_hi, const uint32_t *d_norms, int d, size_t hbytes, size_t nbytes)
{
    if (!d_hi && !d_norms) return NTT_ERR_NULL;
    if (d_hi && round_hmax(p->q, d) > 127) return NTT_ERR_PARAM;
    if ((((uintptr_t)d_hi) & 15u) || (((uintptr_t)d_norms) & 7u)) return NTT_ERR_ALIGN;
    if (d_hi && d_norms && ranges_overlap(d_hi, hbytes, d_norms, nbytes)) return NTT_ERR_ALIAS;
    return NTT_OK;
}

int transform(Xform k, uint32_t *out, const uint32_t *in, size_t batch, int ps, void *stream)
{
    int rc = check_common(ps, in, batch);
    if (rc == NTT_OK && batch) rc = check_common(ps, out, batch);
    if (rc != NTT_OK || batch == 0) return rc;
    if (partial_overlap(in, out, batch * param_set(ps)->n * 4)) return NTT_ERR_ALIAS;
    return launch<LXform>(ps, k, in, out, batch, (hipStream_t)stream);
}

int mul_common(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b, size_t batch, int ps, void *stream,
               bool bhat)
{
    int rc = check_abc(ps, d_a, d_b, d_c, batch);
    if (rc != NTT_OK || batch == 0) return rc;
    return launch<LMul>(ps, d_a, d_b, d_c, batch, (hipStream_t)stream, bhat);
}

// poly_mul_ntt_kl_round and its keyed form: the checks, then the launch
int mul_kl_round_common(uint8_t *d_hi, uint32_t *d_norms, const RowOps &in, bool keyed, size_t batch, int k, int d,
                        int ps, void *stream)
{
    // poly_round's order, not poly_mul_ntt_kl's: the inputs' alignment after the outputs' checks
    const ParamSet *p = row_param_set(ps, k, in.l, in.nkeys);
    if (!p || d < 1 || d > 30) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (in.null()) return NTT_ERR_NULL;
    if (in.too_large(batch)) return NTT_ERR_SIZE;
    const size_t row = (size_t)p->n * 4, hbytes = batch * k * p->n, nbytes = batch * k * 8;
    int rc;
    if ((rc = check_round_out(p, d_hi, d_norms, d, hbytes, nbytes)) != NTT_OK) return rc;
    if (in.bits() & 3u) return NTT_ERR_ALIGN;
    // neither output overlaps any input (the addend included: nothing is accumulated in place)
    const void *outs[2] = {d_hi, d_norms};
    const size_t obytes[2] = {hbytes, nbytes};
    for (int o = 0; o < 2; o++) {
        if (!outs[o]) continue;
        if (in.overlap(outs[o], obytes[o], batch, k, row)) return NTT_ERR_ALIAS;
        if (in.add && ranges_overlap(outs[o], obytes[o], in.add, batch * k * row)) return NTT_ERR_ALIAS;
    }
    const RoundOut ro = {d_hi, (uint2 *)d_norms, (uint32_t)d};
    if (keyed) {
        uint32_t *const no_out = nullptr;
        const RoundOut *const pro = &ro;
        return launch<LMulKLKeyed, LARGE_PS0>(ps, in, no_out, pro, batch, k, (hipStream_t)stream);
    }
    return launch<LMulKLRound, LARGE_PS0>(ps, in.y, in.l, in.ahat, in.add, ro, batch, k, (hipStream_t)stream);
}

// k_sample_gauss<R, C> for the run-time rate and 1 <= cols <= NTT_GAUSS_COLS_MAX
template <int R, int C = 1, class... Args> void launch_gauss(int cols, dim3 grid, hipStream_t s, Args... args)
{
    if constexpr (C <= NTT_GAUSS_COLS_MAX) {
        if (cols == C) hipLaunchKernelGGL((k_sample_gauss<R, C>), grid, dim3(GAUSS_WG), 0, s, args...);
        else launch_gauss<R, C + 1>(cols, grid, s, args...);
    }
}

// poly_hsum (ntt_gauss.hpp): a wave per polynomial, HSUM_WAVES of them a workgroup
template <int PS> struct LHsum {
    static int run(uint64_t *sum, const uint32_t *w, size_t batch, int h, hipStream_t s, const DevInfo &)
    {
        hipLaunchKernelGGL(k_hsum<PS>, dim3((uint32_t)ceil_div(batch, (size_t)HSUM_WAVES)), dim3(HSUM_WAVES * 64), 0, s, sum, w,
                           (uint32_t)batch, (uint32_t)h);
        return finish_launch();
    }
};

// ntt_rows_over / _differ / ntt_select / ntt_rows_move (ntt_rows.hpp): bytes of `rows` rows of `row_bytes` at `stride`
size_t rows_extent(size_t rows, size_t stride, size_t row_bytes) { return rows ? (rows - 1) * stride + row_bytes : 0; }

// log2 of the lanes that share a row of `units` loads: the smallest power of two that covers them, at most 2^max_log
uint32_t row_lanes_log(size_t units, uint32_t max_log)
{
    uint32_t l = 0;
    while (l < max_log && ((size_t)1 << l) < units) ++l;
    return l;
}

// the three grid kernels of ntt_rows.hpp stride over their rows: one workgroup per `per_wg` rows, at most 16 per CU
dim3 rows_grid(size_t rows, size_t per_wg, const DevInfo &d) { return dim3(capped_grid(rows, per_wg, d.cus, 16)); }

}  // namespace

void set_last_hip(int e) { t_last_hip = e; }

}  // namespace qntt

// ==========================================================================
// C ABI (include/qtesla_ntt.h)
// ==========================================================================
using namespace qntt;

extern "C" {

int ntt_param_info(int ps, uint32_t *n, uint32_t *q, uint32_t *psi, uint32_t *omega,
                   uint32_t *omega_inv, uint32_t *n_inv)
{
    const ParamSet *p = param_set(ps);
    if (!p) return NTT_ERR_PARAM;
    const Tables &t = cpu_tables(ps);
    if (n) *n = p->n;
    if (q) *q = p->q;
    if (psi) *psi = p->psi;
    if (omega) *omega = t.omega;
    if (omega_inv) *omega_inv = t.omega_inv;
    if (n_inv) *n_inv = t.n_inv;
    return NTT_OK;
}

int ntt_get_tables(int ps, uint32_t *bitrev_tbl, uint32_t *Phi, uint32_t *invPhi, uint32_t *tf0, uint32_t *ti0)
{
    const ParamSet *p = param_set(ps);
    if (!p) return NTT_ERR_PARAM;
    const Tables &t = cpu_tables(ps);
    const size_t b = (size_t)p->n * 4;
    if (bitrev_tbl) memcpy(bitrev_tbl, t.bitrev_tbl.data(), b);
    if (Phi) memcpy(Phi, t.Phi.data(), b);
    if (invPhi) memcpy(invPhi, t.invPhi.data(), b);
    if (tf0) memcpy(tf0, t.tf0.data(), b);
    if (ti0) memcpy(ti0, t.ti0.data(), b);
    return NTT_OK;
}

int poly_ntt(uint32_t *d_poly, const uint32_t *twiddleFactor, size_t batch, int ps, void *stream)
{
    (void)twiddleFactor;  // dead parameter, as in the reference kernels
    return transform(FWD, d_poly, d_poly, batch, ps, stream);
}

int poly_invntt(uint32_t *d_poly, const uint32_t *twiddleFactor, size_t batch, int ps, void *stream)
{
    (void)twiddleFactor;
    return transform(INV, d_poly, d_poly, batch, ps, stream);
}

int poly_ntt_oop(uint32_t *d_out, const uint32_t *d_in, size_t batch, int ps, void *stream)
{
    return transform(FWD, d_out, d_in, batch, ps, stream);
}

int poly_invntt_oop(uint32_t *d_out, const uint32_t *d_in, size_t batch, int ps, void *stream)
{
    return transform(INV, d_out, d_in, batch, ps, stream);
}

int poly_ntt_bitrev(uint32_t *d_out, const uint32_t *d_in, size_t batch, int ps, void *stream)
{
    return transform(FWD_BR, d_out, d_in, batch, ps, stream);
}

int poly_invntt_bitrev(uint32_t *d_out, const uint32_t *d_in, size_t batch, int ps, void *stream)
{
    return transform(INV_BR, d_out, d_in, batch, ps, stream);
}

int poly_bitrev_copy(uint32_t *d_out, const uint32_t *d_in, size_t batch, int ps, void *stream)
{
    return transform(BITREV, d_out, d_in, batch, ps, stream);
}

int poly_mul(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b, size_t batch, int ps, void *stream)
{
    return mul_common(d_c, d_a, d_b, batch, ps, stream, false);
}

int poly_mul_ntt(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_bhat, size_t batch, int ps, void *stream)
{
    return mul_common(d_c, d_a, d_bhat, batch, ps, stream, true);
}

int poly_mul_ntt_k(uint32_t *d_out, const uint32_t *d_y, const uint32_t *d_ahat, const uint32_t *d_add, size_t batch,
                   int k, int ps, void *stream)
{
    int rc = check_mul_kl(d_out, RowOps{&d_y, 1, d_ahat, d_add}, batch, k, ps);
    if (rc != NTT_OK || batch == 0) return rc;
    return launch<LMulK, LARGE_PS0>(ps, d_y, d_ahat, d_add, d_out, batch, k, (hipStream_t)stream);
}

int ntt_mul_k_shape(int ps, size_t *split_max_batch, int *waves_per_workgroup)
{
    const ParamSet *p = param_set(ps);
    if (!p || p->n > 2048) return NTT_ERR_PARAM;
    if (split_max_batch) *split_max_batch = mulk_split_max(ps);
    if (waves_per_workgroup) *waves_per_workgroup = MULK_WAVES;
    return NTT_OK;
}

int poly_mul_ntt_kl(uint32_t *d_out, const uint32_t *const *d_y, const uint32_t *d_ahat, const uint32_t *d_add,
                    size_t batch, int k, int l, int ps, void *stream)
{
    int rc = check_mul_kl(d_out, RowOps{d_y, l, d_ahat, d_add}, batch, k, ps);
    if (rc != NTT_OK || batch == 0) return rc;
    if (l == 1) return poly_mul_ntt_k(d_out, d_y[0], d_ahat, d_add, batch, k, ps, stream);
    return launch<LMulKL, LARGE_PS0>(ps, d_y, d_ahat, d_add, d_out, batch, k, (hipStream_t)stream);
}

int ntt_mul_kl_shape(int ps, int l, size_t *split_max_batch, int *waves_per_workgroup)
{
    if (l == 1) return ntt_mul_k_shape(ps, split_max_batch, waves_per_workgroup);
    const ParamSet *p = param_set(ps);
    if (!p || p->n > 2048 || l < 1 || l > NTT_MUL_L_MAX) return NTT_ERR_PARAM;
    if (split_max_batch) *split_max_batch = mulkl_split_max(ps);
    if (waves_per_workgroup) *waves_per_workgroup = MULKL_WAVES;
    return NTT_OK;
}

int poly_scatter(uint32_t *d_out, const uint32_t *d_pos, const uint32_t *d_val, size_t batch, int h, int ps, void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p || h < 1 || (uint32_t)h > p->n) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_out || !d_pos || !d_val) return NTT_ERR_NULL;
    if ((((uintptr_t)d_out) | ((uintptr_t)d_pos) | ((uintptr_t)d_val)) & 3u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t obytes = batch * p->n * 4, lbytes = batch * (size_t)h * 4;
    if (ranges_overlap(d_out, obytes, d_pos, lbytes) || ranges_overlap(d_out, obytes, d_val, lbytes)) return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    hipLaunchKernelGGL(k_poly_scatter, dim3((uint32_t)batch), dim3(SCATTER_WG), p->n * 4, (hipStream_t)stream, d_pos, d_val,
                       d_out, p->n, p->q, (uint32_t)h);
    return finish_launch();
}

int poly_round(uint8_t *d_hi, uint32_t *d_norms, const uint32_t *d_w, size_t batch, int d, int ps, void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p || d < 1 || d > 30) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_w) return NTT_ERR_NULL;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t wbytes = batch * p->n * 4, hbytes = batch * p->n, nbytes = batch * 8;
    int rc;
    if ((rc = check_round_out(p, d_hi, d_norms, d, hbytes, nbytes)) != NTT_OK) return rc;
    if (((uintptr_t)d_w) & 15u) return NTT_ERR_ALIGN;
    if ((d_hi && ranges_overlap(d_hi, hbytes, d_w, wbytes)) || (d_norms && ranges_overlap(d_norms, nbytes, d_w, wbytes)))
        return NTT_ERR_ALIAS;
    return launch<LRound>(ps, d_w, d_hi, d_norms, batch, d, (hipStream_t)stream);
}

int poly_mul_ntt_kl_round(uint8_t *d_hi, uint32_t *d_norms, const uint32_t *const *d_y, const uint32_t *d_ahat,
                          const uint32_t *d_add, size_t batch, int k, int l, int d, int ps, void *stream)
{
    return mul_kl_round_common(d_hi, d_norms, RowOps{d_y, l, d_ahat, d_add}, false, batch, k, d, ps, stream);
}

int poly_mul_ntt_kl_keyed(uint32_t *d_out, const uint32_t *const *d_y, const uint32_t *d_ahat, const uint32_t *d_key,
                          size_t nkeys, const uint32_t *d_add, size_t batch, int k, int l, int ps, void *stream)
{
    const RowOps in = {d_y, l, d_ahat, d_add, d_key, nkeys};
    int rc = check_mul_kl(d_out, in, batch, k, ps);
    if (rc != NTT_OK || batch == 0) return rc;
    const RoundOut *const no_ro = nullptr;
    return launch<LMulKLKeyed, LARGE_PS0>(ps, in, d_out, no_ro, batch, k, (hipStream_t)stream);
}

int poly_mul_ntt_kl_round_keyed(uint8_t *d_hi, uint32_t *d_norms, const uint32_t *const *d_y, const uint32_t *d_ahat,
                                const uint32_t *d_key, size_t nkeys, const uint32_t *d_add, size_t batch, int k, int l,
                                int d, int ps, void *stream)
{
    return mul_kl_round_common(d_hi, d_norms, RowOps{d_y, l, d_ahat, d_add, d_key, nkeys}, true, batch, k, d, ps, stream);
}

// Largest batch at which NTT_XOF_PATH_AUTO runs the wave kernels (two messages
// per wave, ntt_xof_wave.hpp), per [ragged][algo]: measured, DESIGN.md section 5q
static constexpr size_t kXofWaveMax[2][2] = {{8192, 8192}, {8192, 8192}};

static bool xof_takes_wave(int path, int ragged, int algo, size_t batch)
{
    return path == NTT_XOF_PATH_WAVE || (path == NTT_XOF_PATH_AUTO && batch <= kXofWaveMax[ragged][algo]);
}

// one workgroup per XOF_WAVE_WG / 64 waves, one wave per two messages, in rows of XOF_WAVE_GRID_X workgroups (a grid
// dimension holds fewer than 2^32 threads, batch = 2^31 - 1 needs 2^36)
static dim3 xof_wave_grid(size_t batch)
{
    const size_t wgs = ceil_div(ceil_div(batch, (size_t)2) * 64, (size_t)XOF_WAVE_WG);
    return dim3((uint32_t)(wgs < XOF_WAVE_GRID_X ? wgs : XOF_WAVE_GRID_X), (uint32_t)ceil_div(wgs, (size_t)XOF_WAVE_GRID_X));
}

int ntt_xof_path(uint8_t *d_out, size_t outlen, const uint8_t *d_in0, size_t len0, const uint8_t *d_in1, size_t len1,
                 size_t batch, int algo, int cstm, int path, void *stream)
{
    if (path < NTT_XOF_PATH_AUTO || path > NTT_XOF_PATH_WAVE) return NTT_ERR_PARAM;
    if ((algo != NTT_XOF_SHAKE128 && algo != NTT_XOF_SHAKE256) || cstm < -1 || cstm > 65535) return NTT_ERR_PARAM;
    if ((len0 & 7u) || (len1 & 7u) || len0 >= ((size_t)1 << 32) || len1 >= ((size_t)1 << 32) ||
        len0 + len1 >= ((size_t)1 << 32))
        return NTT_ERR_PARAM;
    if ((outlen & 7u) || outlen < 8 || outlen > NTT_XOF_OUT_MAX) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    // a segment of length 0 is never read: its pointer takes part in no check
    const uint8_t *in0 = len0 ? d_in0 : nullptr, *in1 = len1 ? d_in1 : nullptr;
    if (!d_out || (len0 && !in0) || (len1 && !in1)) return NTT_ERR_NULL;
    if ((((uintptr_t)d_out) | ((uintptr_t)in0) | ((uintptr_t)in1)) & 7u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t obytes = batch * outlen;
    if ((len0 && ranges_overlap(d_out, obytes, in0, batch * len0)) || (len1 && ranges_overlap(d_out, obytes, in1, batch * len1)))
        return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const bool wave = xof_takes_wave(path, 0, algo, batch);
    const dim3 grid = wave ? xof_wave_grid(batch) : dim3((uint32_t)ceil_div(batch, (size_t)XOF_WG));
    const dim3 wg(wave ? XOF_WAVE_WG : XOF_WG);
    const uint32_t ow = (uint32_t)(outlen / 8), w0 = (uint32_t)(len0 / 8), w1 = (uint32_t)(len1 / 8);
    auto *const k = algo == NTT_XOF_SHAKE128 ? (wave ? k_xof_wave<XOF_RATE128> : k_xof<XOF_RATE128>)
                                             : (wave ? k_xof_wave<XOF_RATE256> : k_xof<XOF_RATE256>);
    hipLaunchKernelGGL(k, grid, wg, 0, (hipStream_t)stream, (uint64_t *)d_out, ow, (const uint64_t *)in0, w0,
                       (const uint64_t *)in1, w1, (uint32_t)batch, cstm);
    return finish_launch();
}

int ntt_xof(uint8_t *d_out, size_t outlen, const uint8_t *d_in0, size_t len0, const uint8_t *d_in1, size_t len1,
            size_t batch, int algo, int cstm, void *stream)
{
    return ntt_xof_path(d_out, outlen, d_in0, len0, d_in1, len1, batch, algo, cstm, NTT_XOF_PATH_AUTO, stream);
}

int ntt_xof_ragged_path(uint8_t *d_out, size_t outlen, const uint8_t *d_msg, size_t msg_bytes, const uint64_t *d_off,
                        size_t batch, int algo, int cstm, int path, void *stream)
{
    if (path < NTT_XOF_PATH_AUTO || path > NTT_XOF_PATH_WAVE) return NTT_ERR_PARAM;
    if ((algo != NTT_XOF_SHAKE128 && algo != NTT_XOF_SHAKE256) || cstm < -1 || cstm > 65535) return NTT_ERR_PARAM;
    if ((outlen & 7u) || outlen < 8 || outlen > NTT_XOF_OUT_MAX || (msg_bytes & 7u)) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    // an empty buffer is never read: its pointer takes part in no check
    const uint8_t *msg = msg_bytes ? d_msg : nullptr;
    if (!d_out || !d_off || (msg_bytes && !msg)) return NTT_ERR_NULL;
    if ((((uintptr_t)d_out) | ((uintptr_t)d_off) | ((uintptr_t)msg)) & 7u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t obytes = batch * outlen;
    if ((msg_bytes && ranges_overlap(d_out, obytes, msg, msg_bytes)) || ranges_overlap(d_out, obytes, d_off, 8 * (batch + 1)))
        return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const bool wave = xof_takes_wave(path, 1, algo, batch);
    const dim3 grid = wave ? xof_wave_grid(batch) : dim3((uint32_t)ceil_div(batch, (size_t)XOF_WG));
    const dim3 wg(wave ? XOF_WAVE_WG : XOF_WG);
    const uint32_t ow = (uint32_t)(outlen / 8);
    auto *const k = algo == NTT_XOF_SHAKE128 ? (wave ? k_xof_ragged_wave<XOF_RATE128> : k_xof_ragged<XOF_RATE128>)
                                             : (wave ? k_xof_ragged_wave<XOF_RATE256> : k_xof_ragged<XOF_RATE256>);
    hipLaunchKernelGGL(k, grid, wg, 0, (hipStream_t)stream, (uint64_t *)d_out, ow, (const uint64_t *)msg, (uint64_t)msg_bytes,
                       d_off, (uint32_t)batch, cstm);
    return finish_launch();
}

int ntt_xof_ragged(uint8_t *d_out, size_t outlen, const uint8_t *d_msg, size_t msg_bytes, const uint64_t *d_off, size_t batch,
                   int algo, int cstm, void *stream)
{
    return ntt_xof_ragged_path(d_out, outlen, d_msg, msg_bytes, d_off, batch, algo, cstm, NTT_XOF_PATH_AUTO, stream);
}

int ntt_xof_small_batch_max(int algo, int ragged, size_t *max_batch)
{
    if ((algo != NTT_XOF_SHAKE128 && algo != NTT_XOF_SHAKE256) || ragged < 0 || ragged > 1) return NTT_ERR_PARAM;
    if (!max_batch) return NTT_ERR_NULL;
    *max_batch = kXofWaveMax[ragged][algo];
    return NTT_OK;
}

int poly_challenge(uint32_t *d_pos, uint32_t *d_val, const uint8_t *d_seed, size_t seedlen, size_t batch, int h, int ps,
                   void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p || h < 1 || h > NTT_CHALLENGE_H_MAX) return NTT_ERR_PARAM;
    if ((seedlen & 7u) || seedlen < 8 || seedlen > 160) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_pos || !d_val || !d_seed) return NTT_ERR_NULL;
    if ((((uintptr_t)d_pos) | ((uintptr_t)d_val) | ((uintptr_t)d_seed)) & 7u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t lbytes = batch * (size_t)h * 4, sbytes = batch * seedlen;
    if (ranges_overlap(d_pos, lbytes, d_val, lbytes) || ranges_overlap(d_pos, lbytes, d_seed, sbytes) ||
        ranges_overlap(d_val, lbytes, d_seed, sbytes))
        return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    hipLaunchKernelGGL(k_challenge, dim3((uint32_t)ceil_div(batch, (size_t)CHALLENGE_WG)), dim3(CHALLENGE_WG),
                       (size_t)p->n / 32 * CHALLENGE_WG * 4, (hipStream_t)stream, d_pos, d_val, (const uint64_t *)d_seed,
                       (uint32_t)(seedlen / 8), (uint32_t)batch, (uint32_t)h, p->n, p->q, (uint32_t)NTT_CHALLENGE_BLOCKS_MAX);
    return finish_launch();
}

int poly_sample_y(uint32_t *d_y, const uint8_t *d_seed, size_t seedlen, const uint32_t *d_nonce, uint32_t nonce, size_t batch,
                  int bits, int algo, int ps, void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p || (algo != NTT_XOF_SHAKE128 && algo != NTT_XOF_SHAKE256)) return NTT_ERR_PARAM;
    const size_t rate = algo == NTT_XOF_SHAKE128 ? 8 * XOF_RATE128 : 8 * XOF_RATE256;
    if (bits < 2 || bits > 24 || nonce > 255) return NTT_ERR_PARAM;
    if ((seedlen & 7u) || seedlen < 8 || seedlen > rate - 8) return NTT_ERR_PARAM;   // one absorb block
    if (batch == 0) return NTT_OK;
    if (!d_y || !d_seed) return NTT_ERR_NULL;
    if ((((uintptr_t)d_y) & 15u) || (((uintptr_t)d_seed) & 7u) || (((uintptr_t)d_nonce) & 3u)) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t ybytes = batch * p->n * 4;
    if (ranges_overlap(d_y, ybytes, d_seed, batch * seedlen) || (d_nonce && ranges_overlap(d_y, ybytes, d_nonce, batch * 4)))
        return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const dim3 grid((uint32_t)ceil_div(batch, (size_t)SAMPLE_WG)), wg(SAMPLE_WG);
    const uint32_t sw = (uint32_t)(seedlen / 8);
    if (algo == NTT_XOF_SHAKE128)
        hipLaunchKernelGGL(k_sample_y<XOF_RATE128>, grid, wg, 0, (hipStream_t)stream, d_y,
                           (const uint64_t *)d_seed, sw, d_nonce, nonce, (uint32_t)batch, p->n, p->q, (uint32_t)bits,
                           (uint32_t)NTT_SAMPLE_Y_REFILLS_MAX);
    else
        hipLaunchKernelGGL(k_sample_y<XOF_RATE256>, grid, wg, 0, (hipStream_t)stream, d_y,
                           (const uint64_t *)d_seed, sw, d_nonce, nonce, (uint32_t)batch, p->n, p->q, (uint32_t)bits,
                           (uint32_t)NTT_SAMPLE_Y_REFILLS_MAX);
    return finish_launch();
}

int poly_gen_a(uint32_t *d_a, size_t pstride, const uint8_t *d_seed, size_t seedlen, size_t batch, int k, int nblocks, int ps,
               void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p) return NTT_ERR_PARAM;
    uint32_t qbits = 0;
    while (qbits < 32 && (p->q >> qbits)) ++qbits;
    if (qbits <= 24) return NTT_ERR_PARAM;   // four-byte draws only: `ref` would need three
    if (k < 1 || k > NTT_MUL_K_MAX || nblocks < 1 || nblocks > NTT_GEN_A_BLOCKS_MAX) return NTT_ERR_PARAM;
    if ((seedlen & 7u) || seedlen < 8 || seedlen > 160) return NTT_ERR_PARAM;   // one absorb block
    if (pstride < p->n || (pstride & 3u)) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_a || !d_seed) return NTT_ERR_NULL;
    if ((((uintptr_t)d_a) & 15u) || (((uintptr_t)d_seed) & 7u)) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t abytes = ((batch * (size_t)k - 1) * pstride + p->n) * 4;
    if (ranges_overlap(d_a, abytes, d_seed, batch * seedlen)) return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const size_t kn = (size_t)k * p->n, refills = 4 * ceil_div(kn, (size_t)40);
    hipLaunchKernelGGL(k_gen_a, dim3((uint32_t)ceil_div(batch, (size_t)GEN_A_WG)), dim3(GEN_A_WG), 0, (hipStream_t)stream, d_a,
                       pstride, (const uint64_t *)d_seed, (uint32_t)(seedlen / 8), (uint32_t)batch, (uint32_t)k, p->logn, p->q,
                       (uint32_t)((1ull << qbits) - 1), (uint32_t)nblocks, (uint32_t)(refills < 65535 ? refills : 65535));
    return finish_launch();
}

int poly_sample_gauss(uint32_t *d_out, const uint8_t *d_seed, size_t seedlen, const uint32_t *d_nonce, uint32_t nonce,
                      const uint32_t *d_cdt, int rows, int cols, size_t batch, int algo, int ps, void *stream)
{
    static_assert(GAUSS_CHUNK == NTT_GAUSS_CHUNK, "the header's chunk");
    const ParamSet *p = param_set(ps);
    if (!p || (algo != NTT_XOF_SHAKE128 && algo != NTT_XOF_SHAKE256)) return NTT_ERR_PARAM;
    const size_t rate = algo == NTT_XOF_SHAKE128 ? 8 * XOF_RATE128 : 8 * XOF_RATE256;
    if (rows < 1 || rows > NTT_GAUSS_ROWS_MAX || cols < 1 || cols > NTT_GAUSS_COLS_MAX || nonce > 255) return NTT_ERR_PARAM;
    if ((seedlen & 7u) || seedlen < 8 || seedlen > rate - 8) return NTT_ERR_PARAM;   // one absorb block
    if (batch == 0) return NTT_OK;
    if (!d_out || !d_seed || !d_cdt) return NTT_ERR_NULL;
    if ((((uintptr_t)d_out) & 15u) || (((uintptr_t)d_seed) & 7u) || (((uintptr_t)d_cdt) & 3u) || (((uintptr_t)d_nonce) & 3u))
        return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t obytes = batch * p->n * 4;
    if (ranges_overlap(d_out, obytes, d_seed, batch * seedlen) || (d_nonce && ranges_overlap(d_out, obytes, d_nonce, batch * 4)) ||
        ranges_overlap(d_out, obytes, d_cdt, (size_t)rows * cols * 4))
        return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const uint32_t lcpp = p->logn - 9;   // n / 512 chunks a polynomial
    const dim3 grid((uint32_t)ceil_div(batch << lcpp, (size_t)GAUSS_WG));
    const uint32_t sw = (uint32_t)(seedlen / 8);
    if (algo == NTT_XOF_SHAKE128)
        launch_gauss<XOF_RATE128>(cols, grid, (hipStream_t)stream, d_out, (const uint64_t *)d_seed, sw, d_nonce, nonce, d_cdt,
                                  (uint32_t)rows, (uint32_t)batch, lcpp, p->q);
    else
        launch_gauss<XOF_RATE256>(cols, grid, (hipStream_t)stream, d_out, (const uint64_t *)d_seed, sw, d_nonce, nonce, d_cdt,
                                  (uint32_t)rows, (uint32_t)batch, lcpp, p->q);
    return finish_launch();
}

int poly_hsum(uint64_t *d_sum, const uint32_t *d_w, size_t batch, int h, int ps, void *stream)
{
    const ParamSet *p = param_set(ps);
    if (!p || h < 1 || (uint32_t)h > p->n) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_sum || !d_w) return NTT_ERR_NULL;
    if ((((uintptr_t)d_w) & 15u) || (((uintptr_t)d_sum) & 7u)) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    if (ranges_overlap(d_sum, batch * 8, d_w, batch * p->n * 4)) return NTT_ERR_ALIAS;
    return launch<LHsum>(ps, d_sum, d_w, batch, h, (hipStream_t)stream);
}

int poly_pack(uint8_t *d_out, size_t stride, const uint32_t *d_w, size_t batch, int k, int bits, int sgn, int ps, void *stream)
{
    return pack_common(d_out, d_w, nullptr, false, stride, batch, k, bits, sgn, ps, stream);
}

int poly_unpack(uint32_t *d_w, uint32_t *d_max, const uint8_t *d_in, size_t stride, size_t batch, int k, int bits, int sgn,
                int ps, void *stream)
{
    return pack_common(d_in, d_w, d_max, true, stride, batch, k, bits, sgn, ps, stream);
}

int poly_unpack_ntt(uint32_t *d_out, size_t pstride, uint32_t *d_max, const uint8_t *d_in, size_t stride, size_t batch, int k,
                    int bits, int sgn, int neg, int ps, void *stream)
{
    const ParamSet *p = row_param_set(ps, k, 1);   // n <= 2048, k
    if (!p || (sgn != 0 && sgn != 1) || (neg != 0 && neg != 1)) return NTT_ERR_PARAM;
    int qbits = 0;
    while (p->q >> qbits) ++qbits;
    if (bits < 8 || bits > qbits - sgn) return NTT_ERR_PARAM;
    const size_t packed = (size_t)k * p->n * (size_t)bits / 8;
    if ((stride & 15u) || stride < packed) return NTT_ERR_PARAM;
    if (pstride < p->n || (pstride & 3u)) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_out || !d_in) return NTT_ERR_NULL;
    if ((((uintptr_t)d_out) | ((uintptr_t)d_in)) & 15u || (((uintptr_t)d_max) & 3u)) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF / (size_t)k) return NTT_ERR_SIZE;
    const size_t bbytes = (batch - 1) * stride + packed, obytes = ((batch * k - 1) * pstride + p->n) * 4, mbytes = batch * k * 4;
    if (ranges_overlap(d_out, obytes, d_in, bbytes)) return NTT_ERR_ALIAS;
    if (d_max && (ranges_overlap(d_max, mbytes, d_in, bbytes) || ranges_overlap(d_max, mbytes, d_out, obytes))) return NTT_ERR_ALIAS;
    const PackRows R = {stride, (uint32_t)k, (uint32_t)bits, sgn ? 1u << (bits - 1) : 0u, p->q,
                        (uint32_t)(((uint64_t)1 << 32) / (uint32_t)bits) + 1u};
    return launch<LUnpackNtt, LARGE_PS0>(ps, d_out, pstride, d_max, (const uint32_t *)d_in, R, neg != 0, batch * k,
                                         (hipStream_t)stream);
}

int ntt_rows_over(uint32_t *d_flag, const void *d_vals, int width, int m, const uint64_t *bounds, int accumulate, size_t batch,
                  void *stream)
{
    if ((width != 32 && width != 64) || m < 1 || m > NTT_ROWS_M_MAX || (accumulate != 0 && accumulate != 1)) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_flag || !d_vals || !bounds) return NTT_ERR_NULL;
    if ((((uintptr_t)d_flag) & 3u) || (((uintptr_t)d_vals) & (uintptr_t)(width / 8 - 1))) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    if (ranges_overlap(d_flag, batch * 4, d_vals, batch * (size_t)m * (size_t)(width / 8))) return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    RowBounds rb = {};
    for (int j = 0; j < m; j++) rb.b[j] = bounds[j];
    const dim3 grid = rows_grid(batch, ROWS_WG, *d), wg(ROWS_WG);
    if (width == 32)
        hipLaunchKernelGGL(k_rows_over<uint32_t>, grid, wg, 0, (hipStream_t)stream, d_flag, (const uint32_t *)d_vals, (uint32_t)m,
                           rb, (uint32_t)accumulate, (uint32_t)batch);
    else
        hipLaunchKernelGGL(k_rows_over<uint64_t>, grid, wg, 0, (hipStream_t)stream, d_flag, (const uint64_t *)d_vals, (uint32_t)m,
                           rb, (uint32_t)accumulate, (uint32_t)batch);
    return finish_launch();
}

int ntt_rows_differ(uint32_t *d_flag, const uint8_t *d_a, size_t a_stride, const uint8_t *d_b, size_t b_stride, size_t row_bytes,
                    int accumulate, size_t batch, void *stream)
{
    if ((row_bytes & 3u) || row_bytes < 4 || ((a_stride | b_stride) & 3u) || a_stride < row_bytes || b_stride < row_bytes)
        return NTT_ERR_PARAM;
    if (accumulate != 0 && accumulate != 1) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_flag || !d_a || !d_b) return NTT_ERR_NULL;
    if ((((uintptr_t)d_flag) | ((uintptr_t)d_a) | ((uintptr_t)d_b)) & 3u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    if (ranges_overlap(d_flag, batch * 4, d_a, rows_extent(batch, a_stride, row_bytes)) ||
        ranges_overlap(d_flag, batch * 4, d_b, rows_extent(batch, b_stride, row_bytes)))
        return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const uint32_t llpr = row_lanes_log(row_bytes / 4, 6);   // a group never spans two waves
    hipLaunchKernelGGL(k_rows_differ, rows_grid(batch, ROWS_WG >> llpr, *d), dim3(ROWS_WG), 0, (hipStream_t)stream, d_flag,
                       (const uint32_t *)d_a, a_stride / 4, (const uint32_t *)d_b, b_stride / 4, row_bytes / 4,
                       (uint32_t)accumulate, (uint32_t)batch, llpr);
    return finish_launch();
}

int ntt_select(uint32_t *d_idx, uint32_t *d_count, const uint32_t *d_flag, int want, uint32_t *d_bump, size_t batch, void *stream)
{
    if (want != 0 && want != 1) return NTT_ERR_PARAM;
    if (batch == 0) return NTT_OK;
    if (!d_idx || !d_count || !d_flag) return NTT_ERR_NULL;
    if ((((uintptr_t)d_idx) | ((uintptr_t)d_count) | ((uintptr_t)d_flag) | ((uintptr_t)d_bump)) & 3u) return NTT_ERR_ALIGN;
    if (batch > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    // idx, count, flag and bump: no two of them overlap
    const void *p[4] = {d_idx, d_count, d_flag, d_bump};
    const size_t bytes[4] = {batch * 4, 4, batch * 4, batch * 4};
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (p[i] && p[j] && ranges_overlap(p[i], bytes[i], p[j], bytes[j])) return NTT_ERR_ALIAS;
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    hipLaunchKernelGGL(k_select, dim3(1), dim3(SELECT_WG), 0, (hipStream_t)stream, d_idx, d_count, d_flag, (uint32_t)want, d_bump,
                       (uint32_t)batch);
    return finish_launch();
}

int ntt_rows_move(uint8_t *d_dst, size_t dst_stride, const uint32_t *d_dst_idx, size_t dst_rows, const uint8_t *d_src,
                  size_t src_stride, const uint32_t *d_src_idx, size_t src_rows, size_t row_bytes, const uint32_t *d_count,
                  size_t count, void *stream)
{
    if ((row_bytes & 3u) || row_bytes < 4 || ((dst_stride | src_stride) & 3u) || dst_stride < row_bytes || src_stride < row_bytes)
        return NTT_ERR_PARAM;
    if (count == 0) return NTT_OK;
    if (!d_dst || !d_src) return NTT_ERR_NULL;
    if ((((uintptr_t)d_dst) | ((uintptr_t)d_src) | ((uintptr_t)d_dst_idx) | ((uintptr_t)d_src_idx) | ((uintptr_t)d_count)) & 3u)
        return NTT_ERR_ALIGN;
    if (count > (size_t)0x7FFFFFFF || dst_rows > (size_t)0x7FFFFFFF || src_rows > (size_t)0x7FFFFFFF) return NTT_ERR_SIZE;
    const size_t dbytes = rows_extent(dst_rows, dst_stride, row_bytes);
    const size_t sbytes = rows_extent(src_rows, src_stride, row_bytes);
    if (dbytes && ((sbytes && ranges_overlap(d_dst, dbytes, d_src, sbytes)) ||
                   (d_dst_idx && ranges_overlap(d_dst, dbytes, d_dst_idx, count * 4)) ||
                   (d_src_idx && ranges_overlap(d_dst, dbytes, d_src_idx, count * 4)) ||
                   (d_count && ranges_overlap(d_dst, dbytes, d_count, 4))))
        return NTT_ERR_ALIAS;   // an extent of no rows overlaps nothing
    int rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    // 16-byte units when both bases, both strides and the row allow it, dwords otherwise
    const bool wide = !((((uintptr_t)d_dst) | ((uintptr_t)d_src) | dst_stride | src_stride | row_bytes) & 15u);
    const size_t units = row_bytes / (wide ? 16 : 4);
    const uint32_t llpr = row_lanes_log(units, 8);   // at most the workgroup
    const dim3 grid = rows_grid(count, ROWS_WG >> llpr, *d), wg(ROWS_WG);
    if (wide)
        hipLaunchKernelGGL(k_rows_move<uint4>, grid, wg, 0, (hipStream_t)stream, d_dst, dst_stride, d_dst_idx, dst_rows, d_src,
                           src_stride, d_src_idx, src_rows, units, d_count, (uint32_t)count, llpr);
    else
        hipLaunchKernelGGL(k_rows_move<uint32_t>, grid, wg, 0, (hipStream_t)stream, d_dst, dst_stride, d_dst_idx, dst_rows, d_src,
                           src_stride, d_src_idx, src_rows, units, d_count, (uint32_t)count, llpr);
    return finish_launch();
}

int poly_mul_nussbaumer(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b, size_t batch, int ps, int ring,
                        void *stream)
{
    int rc;
    if ((rc = check_common(ps, d_a, batch)) != NTT_OK) return rc;
    if (ring != NTT_RING_Q && ring != NTT_RING_M32) return NTT_ERR_PARAM;
    if (param_set(ps)->n > 2048) return NTT_ERR_PARAM;   // Nussbaumer splits for n = 1024 / 2048
    if ((rc = check_abc(ps, d_a, d_b, d_c, batch, 15u)) != NTT_OK || batch == 0) return rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const int e = nussbaumer_launch(ps, ring, d_a, d_b, d_c, batch, stream, d->cus);
    if (e != (int)hipSuccess) return hip_err((hipError_t)e);
    return NTT_OK;
}

int poly_pointwise(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b, size_t batch, int ps, void *stream)
{
    int rc = check_abc(ps, d_a, d_b, d_c, batch, 15u);
    if (rc != NTT_OK || batch == 0) return rc;
    return launch<LPw>(ps, d_a, d_b, d_c, batch * param_set(ps)->n / 4, (hipStream_t)stream);
}

int ntt_fill_uniform(uint32_t *d_poly, size_t batch, int ps, uint64_t seed, uint64_t first_poly, void *stream)
{
    int rc = check_common(ps, d_poly, batch);
    if (rc != NTT_OK || batch == 0) return rc;
    DevInfo *d = nullptr;
    if ((rc = device_ready(&d)) != NTT_OK) return rc;
    const ParamSet *p = param_set(ps);
    const size_t count = batch * p->n;
    hipLaunchKernelGGL(k_fill_uniform, dim3(capped_grid(count, WG, d->cus, 16)), dim3(WG), 0, (hipStream_t)stream, d_poly,
                       count, p->q, seed, first_poly * p->n);
    return finish_launch();
}

int ntt_small_batch_max(int ps, int op, size_t *max_batch)
{
    if (!param_set(ps)) return NTT_ERR_PARAM;
    if (op < 0 || op >= LAT_NOPS) return NTT_ERR_PARAM;
    if (!max_batch) return NTT_ERR_NULL;
    *max_batch = lat_max_batch(ps, op);
    return NTT_OK;
}

int ntt_small_batch_radix(int ps, int op, size_t batch, int *radix)
{
    if (!param_set(ps)) return NTT_ERR_PARAM;
    if (op < 0 || op >= LAT_NOPS) return NTT_ERR_PARAM;
    if (!radix) return NTT_ERR_NULL;
    const int rb = lat_radix(ps, op, batch);
    *radix = rb ? 1 << rb : 0;
    return NTT_OK;
}

int ntt_last_hip_error(void) { return t_last_hip; }

int ntt_sync_expiries(uint32_t *count)
{
    if (!count) return NTT_ERR_NULL;
    const hipError_t e = hipMemcpyFromSymbol(count, HIP_SYMBOL(g_slot_sync_expired), sizeof(uint32_t), 0,
                                             hipMemcpyDeviceToHost);
    return e != hipSuccess ? hip_err(e) : NTT_OK;
}

const char *ntt_strerror(int code)
{
    switch (code) {
    case NTT_OK: return "ok";
    case NTT_ERR_PARAM: return "unknown param_set";
    case NTT_ERR_NULL: return "NULL device pointer";
    case NTT_ERR_ALIGN: return "misaligned device pointer";
    case NTT_ERR_HIP: return "HIP runtime error";
    case NTT_ERR_SIZE: return "batch too large";
    case NTT_ERR_ALIAS: return "partially overlapping buffers";
    default: return "unknown error";
    }
}

// Build identity: the kernel design, the compiled launch configuration and a
// hash of the library sources ("src=<16 hex>"), so that committed counter
// summaries (profiles/pmc_summary.json) can be tied to the build they were
// measured on.
int ntt_build_info(char *buf, size_t len)
{
    static const char *s =
        "qtesla_ntt gfx950: 1 launch/op, wave-per-poly (n=2048) / half-wave-per-poly (n=1024), 32 coeff/lane, "
        "LDS XOR-swizzled transpose, permlane32 bit-5 stage, Shoup/Harvey lazy CT + signed-Shoup GS butterflies, "
        "dispatch-ordered unit chunks; small batches (per-(n, op) switch, ntt_small_batch_max) one poly per "
        "n/4-thread workgroup; wg=" QNTT_STR(NTT_WG)
        " mul_wg=" QNTT_STR(MUL_WG) " mul_compact=1 ppw<=" QNTT_STR(NTT_PPW_MAX)
        " min_wg/cu=" QNTT_STR(NTT_MIN_WG_PER_CU) "; src=" QNTT_SRC_HASH;
    const int n = (int)strlen(s);
    if (!buf || !len) return n;
    snprintf(buf, len, "%s", s);
    return n;
}

}  // extern "C"
