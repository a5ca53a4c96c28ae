// arith_probe.hip -- test-only library (lib/libqtesla_ntt_arith.so, `make
// testlibs`): the device arithmetic primitives of csrc/ntt_device.hpp,
// ntt_mulkl.hpp and ntt_round.hpp, each applied element-wise to `count`
// independent operand tuples, so that tests/test_gpu_device_arith.py can
// compare the functions the kernels inline with exact integer arithmetic on
// operands it chooses (lazy representatives, boundary words, chosen twiddles).
// The product headers are included unchanged; nothing here is linked into
// the product library and csrc/ is not touched, so the product's src= hash
// does not depend on this file.
//
// Data layout: structure of arrays, operand c of element i at in[c * count + i],
// result c at out[c * count + i] (coalesced; the caller states both sizes and
// a mismatch is rejected before any launch).  Every kernel is a grid-stride
// loop whose accesses are all guarded by i < count.
//
//   scalar primitives    one thread per element
//   register-set forms   one lane per 32-register set (BaseMul::run,
//                        inv_pass2's WIDE0 stage, inv_last_stage)
//
// The register-set forms that read a lane twiddle through tw2_idx get a
// per-workgroup LDS table in the kernels' own lane-major layout in which a
// lane's column holds, in every entry, the one pair of that lane's element:
// which entry a stage reads then does not matter, and every element of a
// launch has its own twiddle.
//
// Host entry points return the library's own constexpr constants (cshoup,
// csigned_tw, cqinv_neg, the per-set QNEG / R / NINV_R / ...): no device needed.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../csrc/ntt_device.hpp"
#include "../csrc/ntt_mulkl.hpp"
#include "../csrc/ntt_round.hpp"

namespace {
using namespace qntt;

enum Prim {
    PR_CSUB_Q = 0,
    PR_CSUB_2Q,
    PR_CANON4,
    PR_BM_CANON,    // variant = s
    PR_BM_HALF,     // variant = s
    PR_SHOUP,
    PR_SSHOUP,
    PR_CT_BFLY,     // variant = index into the seven (RED, XS, YS, YOS) forms below
    PR_GS_BFLY,
    PR_MONT_MUL,
    PR_MONT_DOT1,
    PR_MONT_DOT2,
    PR_REDC,
    PR_BM_RUN,      // variant = ODD_S
    PR_INV_WIDE0,
    PR_INV_LAST,    // variant = CANON + 2 * (constants of the MUL_LOGR-short inverse)
    PR_ROUND,
    PR_COUNT
};

// ---- scalar primitives: f(a[NIN], o[NOUT]) --------------------------------
template <class P> struct FCsubQ {
    static constexpr int NIN = 1, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = csub<P::Q>(a[0]); }
};
template <class P> struct FCsub2Q {
    static constexpr int NIN = 1, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = csub<P::Q2>(a[0]); }
};
template <class P> struct FCanon4 {
    static constexpr int NIN = 1, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = canon4<P>(a[0]); }
};
template <class P, bool S> struct FBmCanon {
    static constexpr int NIN = 1, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = BaseMul<P, MUL_LOGR>::canon(S, a[0]); }
};
template <class P, bool S> struct FBmHalf {
    static constexpr int NIN = 1, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = BaseMul<P, MUL_LOGR>::half(S, a[0]); }
};
template <class P> struct FShoup {   // a, w, wp
    static constexpr int NIN = 3, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = shoup_mul<P::Q>(a[0], a[1], a[2]); }
};
template <class P> struct FSShoup {   // d, ws, wps
    static constexpr int NIN = 3, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = sshoup_mul<P::Q>(a[0], a[1], a[2]); }
};
template <class P, bool RED, bool XS, bool YS, bool YOS> struct FCtBfly {   // x, y, wn, wp -> x', y'
    static constexpr int NIN = 4, NOUT = 2;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o)
    {
        uint32_t x = a[0], y = a[1];
        ct_bfly_t<P::Q, RED, XS, YS, YOS>(x, y, a[2], a[3]);
        o[0] = x;
        o[1] = y;
    }
};
template <class P> struct FGsBfly {   // x, y, ws, wps -> x', y'
    static constexpr int NIN = 4, NOUT = 2;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o)
    {
        uint32_t x = a[0], y = a[1];
        gs_bfly<P::Q>(x, y, a[2], a[3]);
        o[0] = x;
        o[1] = y;
    }
};
template <class P> struct FMontMul {
    static constexpr int NIN = 2, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o) { o[0] = mont_mul<P>(a[0], a[1]); }
};
template <class P, int L> struct FMontDot {   // y[0..L), a[0..L)
    static constexpr int NIN = 2 * L, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o)
    {
        uint32_t y[L], v[L];
#pragma unroll
        for (int t = 0; t < L; ++t) {
            y[t] = a[t];
            v[t] = a[L + t];
        }
        o[0] = mont_dot<P, L>(y, v);
    }
};
template <class P> struct FRedc {   // c = lo, hi
    static constexpr int NIN = 2, NOUT = 1;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o)
    {
        o[0] = BaseMul<P, MUL_LOGR>::redc(((uint64_t)a[1] << 32) | a[0]);
    }
};
template <class P> struct FRound {   // x, d -> hi, |c|, |lo|
    static constexpr int NIN = 2, NOUT = 3;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o)
    {
        int32_t hi;
        round_coeff<P>(a[0], a[1], hi, o[1], o[2]);
        o[0] = (uint32_t)hi;
    }
};
// inv_last_stage: r[32] -> r'[32], then the 32 words the emit callback saw
struct EmitTo {
    uint32_t *o;
    __device__ __forceinline__ void operator()(int j, uint32_t v) const { o[j] = v; }
};
template <class P, bool CANON, bool SHORT> struct FInvLast {
    static constexpr int NIN = 32, NOUT = 64;
    static constexpr uint32_t S0 = SHORT ? P::template ninv_r<MUL_LOGR>() : P::NINV_R;
    static constexpr uint32_t S1 = SHORT ? P::template c1_r<MUL_LOGR>() : P::C1_R;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o)
    {
        constexpr uint32_t S0P = cshoup(S0, P::Q);
        constexpr TwPair S1S = csigned_tw(S1, P::Q);
        uint32_t r[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) r[j] = a[j];
        inv_last_stage<P, CANON>(r, S0, S0P, S1S.x, S1S.y, EmitTo{o + 32});
#pragma unroll
        for (int j = 0; j < 32; ++j) o[j] = r[j];
    }
};

constexpr int ELEM_WG = 256;
template <class F>
__global__ __launch_bounds__(ELEM_WG) void k_elem(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count)
{
    const size_t step = (size_t)gridDim.x * ELEM_WG;
    for (size_t i = (size_t)blockIdx.x * ELEM_WG + threadIdx.x; i < count; i += step) {
        uint32_t a[F::NIN], o[F::NOUT];
#pragma unroll
        for (int c = 0; c < F::NIN; ++c) a[c] = in[(size_t)c * count + i];
        F::run(a, o);
#pragma unroll
        for (int c = 0; c < F::NOUT; ++c) out[(size_t)c * count + i] = o[c];
    }
}

// ---- register-set forms with a lane twiddle: f(a, o, tab, lane) -------------
// operands: the registers, then the element's pair (x, y of the table's uint2)
template <class P, bool ODD_S> struct FBmRun {   // ra[32], rb[32], (-w mod 2^32, w') -> ra'[32]
    static constexpr int NIN = 66, NOUT = 32, TW = 64;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o, const uint2 *tab, uint32_t lane)
    {
        uint32_t ra[32], rb[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            ra[j] = a[j];
            rb[j] = a[32 + j];
        }
        BaseMul<P, MUL_LOGR>::template run<ODD_S>(ra, rb, tab, lane);
#pragma unroll
        for (int j = 0; j < 32; ++j) o[j] = ra[j];
    }
};
template <class P> struct FInvWide0 {   // r[32], (ws, wps) -> r'[32]: the stage on pos bit 4 in WIDE0 form
    static constexpr int NIN = 34, NOUT = 32, TW = 32;
    static __device__ __forceinline__ void run(const uint32_t *a, uint32_t *o, const uint2 *tab, uint32_t lane)
    {
        uint32_t r[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) r[j] = a[j];
        inv_pass2<P, 4, true>(r, tab, lane);
#pragma unroll
        for (int j = 0; j < 32; ++j) o[j] = r[j];
    }
};

// One wave per workgroup.  The table is the kernels' lane-major one: entry e,
// lane t at tab[e * tw2_lanes + t]; with 32-lane tables (n = 1024) each
// half-wave owns one table, as each half-wave owns one polynomial there.
constexpr int TAB_WG = 64;
template <class P, class F>
__global__ __launch_bounds__(TAB_WG) void k_tab(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t count)
{
    constexpr uint32_t LANES = tw2_lanes<P>();
    static_assert(TAB_WG % LANES == 0, "the half-wave tables tile the LDS array");
    __shared__ uint2 lds[TW2_ENTRIES * TAB_WG];
    const uint32_t lane = threadIdx.x & (LANES - 1);
    uint2 *tab = lds + (threadIdx.x / LANES) * (TW2_ENTRIES * LANES);
    const size_t step = (size_t)gridDim.x * TAB_WG;
    for (size_t i = (size_t)blockIdx.x * TAB_WG + threadIdx.x; i < count; i += step) {
        uint32_t a[F::NIN], o[F::NOUT];
#pragma unroll
        for (int c = 0; c < F::NIN; ++c) a[c] = in[(size_t)c * count + i];
        // this lane's column only: written and read by the same thread, no barrier
        const uint2 w = make_uint2(a[F::TW], a[F::TW + 1]);
#pragma unroll
        for (int e = 0; e < TW2_ENTRIES; ++e) tab[tw2_idx<P>(e, lane)] = w;
        compiler_fence();
        F::run(a, o, tab, lane);
        compiler_fence();
#pragma unroll
        for (int c = 0; c < F::NOUT; ++c) out[(size_t)c * count + i] = o[c];
    }
}

constexpr int ERR_PARAM = -1, ERR_NULL = -2, ERR_HIP = -4, ERR_SIZE = -5;

template <class F>
int check_sizes(const uint32_t *in, uint32_t *out, size_t in_words, size_t out_words, size_t count)
{
    if (!in || !out) return ERR_NULL;
    if (count == 0 || count > ((size_t)1 << 26)) return ERR_SIZE;
    if (in_words != (size_t)F::NIN * count || out_words != (size_t)F::NOUT * count) return ERR_SIZE;
    return 0;
}
template <class F>
int launch_elem(const uint32_t *in, uint32_t *out, size_t in_words, size_t out_words, size_t count, hipStream_t s)
{
    if (const int rc = check_sizes<F>(in, out, in_words, out_words, count)) return rc;
    const size_t nb = (count + ELEM_WG - 1) / ELEM_WG;
    hipLaunchKernelGGL(k_elem<F>, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(ELEM_WG), 0, s, in, out, count);
    return hipGetLastError() == hipSuccess ? 0 : ERR_HIP;
}
template <class P, class F>
int launch_tab(const uint32_t *in, uint32_t *out, size_t in_words, size_t out_words, size_t count, hipStream_t s)
{
    if (const int rc = check_sizes<F>(in, out, in_words, out_words, count)) return rc;
    const size_t nb = (count + TAB_WG - 1) / TAB_WG;
    hipLaunchKernelGGL((k_tab<P, F>), dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(TAB_WG), 0, s, in, out, count);
    return hipGetLastError() == hipSuccess ? 0 : ERR_HIP;
}

#define ELEM(...) return launch_elem<__VA_ARGS__>(in, out, in_words, out_words, count, s)
#define TAB(...) return launch_tab<P, __VA_ARGS__>(in, out, in_words, out_words, count, s)

template <class P>
int run_set(int prim, int v, const uint32_t *in, uint32_t *out, size_t in_words, size_t out_words, size_t count, hipStream_t s)
{
    switch (prim) {
    case PR_CSUB_Q: if (v == 0) ELEM(FCsubQ<P>); break;
    case PR_CSUB_2Q: if (v == 0) ELEM(FCsub2Q<P>); break;
    case PR_CANON4: if (v == 0) ELEM(FCanon4<P>); break;
    case PR_BM_CANON:
        if (v == 0) ELEM(FBmCanon<P, false>);
        if (v == 1) ELEM(FBmCanon<P, true>);
        break;
    case PR_BM_HALF:
        if (v == 0) ELEM(FBmHalf<P, false>);
        if (v == 1) ELEM(FBmHalf<P, true>);
        break;
    case PR_SHOUP: if (v == 0) ELEM(FShoup<P>); break;
    case PR_SSHOUP: if (v == 0) ELEM(FSShoup<P>); break;
    case PR_CT_BFLY:   // the forms fwd_pass1_lz, fwd_pass2_lz and ct_bfly instantiate
        if (v == 0) ELEM(FCtBfly<P, false, false, false, true>);
        if (v == 1) ELEM(FCtBfly<P, true, true, true, true>);
        if (v == 2) ELEM(FCtBfly<P, true, true, true, false>);
        if (v == 3) ELEM(FCtBfly<P, true, false, false, true>);
        if (v == 4) ELEM(FCtBfly<P, true, false, false, false>);
        if (v == 5) ELEM(FCtBfly<P, true, true, false, true>);
        if (v == 6) ELEM(FCtBfly<P, true, true, false, false>);
        break;
    case PR_GS_BFLY: if (v == 0) ELEM(FGsBfly<P>); break;
    case PR_MONT_MUL: if (v == 0) ELEM(FMontMul<P>); break;
    case PR_MONT_DOT1: if (v == 0) ELEM(FMontDot<P, 1>); break;
    case PR_MONT_DOT2: if (v == 0) ELEM(FMontDot<P, 2>); break;
    case PR_REDC: if (v == 0) ELEM(FRedc<P>); break;
    case PR_BM_RUN:
        if (v == 0) TAB(FBmRun<P, false>);
        if (v == 1) TAB(FBmRun<P, true>);
        break;
    case PR_INV_WIDE0: if (v == 0) TAB(FInvWide0<P>); break;
    case PR_INV_LAST:
        if (v == 0) ELEM(FInvLast<P, false, false>);
        if (v == 1) ELEM(FInvLast<P, true, false>);
        if (v == 2) ELEM(FInvLast<P, false, true>);
        if (v == 3) ELEM(FInvLast<P, true, true>);
        break;
    case PR_ROUND: if (v == 0) ELEM(FRound<P>); break;
    default: break;
    }
    return ERR_PARAM;
}
#undef ELEM
#undef TAB

template <class P>
void consts_of(uint32_t *o)
{
    using BM = BaseMul<P, MUL_LOGR>;
    const uint32_t v[16] = {P::Q, P::N, P::QNEG, P::R, P::NINV, P::C1, P::NINV_R, P::C1_R,
                            P::template ninv_r<MUL_LOGR>(), P::template c1_r<MUL_LOGR>(), (uint32_t)MUL_LOGR, P::PSI,
                            BM::AH, BM::WIDE, BM::OUT_CSUB_Z, BM::OUT_CSUB_H};
    for (int i = 0; i < 16; ++i) o[i] = v[i];
}
}  // namespace

// Applies primitive `prim` (enum Prim above) in form `variant` for parameter
// set ps (0 ref, 1 p-I, 2 p-III) to `count` elements.  d_in / d_out: device
// arrays of in_words / out_words words, which must equal the primitive's
// operand / result count times `count`.  0, or a negative NTT_ERR_* value.
extern "C" int arith_probe(int prim, int variant, int ps, const uint32_t *d_in, size_t in_words, uint32_t *d_out,
                           size_t out_words, size_t count, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (ps) {
    case 0: return run_set<qntt::PS0>(prim, variant, d_in, d_out, in_words, out_words, count, s);
    case 1: return run_set<qntt::PS1>(prim, variant, d_in, d_out, in_words, out_words, count, s);
    case 2: return run_set<qntt::PS2>(prim, variant, d_in, d_out, in_words, out_words, count, s);
    default: return ERR_PARAM;
    }
}

// Host only.  out[16]: Q, N, QNEG, R, NINV, C1, NINV_R, C1_R, ninv_r<MUL_LOGR>(),
// c1_r<MUL_LOGR>(), MUL_LOGR, PSI, then BaseMul<P, MUL_LOGR>'s AH, WIDE,
// OUT_CSUB_Z, OUT_CSUB_H.
extern "C" int arith_probe_consts(int ps, uint32_t *out)
{
    if (!out) return ERR_NULL;
    switch (ps) {
    case 0: consts_of<qntt::PS0>(out); return 0;
    case 1: consts_of<qntt::PS1>(out); return 0;
    case 2: consts_of<qntt::PS2>(out); return 0;
    default: return ERR_PARAM;
    }
}
extern "C" uint32_t arith_probe_cshoup(uint32_t w, uint32_t q) { return qntt::cshoup(w, q); }
extern "C" void arith_probe_csigned_tw(uint32_t w, uint32_t q, uint32_t *out)
{
    const qntt::TwPair p = qntt::csigned_tw(w, q);
    out[0] = p.x;
    out[1] = p.y;
}
extern "C" uint32_t arith_probe_cqinv_neg(uint32_t q) { return qntt::cqinv_neg(q); }
