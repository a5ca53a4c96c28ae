// ntt_main.cpp -- C++ host driver over the C ABI (include/qtesla_ntt.h).
//
// Mirrors the reference's CLI and GPU test drivers (benlwk/ntt-gpu-qTESLA
// main.cu:12-230, NTT.cu:2008-2443) so the same experiments can be run on
// MI355X through the drop-in boundary:
//
//   -speedgpu 4   CT-CT negacyclic poly-mul   (test_NTT_CT_CT_nega_gpu, NTT.cu:2181)
//   -speedgpu 6   CT-GS negacyclic poly-mul   (test_NTT_CT_GS_nega_gpu, NTT.cu:2358)
//                 both as poly_ntt x2 + poly_pointwise + poly_invntt
//   -speedgpu 7   fused poly_mul (one launch per batch)
//   -speedgpu 8   speed suite: 5 x option 6 then 5 x option 7 (main.cu:213-225)
//   -speedgpu 9   forward+inverse transform throughput (BASELINE metric)
//   -speedgpu 10  fused poly-mul host -> host through the pipelined host-buffer
//                 context (ntt_host_ctx: H2D / kernel / D2H overlapped), the
//                 reference's PCIe-inclusive timing region (NTT.cu:2384-2428)
//   -speedgpu 11  Nussbaumer product on the GPU in the reference's ring
//                 Z/(2^32-1) (test_nussbaumer, NTT.cu:1987-2005; -speedcpu 6 there)
//   -speedgpu 12  per-call latency through the C ABI, the qTESLA signing loop's
//                 use (one small batch per call): poly_ntt, poly_invntt and
//                 poly_mul, each (a) called back to back (calls/s the host
//                 sustains, HIP events around R calls) and (b) synchronised
//                 after every call (the round trip a caller that consumes the
//                 result sees)
//   -speedgpu 13  poly_mul_ntt_k, k shared NTT-domain rows times a batch in one
//                 launch (qTESLA's t_i = a_i y), against the k poly_mul_ntt
//                 launches over a materialised broadcast it replaces; -k K rows
//                 (default: the set's k, 1 / 4 / 5 for ref / p-I / p-III)
//   -speedgpu 14  poly_mul_ntt_kl with l = 2, qTESLA's verification
//                 w_i = a_i z - t_i c in one launch, against the two
//                 poly_mul_ntt_k launches it replaces (tmp = (-t_i) c, then
//                 a_i z + tmp accumulated in place); -k K as for 13
//   -speedgpu 15  poly_round (qTESLA's high bits and norm maxima): (a) alone,
//                 with both outputs, hi only and norms only, beside
//                 poly_pointwise over the same coefficients; (b) n <= 2048:
//                 poly_mul_ntt_kl_round (l = 2) against poly_mul_ntt_kl then
//                 poly_round; -k K as for 13, -d D bits (default: the set's
//                 own, 22 / 22 / 24), -leg a|b for one leg only
//   -speedgpu 16  the hashes round a verification, n <= 2048: (a) ntt_xof at the
//                 set's H shape (SHAKE128 / SHAKE256 over k n + 64 bytes, 32
//                 out) beside the same round's poly_mul_ntt_kl_round; (b)
//                 poly_challenge (seed 32, h = 25 / 40) then poly_scatter
//   -param ref|p-I|p-III|p-III-4096|p-III-8192   parameter set (reference:
//                 compile-time QTESLA set; the n = 4096 / 8192 sets run every
//                 option but 11, whose Nussbaumer split is n <= 2048)
//   -batch B      polynomials per batch (reference: BATCH macro, main.cuh:7)
//   -r seed       random operands from the device generator (reference parses
//                 -r but never uses it, main.cu:89-91); default: all-ones
//                 operands as in NTT.cu:2360, checked against the KAT
//                 z[k] = 2k + 2 - n mod q
//   -pcie         include H2D/D2H copies in the timed region like the reference
//                 (NTT.cu:2384-2428); default times device-resident data
//   -debug        print the first/last coefficients of z (the DEBUG dump)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qtesla_ntt.h"

#define HIP_OK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(2);                                                                       \
        }                                                                                  \
    } while (0)
#define NTT_CALL(x)                                                                        \
    do {                                                                                   \
        int rc_ = (x);                                                                     \
        if (rc_ != NTT_OK) {                                                               \
            fprintf(stderr, "%s failed: %s\n", #x, ntt_strerror(rc_));                     \
            exit(3);                                                                       \
        }                                                                                  \
    } while (0)

struct Opts {
    int option = 6, ps = NTT_PARAM_REF, reps = 1, k = 0, d = 0;
    char leg = 0;   // -speedgpu 15 / 16: 'a' / 'b' for one leg, 0 for both
    size_t batch = 2;
    bool random = false, pcie = false, debug = false;
    uint64_t seed = 0;
};

// ---- resource owners: what a run_* declares is released when it returns

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// `count` elements of device memory
template <class T> struct DevBuf : NoCopy {
    T *p = nullptr;
    explicit DevBuf(size_t count) { HIP_OK(hipMalloc(&p, count * sizeof(T))); }
    ~DevBuf() { HIP_OK(hipFree(p)); }
    operator T *() const { return p; }
};

struct Stream : NoCopy {
    hipStream_t s;
    Stream() { HIP_OK(hipStreamCreate(&s)); }
    ~Stream() { HIP_OK(hipStreamDestroy(s)); }
    operator hipStream_t() const { return s; }
};

template <int N> struct Events : NoCopy {
    hipEvent_t e[N];
    Events() { for (auto &x : e) HIP_OK(hipEventCreate(&x)); }
    ~Events() { for (auto &x : e) HIP_OK(hipEventDestroy(x)); }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// pinned host words for the host-buffer context (-speedgpu 10)
struct HostBuf : NoCopy {
    uint32_t *p;
    explicit HostBuf(size_t bytes) : p((uint32_t *)ntt_host_alloc(bytes))
    {
        if (!p) { fprintf(stderr, "ntt_host_alloc failed\n"); exit(2); }
    }
    ~HostBuf() { ntt_host_free(p); }
    operator uint32_t *() const { return p; }
};

// ---- the parameter set's shape and qTESLA's constants for it, -k / -d applied

struct Set {
    uint32_t n, q;
    int k, d;      // rows of the public matrix; bits dropped by the rounding
    int algo, h;   // -speedgpu 16: the hash H and the challenge's weight
};

static Set set_of(const Opts &o)
{
    Set p;
    NTT_CALL(ntt_param_info(o.ps, &p.n, &p.q, nullptr, nullptr, nullptr, nullptr));
    p.k = o.k > 0 ? o.k : o.ps == NTT_PARAM_REF ? 1 : o.ps == NTT_PARAM_P_I ? 4 : 5;
    p.d = o.d > 0 ? o.d : o.ps <= NTT_PARAM_P_I ? 22 : 24;
    p.algo = p.n == 1024 ? NTT_XOF_SHAKE128 : NTT_XOF_SHAKE256;
    p.h = p.n == 1024 ? 25 : 40;
    return p;
}

// ---- operands

// dst[0 .. count) = the n-word row at src, by doubling device copies
static void bcast(uint32_t *dst, const uint32_t *src, size_t count, uint32_t n, hipStream_t s)
{
    const size_t row = (size_t)n * 4;
    if (dst != src) HIP_OK(hipMemcpyAsync(dst, src, row, hipMemcpyDeviceToDevice, s));
    for (size_t have = 1; have < count; have *= 2) {
        const size_t cnt = have < count - have ? have : count - have;
        HIP_OK(hipMemcpyAsync(dst + have * n, dst, cnt * row, hipMemcpyDeviceToDevice, s));
    }
}

// dst[0 .. count) = the all-ones polynomial
static void fill_ones(uint32_t *dst, size_t count, uint32_t n, hipStream_t s)
{
    const std::vector<uint32_t> ones(n, 1);
    HIP_OK(hipMemcpy(dst, ones.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    bcast(dst, dst, count, n, s);
}

// ---- the timing protocol of -speedgpu 13 .. 16

struct Stat {
    double med, lo, hi;
};

static Stat stats(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return {v[v.size() / 2], v.front(), v.back()};
}

// The paths (fused first, then what it replaces) are timed with HIP events on
// the one stream `s`, alternating: after `warm` rounds of every path, each of
// the `reps` repetitions records an event, then per path runs it `inner` times
// back to back (small batches: event resolution) and records the next event.
// Returns median, min and max of the milliseconds per call, per path.
template <class... Path>
static std::array<Stat, sizeof...(Path)> time_paths(hipStream_t s, int reps, int inner, int warm, Path &&...path)
{
    constexpr int N = sizeof...(Path);
    for (int w = 0; w < warm; w++) (path(), ...);
    HIP_OK(hipStreamSynchronize(s));
    Events<N + 1> ev;
    std::vector<double> t[N];
    for (int r = 0; r < reps; r++) {
        int p = 0;
        auto leg = [&](auto &run) {
            for (int i = 0; i < inner; i++) run();
            HIP_OK(hipEventRecord(ev[++p], s));
        };
        HIP_OK(hipEventRecord(ev[0], s));
        (leg(path), ...);
        HIP_OK(hipEventSynchronize(ev[N]));
        for (p = 0; p < N; p++) {
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ev[p], ev[p + 1]));
            t[p].push_back(ms / inner);
        }
    }
    std::array<Stat, N> out;
    for (int p = 0; p < N; p++) out[p] = stats(t[p]);
    return out;
}

// ---- checks

// the product of two all-ones polynomials mod (x^n + 1, m)
static uint32_t kat_word(uint32_t j, uint32_t n, uint64_t m) { return (uint32_t)((2ull * j + 2 + m - n) % m); }

// every one of the `polys` polynomials at z is `scale` times that KAT
static bool all_kat(const uint32_t *z, size_t polys, uint32_t n, uint64_t m, uint32_t scale)
{
    for (size_t b = 0; b < polys; b++)
        for (uint32_t j = 0; j < n; j++)
            if (z[b * n + j] != (uint32_t)((uint64_t)scale * kat_word(j, n, m) % m)) return false;
    return true;
}

static const char *verdict(bool ok) { return ok ? "Identical." : "Incorrect result."; }

// 13 / 14 / 15(b) compare the first and the last min(batch, 256) entries of a
// batch (below 256 both windows are the whole batch): check(first, count) is
// called for the head, then for the tail, until one fails.
static size_t window(size_t batch) { return batch < 256 ? batch : 256; }

template <class Check> static bool head_and_tail(size_t batch, Check &&check)
{
    const size_t cnt = window(batch);
    return check((size_t)0, cnt) && check(batch - cnt, cnt);
}

// ---- what every option prints

__attribute__((format(printf, 1, 2))) static void banner(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    printf("\n========================\n");
    vprintf(fmt, ap);
    printf("\n========================\n");
    va_end(ap);
}

// -speedgpu 4 .. 11: time and rate of one product per polynomial, then the KAT (kat < 0: not checked)
static void print_product(const char *what, double ms, size_t batch, int kat, const char *ring)
{
    printf("Performance GPU %s \n Time\t\t: % .4f ms. \nThroughput\t: %.2f Multiplications per second\n", what, ms,
           (double)batch / ms * 1000.0);
    if (kat >= 0) printf("all-ones KAT z[k] = 2k+2-n mod %s: %s\n", ring, verdict(kat));
}

// -speedgpu 13 .. 15: a fused launch beside what it replaces, `work` items per call
static void print_pair(const char *fused, const char *base, const char *ratio, const Stat &f, const Stat &b, int reps,
                       double work, const char *unit)
{
    printf("%s: median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e %s\n", fused, f.med, f.lo, f.hi, reps,
           work / f.med * 1e3, unit);
    printf("%s: median %.4f ms (min %.4f, max %.4f), %.3e %s\n", base, b.med, b.lo, b.hi, work / b.med * 1e3, unit);
    printf("%s: %.3f\n", ratio, b.med / f.med);
}

// ---- the options

// -speedgpu 4 / 6 / 7: negacyclic poly-mul, inputs x, y (all ones or random), output z.
static void run_polymul(const Opts &o, const char *name, bool fused)
{
    const Set p = set_of(o);
    const uint32_t n = p.n;
    const size_t count = o.batch * n, bytes = count * 4;
    std::vector<uint32_t> x(count, 1), y(count, 1), z(count, 0);
    DevBuf<uint32_t> d_x(count), d_y(count), d_z(count);
    Stream s;
    if (o.random) {
        NTT_CALL(ntt_fill_uniform(d_x, o.batch, o.ps, o.seed, 0, s));
        NTT_CALL(ntt_fill_uniform(d_y, o.batch, o.ps, o.seed ^ 0xFFFF, 0, s));
        HIP_OK(hipMemcpyAsync(x.data(), d_x, bytes, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(y.data(), d_y, bytes, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    }
    auto body = [&]() {
        if (o.pcie) {
            HIP_OK(hipMemcpyAsync(d_x, x.data(), bytes, hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(d_y, y.data(), bytes, hipMemcpyHostToDevice, s));
        }
        if (fused) {
            NTT_CALL(poly_mul(d_z, d_x, d_y, o.batch, o.ps, s));
        } else {
            // CT-GS composition; unlike bit_reverse_copy_tbl_Phi_gpu the inputs are
            // kept (out-of-place forward transforms into d_z / scratch)
            NTT_CALL(poly_ntt_oop(d_z, d_x, o.batch, o.ps, s));
            NTT_CALL(poly_ntt(d_y, nullptr, o.batch, o.ps, s));
            NTT_CALL(poly_pointwise(d_z, d_z, d_y, o.batch, o.ps, s));
            NTT_CALL(poly_invntt(d_z, nullptr, o.batch, o.ps, s));
        }
        if (o.pcie) HIP_OK(hipMemcpyAsync(z.data(), d_z, bytes, hipMemcpyDeviceToHost, s));
    };
    if (!o.pcie) {   // device-resident: restore y each rep in the composed path
        HIP_OK(hipMemcpyAsync(d_x, x.data(), bytes, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(d_y, y.data(), bytes, hipMemcpyHostToDevice, s));
    }
    body();  // warm-up (also uploads the twiddle tables)
    HIP_OK(hipStreamSynchronize(s));
    double ms = 0.0;
    for (int r = 0; r < o.reps; r++) {
        if (!o.pcie && !fused) HIP_OK(hipMemcpyAsync(d_y, y.data(), bytes, hipMemcpyHostToDevice, s));
        HIP_OK(hipStreamSynchronize(s));
        auto t0 = std::chrono::steady_clock::now();
        body();
        HIP_OK(hipStreamSynchronize(s));
        auto t1 = std::chrono::steady_clock::now();
        ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    ms /= o.reps;
    if (!o.pcie) HIP_OK(hipMemcpy(z.data(), d_z, bytes, hipMemcpyDeviceToHost));
    banner("test_NTT_negacyclic %s GPU. Batch Size is %zu", name, o.batch);
    print_product((std::string(name) + " GPU").c_str(), ms, o.batch, o.random ? -1 : all_kat(z.data(), o.batch, n, p.q, 1), "q");
    if (o.debug) {
        printf("z: ");
        for (uint32_t i = 0; i < 8 && i < n; i++) printf("%u ", z[i]);
        printf("... %u\n", z[n - 1]);
    }
}

// -speedgpu 9: forward + inverse transform pairs, in place, and their round trip
static int run_fwdinv(const Opts &o)
{
    const uint32_t n = set_of(o).n;
    const size_t count = o.batch * n, bytes = count * 4;
    DevBuf<uint32_t> d_x(count), d_ref(count);
    Stream s;
    NTT_CALL(ntt_fill_uniform(d_x, o.batch, o.ps, o.seed, 0, s));
    HIP_OK(hipMemcpyAsync(d_ref, d_x, bytes, hipMemcpyDeviceToDevice, s));
    NTT_CALL(poly_ntt(d_x, nullptr, o.batch, o.ps, s));
    NTT_CALL(poly_invntt(d_x, nullptr, o.batch, o.ps, s));
    Events<2> ev;
    HIP_OK(hipEventRecord(ev[0], s));
    for (int r = 0; r < o.reps; r++) {
        NTT_CALL(poly_ntt(d_x, nullptr, o.batch, o.ps, s));
        NTT_CALL(poly_invntt(d_x, nullptr, o.batch, o.ps, s));
    }
    HIP_OK(hipEventRecord(ev[1], s));
    HIP_OK(hipEventSynchronize(ev[1]));
    float total = 0.f;
    HIP_OK(hipEventElapsedTime(&total, ev[0], ev[1]));
    const double ms = total / o.reps;
    std::vector<uint32_t> a(count), b(count);
    HIP_OK(hipMemcpy(a.data(), d_x, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b.data(), d_ref, bytes, hipMemcpyDeviceToHost));
    const bool ok = a == b;
    printf("fwd+inv n=%u: %.4f ms per batch of %zu -> %.3e pairs/s, %.1f GB/s algorithmic; round trip %s\n", n, ms, o.batch,
           o.batch / ms * 1e3, o.batch * 16.0 * n / ms / 1e6, verdict(ok));
    return ok ? 0 : 1;
}

// -speedgpu 10: host -> host fused product through ntt_host_ctx; all-ones (KAT) or random operands
static int run_polymul_host(const Opts &o)
{
    const Set p = set_of(o);
    const size_t count = o.batch * p.n, bytes = count * 4;
    HostBuf x(bytes), y(bytes), z(bytes);
    for (size_t i = 0; i < count; i++) x[i] = y[i] = 1;
    if (o.random) {
        DevBuf<uint32_t> d(count);
        NTT_CALL(ntt_fill_uniform(d, o.batch, o.ps, o.seed, 0, nullptr));
        HIP_OK(hipMemcpy(x, d, bytes, hipMemcpyDeviceToHost));
        NTT_CALL(ntt_fill_uniform(d, o.batch, o.ps, o.seed ^ 0xFFFF, 0, nullptr));
        HIP_OK(hipMemcpy(y, d, bytes, hipMemcpyDeviceToHost));
    }
    ntt_host_ctx *ctx = nullptr;
    NTT_CALL(ntt_host_ctx_create(&ctx, o.ps, 0, 0));
    NTT_CALL(poly_mul_host(ctx, z, x, y, o.batch));   // warm-up
    double ms = 0.0;
    for (int r = 0; r < o.reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        NTT_CALL(poly_mul_host(ctx, z, x, y, o.batch));
        auto t1 = std::chrono::steady_clock::now();
        ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    ms /= o.reps;
    NTT_CALL(ntt_host_ctx_destroy(ctx));
    const int kat = o.random ? -1 : all_kat(z, o.batch, p.n, p.q, 1);
    banner("test_NTT_negacyclic fused host->host (pipelined PCIe). Batch Size is %zu", o.batch);
    print_product("fused host->host", ms, o.batch, kat, "q");
    return kat == 0 ? 1 : 0;
}

// -speedgpu 11: Nussbaumer mod 2^32-1 on the GPU, all-ones operands
static int run_nussbaumer(const Opts &o)
{
    const uint32_t n = set_of(o).n;
    const size_t count = o.batch * n, bytes = count * 4;
    std::vector<uint32_t> z(count, 0);
    DevBuf<uint32_t> d_x(count), d_z(count);
    fill_ones(d_x, o.batch, n, nullptr);
    NTT_CALL(poly_mul_nussbaumer(d_z, d_x, d_x, o.batch, o.ps, NTT_RING_M32, nullptr));
    HIP_OK(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < o.reps; r++) NTT_CALL(poly_mul_nussbaumer(d_z, d_x, d_x, o.batch, o.ps, NTT_RING_M32, nullptr));
    HIP_OK(hipDeviceSynchronize());
    auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count() / o.reps;
    HIP_OK(hipMemcpy(z.data(), d_z, bytes, hipMemcpyDeviceToHost));
    const bool kat = all_kat(z.data(), o.batch, n, 0xFFFFFFFFull, 1);
    banner("test_nussbaumer GPU (mod 2^32-1). Batch Size is %zu", o.batch);
    print_product("Nussbaumer", ms, o.batch, kat, "2^32-1");
    return kat ? 0 : 1;
}

// -speedgpu 12: per-call latency of the small-batch entry points.  Not
// time_paths: (a) is a host-submission figure, wall clock around the calls.
static int run_latency(const Opts &o)
{
    const uint32_t n = set_of(o).n;
    const size_t count = o.batch * n;
    DevBuf<uint32_t> d_x(count), d_y(count), d_z(count);
    Stream s;
    NTT_CALL(ntt_fill_uniform(d_x, o.batch, o.ps, 1, 0, s));
    NTT_CALL(ntt_fill_uniform(d_y, o.batch, o.ps, 2, 0, s));
    Events<2> ev;
    const int calls = o.reps > 1 ? o.reps : 2000;
    struct Case {
        const char *name;
        int (*fn)(uint32_t *, uint32_t *, uint32_t *, size_t, int, hipStream_t);
    };
    const Case cases[] = {
        {"poly_ntt", [](uint32_t *x, uint32_t *, uint32_t *, size_t b, int ps, hipStream_t st) {
             return poly_ntt(x, nullptr, b, ps, st);
         }},
        {"poly_invntt", [](uint32_t *x, uint32_t *, uint32_t *, size_t b, int ps, hipStream_t st) {
             return poly_invntt(x, nullptr, b, ps, st);
         }},
        {"poly_mul", [](uint32_t *x, uint32_t *y, uint32_t *z, size_t b, int ps, hipStream_t st) {
             return poly_mul(z, x, y, b, ps, st);
         }},
    };
    for (const Case &c : cases) {
        for (int w = 0; w < 50; w++) NTT_CALL(c.fn(d_x, d_y, d_z, o.batch, o.ps, s));
        HIP_OK(hipStreamSynchronize(s));
        // (a) back to back
        auto t0 = std::chrono::steady_clock::now();
        HIP_OK(hipEventRecord(ev[0], s));
        for (int i = 0; i < calls; i++) NTT_CALL(c.fn(d_x, d_y, d_z, o.batch, o.ps, s));
        HIP_OK(hipEventRecord(ev[1], s));
        HIP_OK(hipEventSynchronize(ev[1]));
        auto t1 = std::chrono::steady_clock::now();
        float gpu_ms = 0.f;
        HIP_OK(hipEventElapsedTime(&gpu_ms, ev[0], ev[1]));
        const double wall_us = std::chrono::duration<double, std::micro>(t1 - t0).count() / calls;
        // (b) synchronised after every call
        auto t2 = std::chrono::steady_clock::now();
        for (int i = 0; i < calls; i++) {
            NTT_CALL(c.fn(d_x, d_y, d_z, o.batch, o.ps, s));
            HIP_OK(hipStreamSynchronize(s));
        }
        auto t3 = std::chrono::steady_clock::now();
        const double rt_us = std::chrono::duration<double, std::micro>(t3 - t2).count() / calls;
        printf("{\"op\": \"%s\", \"n\": %u, \"batch\": %zu, \"calls\": %d, \"back_to_back_us\": %.3f, "
               "\"gpu_events_us\": %.3f, \"round_trip_us\": %.3f}\n",
               c.name, n, o.batch, calls, wall_us, gpu_ms * 1e3 / calls, rt_us);
    }
    return 0;
}

// -speedgpu 13: out[b][i] = a_i * y_b for k shared NTT-domain rows, (a) one
// poly_mul_ntt_k launch, (b) the baseline it replaces: k back-to-back
// poly_mul_ntt launches over a materialised [k][batch][n] broadcast of the
// rows (time_paths).  All-ones operands: every row is the KAT; -r: random
// operands, the two paths must agree (head_and_tail).
static int run_mul_ntt_k(const Opts &o)
{
    const Set p = set_of(o);
    const uint32_t n = p.n;
    const int k = p.k;
    const size_t row = (size_t)n * 4, plane = o.batch * n;
    DevBuf<uint32_t> d_y(plane), d_ahat((size_t)k * n), d_out(k * plane);
    DevBuf<uint32_t> d_bc(k * plane), d_c(k * plane);   // the baseline's operand and result, [k][batch][n]
    Stream s;
    if (o.random) {
        NTT_CALL(ntt_fill_uniform(d_y, o.batch, o.ps, o.seed, 0, s));
        NTT_CALL(ntt_fill_uniform(d_ahat, k, o.ps, o.seed ^ 0xFFFF, 0, s));
    } else {
        fill_ones(d_y, o.batch, n, s);
        bcast(d_ahat, d_y, k, n, s);
    }
    NTT_CALL(poly_ntt(d_ahat, nullptr, k, o.ps, s));
    for (int i = 0; i < k; i++) bcast(d_bc + i * plane, d_ahat + (size_t)i * n, o.batch, n, s);
    auto fused = [&]() { NTT_CALL(poly_mul_ntt_k(d_out, d_y, d_ahat, nullptr, o.batch, k, o.ps, s)); };
    auto base = [&]() {
        for (int i = 0; i < k; i++) NTT_CALL(poly_mul_ntt(d_c + i * plane, d_y, d_bc + i * plane, o.batch, o.ps, s));
    };
    const int inner = k * plane < (1u << 24) ? 20 : 1;
    const auto [f, b] = time_paths(s, o.reps, inner, 3, fused, base);
    std::vector<uint32_t> z(window(o.batch) * k * n), c(window(o.batch) * n);
    const bool ok = head_and_tail(o.batch, [&](size_t b0, size_t cnt) {
        HIP_OK(hipMemcpy(z.data(), d_out + b0 * k * n, cnt * k * row, hipMemcpyDeviceToHost));
        if (!o.random) return all_kat(z.data(), cnt * k, n, p.q, 1);
        for (int i = 0; i < k; i++) {
            HIP_OK(hipMemcpy(c.data(), d_c + i * plane + b0 * n, cnt * row, hipMemcpyDeviceToHost));
            for (size_t t = 0; t < cnt; t++)
                if (memcmp(&c[t * n], &z[(t * k + i) * n], row) != 0) return false;
        }
        return true;
    });
    banner("poly_mul_ntt_k GPU. Batch Size is %zu, k = %d", o.batch, k);
    print_pair("poly_mul_ntt_k      ", (std::to_string(k) + " x poly_mul_ntt    ").c_str(), "baseline / fused    ", f, b, o.reps,
               (double)o.batch * k, "products/s");
    printf("%s: %s\n", o.random ? "fused == k x poly_mul_ntt" : "all-ones KAT z[k] = 2k+2-n mod q, every row", verdict(ok));
    return ok ? 0 : 1;
}

// -speedgpu 14: out[b][i] = a_i * z_b + t'_i * c_b for k rows of two shared
// NTT-domain polynomials (verification: t'_i-hat = q - t_i-hat), (a) one
// poly_mul_ntt_kl launch, (b) the composition it replaces: poly_mul_ntt_k of
// c over the rows t'_i, then poly_mul_ntt_k of z over the rows a_i with the
// first result as addend, in place (time_paths).  All-ones operands: every
// row is twice the KAT; -r: random operands, the two paths must agree
// (head_and_tail).
static int run_mul_ntt_kl(const Opts &o)
{
    const Set p = set_of(o);
    const uint32_t n = p.n;
    const int k = p.k;
    const size_t row = (size_t)n * 4, plane = o.batch * n, rows = (size_t)k * n;
    DevBuf<uint32_t> d_z(plane), d_c(plane);
    DevBuf<uint32_t> d_a(rows), d_t(rows);   // [k][n] a_i-hat and t'_i-hat
    DevBuf<uint32_t> d_at(2 * rows);         // [k][2][n] both, the fused launch's rows
    DevBuf<uint32_t> d_out(k * plane), d_base(k * plane);
    Stream s;
    if (o.random) {
        NTT_CALL(ntt_fill_uniform(d_z, o.batch, o.ps, o.seed, 0, s));
        NTT_CALL(ntt_fill_uniform(d_c, o.batch, o.ps, o.seed ^ 0xCCCC, 0, s));
        NTT_CALL(ntt_fill_uniform(d_a, k, o.ps, o.seed ^ 0xFFFF, 0, s));
        NTT_CALL(ntt_fill_uniform(d_t, k, o.ps, o.seed ^ 0xEEEE, 0, s));
    } else {
        fill_ones(d_z, o.batch, n, s);
        bcast(d_c, d_z, o.batch, n, s);
        bcast(d_a, d_z, k, n, s);
        bcast(d_t, d_z, k, n, s);
    }
    NTT_CALL(poly_ntt(d_a, nullptr, k, o.ps, s));
    NTT_CALL(poly_ntt(d_t, nullptr, k, o.ps, s));
    for (int i = 0; i < k; i++) {
        HIP_OK(hipMemcpyAsync(d_at + (size_t)(2 * i) * n, d_a + (size_t)i * n, row, hipMemcpyDeviceToDevice, s));
        HIP_OK(hipMemcpyAsync(d_at + (size_t)(2 * i + 1) * n, d_t + (size_t)i * n, row, hipMemcpyDeviceToDevice, s));
    }
    const uint32_t *ys[2] = {d_z, d_c};
    auto fused = [&]() { NTT_CALL(poly_mul_ntt_kl(d_out, ys, d_at, nullptr, o.batch, k, 2, o.ps, s)); };
    auto base = [&]() {
        NTT_CALL(poly_mul_ntt_k(d_base, d_c, d_t, nullptr, o.batch, k, o.ps, s));
        NTT_CALL(poly_mul_ntt_k(d_base, d_z, d_a, d_base, o.batch, k, o.ps, s));
    };
    const int inner = k * plane < (1u << 24) ? 20 : 1;
    const auto [f, b] = time_paths(s, o.reps, inner, 3, fused, base);
    std::vector<uint32_t> z(window(o.batch) * rows), c(window(o.batch) * rows);
    const bool ok = head_and_tail(o.batch, [&](size_t b0, size_t cnt) {
        HIP_OK(hipMemcpy(z.data(), d_out + b0 * rows, cnt * rows * 4, hipMemcpyDeviceToHost));
        if (!o.random) return all_kat(z.data(), cnt * k, n, p.q, 2);
        HIP_OK(hipMemcpy(c.data(), d_base + b0 * rows, cnt * rows * 4, hipMemcpyDeviceToHost));
        return memcmp(c.data(), z.data(), cnt * rows * 4) == 0;
    });
    banner("poly_mul_ntt_kl GPU. Batch Size is %zu, k = %d, l = 2", o.batch, k);
    print_pair("poly_mul_ntt_kl     ", "2 x poly_mul_ntt_k  ", "baseline / fused    ", f, b, o.reps, (double)o.batch * k, "rows/s");
    printf("%s: %s\n", o.random ? "fused == 2 x poly_mul_ntt_k" : "all-ones KAT z[k] = 2 (2k+2-n) mod q, every row", verdict(ok));
    return ok ? 0 : 1;
}

// -speedgpu 15, leg (a): poly_round alone over `batch` polynomials -- both
// outputs, hi only, norms only -- and poly_pointwise (12 B per coefficient)
// over the same coefficients; time and achieved bytes/s of each (time_paths).
static void run_round_alone(const Opts &o, const Set &p, hipStream_t s)
{
    const size_t coeffs = o.batch * p.n;
    const int d = p.d;
    DevBuf<uint32_t> d_w(coeffs), d_b(coeffs), d_c(coeffs), d_norms(o.batch * 2);
    DevBuf<uint8_t> d_hi(coeffs);
    NTT_CALL(ntt_fill_uniform(d_w, o.batch, o.ps, o.seed ^ 0x1111, 0, s));
    NTT_CALL(ntt_fill_uniform(d_b, o.batch, o.ps, o.seed ^ 0x2222, 0, s));
    const auto t = time_paths(
        s, o.reps, coeffs < (1u << 24) ? 20 : 1, 3,
        [&]() { NTT_CALL(poly_round(d_hi, d_norms, d_w, o.batch, d, o.ps, s)); },
        [&]() { NTT_CALL(poly_round(d_hi, nullptr, d_w, o.batch, d, o.ps, s)); },
        [&]() { NTT_CALL(poly_round(nullptr, d_norms, d_w, o.batch, d, o.ps, s)); },
        [&]() { NTT_CALL(poly_pointwise(d_c, d_w, d_b, o.batch, o.ps, s)); });
    const char *name[4] = {"poly_round hi+norms", "poly_round hi      ", "poly_round norms   ", "poly_pointwise     "};
    const double bytes[4] = {5.0 * coeffs + 8.0 * o.batch, 5.0 * coeffs, 4.0 * coeffs + 8.0 * o.batch, 12.0 * coeffs};
    banner("poly_round GPU. Batch Size is %zu, d = %d", o.batch, d);
    for (int i = 0; i < 4; i++)
        printf("%s : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.4e bytes, %.3f TB/s\n", name[i], t[i].med,
               t[i].lo, t[i].hi, o.reps, bytes[i], bytes[i] / t[i].med / 1e9);
}

// -speedgpu 15, leg (b): poly_mul_ntt_kl_round (l = 2) against poly_mul_ntt_kl
// into a temporary followed by poly_round over batch * k polynomials
// (time_paths); hi and norms of the two paths are compared (head_and_tail).
static bool run_round_fused(const Opts &o, const Set &p, hipStream_t s)
{
    const uint32_t n = p.n;
    const int k = p.k, d = p.d;
    const size_t plane = o.batch * n, npoly = o.batch * k;
    DevBuf<uint32_t> d_z(plane), d_c(plane), d_at((size_t)2 * k * n) /* [k][2][n] */, d_tmp(npoly * n);
    DevBuf<uint8_t> d_hf(npoly * n), d_hc(npoly * n);
    DevBuf<uint32_t> d_nf(npoly * 2), d_nc(npoly * 2);
    NTT_CALL(ntt_fill_uniform(d_z, o.batch, o.ps, o.seed ^ 0x3333, 0, s));
    NTT_CALL(ntt_fill_uniform(d_c, o.batch, o.ps, o.seed ^ 0x4444, 0, s));
    NTT_CALL(ntt_fill_uniform(d_at, 2 * k, o.ps, o.seed ^ 0x5555, 0, s));
    const uint32_t *ys[2] = {d_z, d_c};
    auto fused = [&]() { NTT_CALL(poly_mul_ntt_kl_round(d_hf, d_nf, ys, d_at, nullptr, o.batch, k, 2, d, o.ps, s)); };
    auto comp = [&]() {
        NTT_CALL(poly_mul_ntt_kl(d_tmp, ys, d_at, nullptr, o.batch, k, 2, o.ps, s));
        NTT_CALL(poly_round(d_hc, d_nc, d_tmp, npoly, d, o.ps, s));
    };
    const auto [f, c] = time_paths(s, o.reps, npoly * n < (1u << 24) ? 20 : 1, 3, fused, comp);
    const size_t chk = window(o.batch) * k;   // polynomials at the head and at the tail
    std::vector<uint8_t> hf(chk * n), hc(chk * n);
    std::vector<uint32_t> nf(chk * 2), nc(chk * 2);
    const bool ok = head_and_tail(o.batch, [&](size_t b0, size_t) {
        const size_t p0 = b0 * k;
        HIP_OK(hipMemcpy(hf.data(), d_hf + p0 * n, chk * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(hc.data(), d_hc + p0 * n, chk * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(nf.data(), d_nf + p0 * 2, chk * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(nc.data(), d_nc + p0 * 2, chk * 8, hipMemcpyDeviceToHost));
        return memcmp(hf.data(), hc.data(), chk * n) == 0 && memcmp(nf.data(), nc.data(), chk * 8) == 0;
    });
    banner("poly_mul_ntt_kl_round GPU. Batch Size is %zu, k = %d, l = 2, d = %d", o.batch, k, d);
    print_pair("poly_mul_ntt_kl_round        ", "poly_mul_ntt_kl + poly_round ", "composition / fused          ", f, c, o.reps,
               (double)npoly, "rows/s");
    printf("fused == poly_mul_ntt_kl + poly_round (hi and norms, first and last %zu polynomials): %s\n", chk, verdict(ok));
    return ok;
}

// -speedgpu 15: poly_round, random operands; leg (b) for n <= 2048
static int run_round(const Opts &o)
{
    const Set p = set_of(o);
    Stream s;
    bool ok = true;
    if (o.leg != 'b') run_round_alone(o, p, s);
    if (o.leg != 'a' && p.n <= 2048) ok = run_round_fused(o, p, s);
    return ok ? 0 : 1;
}

// -speedgpu 16: the two hashes round a verification, inputs from the device
// generator, all four launches timed in one time_paths.
// Leg (a): ntt_xof at qTESLA's H shape of the set -- SHAKE128 over k n + 64
// bytes for n = 1024 (p-I: 4 * 1024 + 64), SHAKE256 for n = 2048 (p-III:
// 5 * 2048 + 64), 32 bytes out -- reading the hi bytes the same round's
// poly_mul_ntt_kl_round (l = 2) has just written and a separate buffer of
// digests; time, messages/s, input GB/s of the hash, the product's time and
// the ratio of the two.
// Leg (b): poly_challenge on the 32-byte outputs of leg (a) (h = 25 for
// n = 1024, 40 for n = 2048) followed by poly_scatter, each timed.
static int run_xof(const Opts &o)
{
    const Set p = set_of(o);
    const uint32_t n = p.n;
    if (n > 2048) {
        fprintf(stderr, "-speedgpu 16: qTESLA's H shapes are defined for n = 1024 / 2048\n");
        return -1;
    }
    const int k = p.k, d = p.d, algo = p.algo, h = p.h;
    const size_t row = (size_t)n * 4, hlen = (size_t)k * n, glen = 64, outlen = 32;
    Stream s;
    // the generator fills whole polynomials: byte buffers are rounded up to n words
    auto polys = [&](size_t bytes) { return (bytes + row - 1) / row; };
    DevBuf<uint32_t> d_z(o.batch * n), d_c(o.batch * n), d_at((size_t)2 * k * n);
    DevBuf<uint32_t> d_hi(polys(o.batch * hlen) * n), d_g(polys(o.batch * glen) * n);   // hlen and glen bytes per message
    DevBuf<uint8_t> d_out(o.batch * outlen);
    DevBuf<uint32_t> d_pos(o.batch * h), d_val(o.batch * h), d_dense(o.batch * n);
    NTT_CALL(ntt_fill_uniform(d_z, o.batch, o.ps, o.seed ^ 0x6666, 0, s));
    NTT_CALL(ntt_fill_uniform(d_c, o.batch, o.ps, o.seed ^ 0x7777, 0, s));
    NTT_CALL(ntt_fill_uniform(d_at, 2 * k, o.ps, o.seed ^ 0x8888, 0, s));
    NTT_CALL(ntt_fill_uniform(d_hi, polys(o.batch * hlen), o.ps, o.seed ^ 0x9999, 0, s));
    NTT_CALL(ntt_fill_uniform(d_g, polys(o.batch * glen), o.ps, o.seed ^ 0xAAAA, 0, s));
    uint8_t *const hi = (uint8_t *)d_hi.p;
    const uint8_t *const g = (const uint8_t *)d_g.p;
    const uint32_t *ys[2] = {d_z, d_c};
    auto product = [&]() { NTT_CALL(poly_mul_ntt_kl_round(hi, nullptr, ys, d_at, nullptr, o.batch, k, 2, d, o.ps, s)); };
    auto hash = [&]() { NTT_CALL(ntt_xof(d_out, outlen, hi, hlen, g, glen, o.batch, algo, -1, s)); };
    auto chal = [&]() { NTT_CALL(poly_challenge(d_pos, d_val, d_out, outlen, o.batch, h, o.ps, s)); };
    auto scat = [&]() { NTT_CALL(poly_scatter(d_dense, d_pos, d_val, o.batch, h, o.ps, s)); };
    const int inner = o.batch <= 4096 ? 5 : 1;
    const auto [prod, xof, ch, sc] = time_paths(s, o.reps, inner, 3, product, hash, chal, scat);
    uint8_t first[32];
    HIP_OK(hipMemcpy(first, d_out, 32, hipMemcpyDeviceToHost));
    const double in_bytes = (double)o.batch * (hlen + glen);
    if (o.leg != 'b') {
        banner("ntt_xof GPU. Batch Size is %zu, %s over %zu + %zu bytes, %zu bytes out", o.batch,
               algo == NTT_XOF_SHAKE128 ? "SHAKE128" : "SHAKE256", hlen, glen, outlen);
        printf("ntt_xof                : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e messages/s, %.2f GB/s in\n",
               xof.med, xof.lo, xof.hi, o.reps, (double)o.batch / xof.med * 1e3, in_bytes / xof.med / 1e6);
        printf("poly_mul_ntt_kl_round  : median %.4f ms (min %.4f, max %.4f), k = %d, l = 2, d = %d\n", prod.med, prod.lo, prod.hi,
               k, d);
        printf("ntt_xof / product      : %.3f\n", xof.med / prod.med);
        printf("out[0]                 : ");
        for (int i = 0; i < 32; i++) printf("%02x", first[i]);
        printf("\n");
    }
    if (o.leg != 'a') {
        banner("poly_challenge GPU. Batch Size is %zu, seed 32 bytes, h = %d", o.batch, h);
        printf("poly_challenge         : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e seeds/s\n", ch.med, ch.lo,
               ch.hi, o.reps, (double)o.batch / ch.med * 1e3);
        printf("poly_scatter           : median %.4f ms (min %.4f, max %.4f)\n", sc.med, sc.lo, sc.hi);
        printf("challenge + scatter    : %.4f ms\n", ch.med + sc.med);
    }
    return 0;
}

// ---- usage and dispatch, both from this table

static const struct {
    int id;
    int (*run)(const Opts &);
} options[] = {
    {4, [](const Opts &o) { run_polymul(o, "CT-CT", false); return 0; }},
    {6, [](const Opts &o) { run_polymul(o, "CT-GS", false); return 0; }},
    {7, [](const Opts &o) { run_polymul(o, "fused", true); return 0; }},
    {8, [](const Opts &o) {
         for (int i = 0; i < 5; i++) run_polymul(o, "CT-GS", false);
         for (int i = 0; i < 5; i++) run_polymul(o, "fused", true);
         return 0;
     }},
    {9, run_fwdinv},
    {10, run_polymul_host},
    {11, run_nussbaumer},
    {12, run_latency},
    {13, run_mul_ntt_k},
    {14, run_mul_ntt_kl},
    {15, run_round},
    {16, run_xof},
};

static void help_message()
{
    printf("usage: ntt_main -speedgpu {");
    for (const auto &op : options) printf("%s%d", &op == options ? "" : ",", op.id);
    printf("} [-param ref|p-I|p-III|p-III-4096|p-III-8192] [-batch B] [-reps R] [-k K] [-d D] [-leg a|b] [-r seed] [-pcie] [-debug]\n");
}

int main(int argc, char **argv)
{
    Opts o;
    if (argc < 3) {
        help_message();
        return -1;
    }
    for (int i = 1; i < argc;) {
        std::string a = argv[i];
        auto next = [&](void) -> const char * {
            if (i + 1 >= argc) { help_message(); exit(-1); }
            return argv[i + 1];
        };
        if (a == "-speedgpu") { o.option = atoi(next()); i += 2; }
        else if (a == "-param") {
            std::string p = next();
            o.ps = p == "ref" ? NTT_PARAM_REF : p == "p-I" ? NTT_PARAM_P_I : p == "p-III" ? NTT_PARAM_P_III
                 : p == "p-III-4096" ? NTT_PARAM_N4096 : p == "p-III-8192" ? NTT_PARAM_N8192 : -1;
            i += 2;
        }
        else if (a == "-batch") { o.batch = strtoull(next(), nullptr, 10); i += 2; }
        else if (a == "-reps") { o.reps = atoi(next()); i += 2; }
        else if (a == "-k") { o.k = atoi(next()); i += 2; }
        else if (a == "-d") { o.d = atoi(next()); i += 2; }
        else if (a == "-leg") { o.leg = next()[0]; i += 2; }
        else if (a == "-r") { o.random = true; o.seed = strtoull(next(), nullptr, 0); i += 2; }
        else if (a == "-pcie") { o.pcie = true; i += 1; }
        else if (a == "-debug") { o.debug = true; i += 1; }
        else { help_message(); return -1; }
    }
    uint32_t n, q, psi;
    if (ntt_param_info(o.ps, &n, &q, &psi, nullptr, nullptr, nullptr) != NTT_OK) {
        fprintf(stderr, "unknown parameter set\n");
        return -1;
    }
    printf("NTT Parameters==> NTTSIZE: %u P: %u psi: %u batch: %zu\n", n, q, psi, o.batch);
    for (const auto &op : options)
        if (op.id == o.option) return op.run(o);
    help_message();
    return -1;
}
