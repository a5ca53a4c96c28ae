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
#include <chrono>
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

static void help_message()
{
    printf("usage: ntt_main -speedgpu {4,6,7,8,9,10,11,12,13,14,15,16} [-param ref|p-I|p-III|p-III-4096|p-III-8192] [-batch B] [-reps R] [-k K] [-d D] [-leg a|b] [-r seed] [-pcie] [-debug]\n");
}

struct Opts {
    int option = 6, ps = NTT_PARAM_REF, reps = 1, k = 0, d = 0;
    char leg = 0;   // -speedgpu 15 / 16: 'a' / 'b' for one leg, 0 for both
    size_t batch = 2;
    bool random = false, pcie = false, debug = false;
    uint64_t seed = 0;
};

// Negacyclic poly-mul driver: inputs x, y (all ones or random), output z.
static double run_polymul(const Opts &o, bool fused, std::vector<uint32_t> &z, int *kat_ok)
{
    uint32_t n, q;
    NTT_CALL(ntt_param_info(o.ps, &n, &q, nullptr, nullptr, nullptr, nullptr));
    const size_t count = o.batch * n, bytes = count * 4;
    std::vector<uint32_t> x(count, 1), y(count, 1);
    uint32_t *d_x, *d_y, *d_z;
    HIP_OK(hipMalloc(&d_x, bytes));
    HIP_OK(hipMalloc(&d_y, bytes));
    HIP_OK(hipMalloc(&d_z, bytes));
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
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
    z.assign(count, 0);
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
    if (!o.pcie) HIP_OK(hipMemcpy(z.data(), d_z, bytes, hipMemcpyDeviceToHost));
    *kat_ok = -1;
    if (!o.random) {
        *kat_ok = 1;
        for (size_t b = 0; b < o.batch && *kat_ok; b++)
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t want = (uint32_t)((2ull * k + 2 + q - n) % q);
                if (z[b * n + k] != want) { *kat_ok = 0; break; }
            }
    }
    HIP_OK(hipFree(d_x));
    HIP_OK(hipFree(d_y));
    HIP_OK(hipFree(d_z));
    HIP_OK(hipStreamDestroy(s));
    return ms / o.reps;
}

static double run_fwdinv(const Opts &o, int *roundtrip_ok)
{
    uint32_t n;
    NTT_CALL(ntt_param_info(o.ps, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    const size_t bytes = o.batch * n * 4;
    uint32_t *d_x, *d_ref;
    HIP_OK(hipMalloc(&d_x, bytes));
    HIP_OK(hipMalloc(&d_ref, bytes));
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    NTT_CALL(ntt_fill_uniform(d_x, o.batch, o.ps, o.seed, 0, s));
    HIP_OK(hipMemcpyAsync(d_ref, d_x, bytes, hipMemcpyDeviceToDevice, s));
    NTT_CALL(poly_ntt(d_x, nullptr, o.batch, o.ps, s));
    NTT_CALL(poly_invntt(d_x, nullptr, o.batch, o.ps, s));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipEventRecord(e0, s));
    for (int r = 0; r < o.reps; r++) {
        NTT_CALL(poly_ntt(d_x, nullptr, o.batch, o.ps, s));
        NTT_CALL(poly_invntt(d_x, nullptr, o.batch, o.ps, s));
    }
    HIP_OK(hipEventRecord(e1, s));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<uint32_t> a(o.batch * n), b(o.batch * n);
    HIP_OK(hipMemcpy(a.data(), d_x, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b.data(), d_ref, bytes, hipMemcpyDeviceToHost));
    *roundtrip_ok = (a == b);
    HIP_OK(hipFree(d_x));
    HIP_OK(hipFree(d_ref));
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipStreamDestroy(s));
    return ms / o.reps;
}

// host -> host fused product through ntt_host_ctx; all-ones (KAT) or random operands
static double run_polymul_host(const Opts &o, int *kat_ok)
{
    uint32_t n, q;
    NTT_CALL(ntt_param_info(o.ps, &n, &q, nullptr, nullptr, nullptr, nullptr));
    const size_t count = o.batch * n, bytes = count * 4;
    uint32_t *x = (uint32_t *)ntt_host_alloc(bytes), *y = (uint32_t *)ntt_host_alloc(bytes),
             *z = (uint32_t *)ntt_host_alloc(bytes);
    if (!x || !y || !z) { fprintf(stderr, "ntt_host_alloc failed\n"); exit(2); }
    for (size_t i = 0; i < count; i++) x[i] = y[i] = 1;
    if (o.random) {
        uint32_t *d;
        HIP_OK(hipMalloc(&d, bytes));
        NTT_CALL(ntt_fill_uniform(d, o.batch, o.ps, o.seed, 0, nullptr));
        HIP_OK(hipMemcpy(x, d, bytes, hipMemcpyDeviceToHost));
        NTT_CALL(ntt_fill_uniform(d, o.batch, o.ps, o.seed ^ 0xFFFF, 0, nullptr));
        HIP_OK(hipMemcpy(y, d, bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d));
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
    *kat_ok = -1;
    if (!o.random) {
        *kat_ok = 1;
        for (size_t b = 0; b < o.batch && *kat_ok; b++)
            for (uint32_t k = 0; k < n; k++)
                if (z[b * n + k] != (uint32_t)((2ull * k + 2 + q - n) % q)) { *kat_ok = 0; break; }
    }
    NTT_CALL(ntt_host_ctx_destroy(ctx));
    ntt_host_free(x);
    ntt_host_free(y);
    ntt_host_free(z);
    return ms / o.reps;
}

// Nussbaumer mod 2^32-1 on the GPU, all-ones operands: z[k] = 2k + 2 - n mod 2^32-1
static double run_nussbaumer(const Opts &o, int *kat_ok)
{
    uint32_t n;
    NTT_CALL(ntt_param_info(o.ps, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    const size_t count = o.batch * n, bytes = count * 4;
    std::vector<uint32_t> x(count, 1), z(count, 0);
    uint32_t *d_x, *d_z;
    HIP_OK(hipMalloc(&d_x, bytes));
    HIP_OK(hipMalloc(&d_z, bytes));
    HIP_OK(hipMemcpy(d_x, x.data(), bytes, hipMemcpyHostToDevice));
    NTT_CALL(poly_mul_nussbaumer(d_z, d_x, d_x, o.batch, o.ps, NTT_RING_M32, nullptr));
    HIP_OK(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < o.reps; r++) NTT_CALL(poly_mul_nussbaumer(d_z, d_x, d_x, o.batch, o.ps, NTT_RING_M32, nullptr));
    HIP_OK(hipDeviceSynchronize());
    auto t1 = std::chrono::steady_clock::now();
    HIP_OK(hipMemcpy(z.data(), d_z, bytes, hipMemcpyDeviceToHost));
    *kat_ok = 1;
    const uint64_t m = 0xFFFFFFFFull;
    for (size_t b = 0; b < o.batch && *kat_ok; b++)
        for (uint32_t k = 0; k < n; k++)
            if (z[b * n + k] != (uint32_t)((2ull * k + 2 + m - n) % m)) { *kat_ok = 0; break; }
    HIP_OK(hipFree(d_x));
    HIP_OK(hipFree(d_z));
    return std::chrono::duration<double, std::milli>(t1 - t0).count() / o.reps;
}

static void report_polymul(const Opts &o, const char *name, bool fused)
{
    std::vector<uint32_t> z;
    int kat = -1;
    const double ms = run_polymul(o, fused, z, &kat);
    printf("\n========================\n");
    printf("test_NTT_negacyclic %s GPU. Batch Size is %zu", name, o.batch);
    printf("\n========================\n");
    printf("Performance GPU %s GPU \n Time\t\t: % .4f ms. \nThroughput\t: %.2f Multiplications per second\n", name, ms,
           (double)o.batch / ms * 1000.0);
    if (kat >= 0) printf("all-ones KAT z[k] = 2k+2-n mod q: %s\n", kat ? "Identical." : "Incorrect result.");
    if (o.debug) {
        uint32_t n;
        ntt_param_info(o.ps, &n, nullptr, nullptr, nullptr, nullptr, nullptr);
        printf("z: ");
        for (uint32_t i = 0; i < 8 && i < n; i++) printf("%u ", z[i]);
        printf("... %u\n", z[n - 1]);
    }
}

// -speedgpu 12: per-call latency of the small-batch entry points.
static int run_latency(const Opts &o)
{
    uint32_t n;
    NTT_CALL(ntt_param_info(o.ps, &n, nullptr, nullptr, nullptr, nullptr, nullptr));
    const size_t bytes = o.batch * n * 4;
    uint32_t *d_x, *d_y, *d_z;
    HIP_OK(hipMalloc(&d_x, bytes));
    HIP_OK(hipMalloc(&d_y, bytes));
    HIP_OK(hipMalloc(&d_z, bytes));
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    NTT_CALL(ntt_fill_uniform(d_x, o.batch, o.ps, 1, 0, s));
    NTT_CALL(ntt_fill_uniform(d_y, o.batch, o.ps, 2, 0, s));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
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
        HIP_OK(hipEventRecord(e0, s));
        for (int i = 0; i < calls; i++) NTT_CALL(c.fn(d_x, d_y, d_z, o.batch, o.ps, s));
        HIP_OK(hipEventRecord(e1, s));
        HIP_OK(hipEventSynchronize(e1));
        auto t1 = std::chrono::steady_clock::now();
        float gpu_ms = 0.f;
        HIP_OK(hipEventElapsedTime(&gpu_ms, e0, e1));
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
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipStreamDestroy(s));
    HIP_OK(hipFree(d_x));
    HIP_OK(hipFree(d_y));
    HIP_OK(hipFree(d_z));
    return 0;
}

// -speedgpu 13: out[b][i] = a_i * y_b for k shared NTT-domain rows, (a) one
// poly_mul_ntt_k launch, (b) the baseline it replaces: k back-to-back
// poly_mul_ntt launches over a materialised [k][batch][n] broadcast of the
// rows.  Both timed per rep with HIP events on one stream, alternating.
// All-ones operands: every row is the KAT z[k] = 2k + 2 - n mod q; -r:
// random operands, the two paths must agree.  The first and last (up to) 256
// polynomials are checked.
static int run_mul_ntt_k(const Opts &o)
{
    uint32_t n, q;
    NTT_CALL(ntt_param_info(o.ps, &n, &q, nullptr, nullptr, nullptr, nullptr));
    const int k = o.k > 0 ? o.k : o.ps == NTT_PARAM_REF ? 1 : o.ps == NTT_PARAM_P_I ? 4 : 5;
    const size_t row = (size_t)n * 4, pbytes = o.batch * row;
    uint32_t *d_y, *d_ahat, *d_out, *d_bc, *d_c;
    HIP_OK(hipMalloc(&d_y, pbytes));
    HIP_OK(hipMalloc(&d_ahat, k * row));
    HIP_OK(hipMalloc(&d_out, k * pbytes));
    HIP_OK(hipMalloc(&d_bc, k * pbytes));   // baseline operand [k][batch][n]
    HIP_OK(hipMalloc(&d_c, k * pbytes));    // baseline result  [k][batch][n]
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    // dst[0 .. count) = the n-word row at src, by doubling device copies
    auto bcast = [&](uint32_t *dst, const uint32_t *src, size_t count) {
        if (dst != src) HIP_OK(hipMemcpyAsync(dst, src, row, hipMemcpyDeviceToDevice, s));
        for (size_t have = 1; have < count; have *= 2) {
            const size_t cnt = have < count - have ? have : count - have;
            HIP_OK(hipMemcpyAsync(dst + have * n, dst, cnt * row, hipMemcpyDeviceToDevice, s));
        }
    };
    if (o.random) {
        NTT_CALL(ntt_fill_uniform(d_y, o.batch, o.ps, o.seed, 0, s));
        NTT_CALL(ntt_fill_uniform(d_ahat, k, o.ps, o.seed ^ 0xFFFF, 0, s));
    } else {
        const std::vector<uint32_t> ones(n, 1);
        HIP_OK(hipMemcpy(d_y, ones.data(), row, hipMemcpyHostToDevice));
        bcast(d_y, d_y, o.batch);
        bcast(d_ahat, d_y, k);
    }
    NTT_CALL(poly_ntt(d_ahat, nullptr, k, o.ps, s));
    for (int i = 0; i < k; i++) bcast(d_bc + (size_t)i * o.batch * n, d_ahat + (size_t)i * n, o.batch);
    auto fused = [&]() { NTT_CALL(poly_mul_ntt_k(d_out, d_y, d_ahat, nullptr, o.batch, k, o.ps, s)); };
    auto base = [&]() {
        for (int i = 0; i < k; i++)
            NTT_CALL(poly_mul_ntt(d_c + (size_t)i * o.batch * n, d_y, d_bc + (size_t)i * o.batch * n, o.batch, o.ps, s));
    };
    for (int w = 0; w < 3; w++) { fused(); base(); }
    HIP_OK(hipStreamSynchronize(s));
    hipEvent_t e0, e1, e2;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipEventCreate(&e2));
    // small batches: `inner` launches per timed rep (event resolution)
    const int inner = o.batch * k * n < (1u << 24) ? 20 : 1;
    std::vector<double> tf, tb;
    for (int r = 0; r < o.reps; r++) {
        HIP_OK(hipEventRecord(e0, s));
        for (int t = 0; t < inner; t++) fused();
        HIP_OK(hipEventRecord(e1, s));
        for (int t = 0; t < inner; t++) base();
        HIP_OK(hipEventRecord(e2, s));
        HIP_OK(hipEventSynchronize(e2));
        float a = 0.f, b = 0.f;
        HIP_OK(hipEventElapsedTime(&a, e0, e1));
        HIP_OK(hipEventElapsedTime(&b, e1, e2));
        tf.push_back(a / inner);
        tb.push_back(b / inner);
    }
    auto stats = [](std::vector<double> v, double *lo, double *hi) {
        std::sort(v.begin(), v.end());
        *lo = v.front();
        *hi = v.back();
        return v[v.size() / 2];
    };
    double flo, fhi, blo, bhi;
    const double fm = stats(tf, &flo, &fhi), bm = stats(tb, &blo, &bhi);
    // check the head and the tail of the batch
    const size_t chk = o.batch < 256 ? o.batch : 256;
    int ok = 1;
    std::vector<uint32_t> z(k * (size_t)n), c(n);
    for (int part = 0; part < 2 && ok; part++) {
        for (size_t t = 0; t < chk && ok; t++) {
            const size_t b = part ? o.batch - 1 - t : t;
            HIP_OK(hipMemcpy(z.data(), d_out + b * k * n, k * row, hipMemcpyDeviceToHost));
            for (int i = 0; i < k && ok; i++) {
                if (o.random) {
                    HIP_OK(hipMemcpy(c.data(), d_c + ((size_t)i * o.batch + b) * n, row, hipMemcpyDeviceToHost));
                    ok = memcmp(c.data(), z.data() + (size_t)i * n, row) == 0;
                } else {
                    for (uint32_t j = 0; j < n; j++)
                        if (z[(size_t)i * n + j] != (uint32_t)((2ull * j + 2 + q - n) % q)) { ok = 0; break; }
                }
            }
        }
    }
    printf("\n========================\npoly_mul_ntt_k GPU. Batch Size is %zu, k = %d\n========================\n", o.batch, k);
    printf("poly_mul_ntt_k      : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e products/s\n", fm, flo,
           fhi, o.reps, (double)o.batch * k / fm * 1e3);
    printf("%d x poly_mul_ntt    : median %.4f ms (min %.4f, max %.4f), %.3e products/s\n", k, bm, blo, bhi,
           (double)o.batch * k / bm * 1e3);
    printf("baseline / fused    : %.3f\n", bm / fm);
    printf("%s: %s\n", o.random ? "fused == k x poly_mul_ntt" : "all-ones KAT z[k] = 2k+2-n mod q, every row",
           ok ? "Identical." : "Incorrect result.");
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipEventDestroy(e2));
    HIP_OK(hipStreamDestroy(s));
    HIP_OK(hipFree(d_y));
    HIP_OK(hipFree(d_ahat));
    HIP_OK(hipFree(d_out));
    HIP_OK(hipFree(d_bc));
    HIP_OK(hipFree(d_c));
    return ok ? 0 : 1;
}

// -speedgpu 14: out[b][i] = a_i * z_b + t'_i * c_b for k rows of two shared
// NTT-domain polynomials (verification: t'_i-hat = q - t_i-hat), (a) one
// poly_mul_ntt_kl launch, (b) the composition it replaces: poly_mul_ntt_k of
// c over the rows t'_i, then poly_mul_ntt_k of z over the rows a_i with the
// first result as addend, in place.  -speedgpu 13's protocol: both timed per
// rep with HIP events on one stream, alternating.  All-ones operands: every
// row is twice the KAT, z[k] = 2 (2k + 2 - n) mod q; -r: random operands, the
// two paths must agree.  The first and last (up to) 256 polynomials are
// checked.
static int run_mul_ntt_kl(const Opts &o)
{
    uint32_t n, q;
    NTT_CALL(ntt_param_info(o.ps, &n, &q, nullptr, nullptr, nullptr, nullptr));
    const int k = o.k > 0 ? o.k : o.ps == NTT_PARAM_REF ? 1 : o.ps == NTT_PARAM_P_I ? 4 : 5;
    const size_t row = (size_t)n * 4, pbytes = o.batch * row;
    uint32_t *d_z, *d_c, *d_a, *d_t, *d_at, *d_out, *d_base;
    HIP_OK(hipMalloc(&d_z, pbytes));
    HIP_OK(hipMalloc(&d_c, pbytes));
    HIP_OK(hipMalloc(&d_a, k * row));        // [k][n]    a_i-hat
    HIP_OK(hipMalloc(&d_t, k * row));        // [k][n]    t'_i-hat
    HIP_OK(hipMalloc(&d_at, 2 * k * row));   // [k][2][n] both, the fused launch's rows
    HIP_OK(hipMalloc(&d_out, k * pbytes));
    HIP_OK(hipMalloc(&d_base, k * pbytes));
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    // dst[0 .. count) = the n-word row at src, by doubling device copies
    auto bcast = [&](uint32_t *dst, const uint32_t *src, size_t count) {
        if (dst != src) HIP_OK(hipMemcpyAsync(dst, src, row, hipMemcpyDeviceToDevice, s));
        for (size_t have = 1; have < count; have *= 2) {
            const size_t cnt = have < count - have ? have : count - have;
            HIP_OK(hipMemcpyAsync(dst + have * n, dst, cnt * row, hipMemcpyDeviceToDevice, s));
        }
    };
    if (o.random) {
        NTT_CALL(ntt_fill_uniform(d_z, o.batch, o.ps, o.seed, 0, s));
        NTT_CALL(ntt_fill_uniform(d_c, o.batch, o.ps, o.seed ^ 0xCCCC, 0, s));
        NTT_CALL(ntt_fill_uniform(d_a, k, o.ps, o.seed ^ 0xFFFF, 0, s));
        NTT_CALL(ntt_fill_uniform(d_t, k, o.ps, o.seed ^ 0xEEEE, 0, s));
    } else {
        const std::vector<uint32_t> ones(n, 1);
        HIP_OK(hipMemcpy(d_z, ones.data(), row, hipMemcpyHostToDevice));
        bcast(d_z, d_z, o.batch);
        bcast(d_c, d_z, o.batch);
        bcast(d_a, d_z, k);
        bcast(d_t, d_z, k);
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
    for (int w = 0; w < 3; w++) { fused(); base(); }
    HIP_OK(hipStreamSynchronize(s));
    hipEvent_t e0, e1, e2;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipEventCreate(&e2));
    // small batches: `inner` launches per timed rep (event resolution)
    const int inner = o.batch * k * n < (1u << 24) ? 20 : 1;
    std::vector<double> tf, tb;
    for (int r = 0; r < o.reps; r++) {
        HIP_OK(hipEventRecord(e0, s));
        for (int t = 0; t < inner; t++) fused();
        HIP_OK(hipEventRecord(e1, s));
        for (int t = 0; t < inner; t++) base();
        HIP_OK(hipEventRecord(e2, s));
        HIP_OK(hipEventSynchronize(e2));
        float a = 0.f, b = 0.f;
        HIP_OK(hipEventElapsedTime(&a, e0, e1));
        HIP_OK(hipEventElapsedTime(&b, e1, e2));
        tf.push_back(a / inner);
        tb.push_back(b / inner);
    }
    auto stats = [](std::vector<double> v, double *lo, double *hi) {
        std::sort(v.begin(), v.end());
        *lo = v.front();
        *hi = v.back();
        return v[v.size() / 2];
    };
    double flo, fhi, blo, bhi;
    const double fm = stats(tf, &flo, &fhi), bm = stats(tb, &blo, &bhi);
    // check the head and the tail of the batch
    const size_t chk = o.batch < 256 ? o.batch : 256;
    int ok = 1;
    std::vector<uint32_t> z(k * (size_t)n), c(k * (size_t)n);
    for (int part = 0; part < 2 && ok; part++) {
        for (size_t t = 0; t < chk && ok; t++) {
            const size_t b = part ? o.batch - 1 - t : t;
            HIP_OK(hipMemcpy(z.data(), d_out + b * k * n, k * row, hipMemcpyDeviceToHost));
            if (o.random) {
                HIP_OK(hipMemcpy(c.data(), d_base + b * k * n, k * row, hipMemcpyDeviceToHost));
                ok = memcmp(c.data(), z.data(), k * row) == 0;
            } else {
                for (size_t j = 0; j < (size_t)k * n && ok; j++)
                    ok = z[j] == (uint32_t)(2 * ((2ull * (j % n) + 2 + q - n) % q) % q);
            }
        }
    }
    printf("\n========================\npoly_mul_ntt_kl GPU. Batch Size is %zu, k = %d, l = 2\n========================\n", o.batch, k);
    printf("poly_mul_ntt_kl     : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e rows/s\n", fm, flo, fhi,
           o.reps, (double)o.batch * k / fm * 1e3);
    printf("2 x poly_mul_ntt_k  : median %.4f ms (min %.4f, max %.4f), %.3e rows/s\n", bm, blo, bhi,
           (double)o.batch * k / bm * 1e3);
    printf("baseline / fused    : %.3f\n", bm / fm);
    printf("%s: %s\n", o.random ? "fused == 2 x poly_mul_ntt_k" : "all-ones KAT z[k] = 2 (2k+2-n) mod q, every row",
           ok ? "Identical." : "Incorrect result.");
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipEventDestroy(e2));
    HIP_OK(hipStreamDestroy(s));
    HIP_OK(hipFree(d_z));
    HIP_OK(hipFree(d_c));
    HIP_OK(hipFree(d_a));
    HIP_OK(hipFree(d_t));
    HIP_OK(hipFree(d_at));
    HIP_OK(hipFree(d_out));
    HIP_OK(hipFree(d_base));
    return ok ? 0 : 1;
}

// -speedgpu 15: poly_round.  -speedgpu 13's protocol throughout: random
// operands, the paths of a leg timed per rep with HIP events on one stream,
// alternating, after a warm-up; median with (min - max).
// Leg (a): poly_round alone over `batch` polynomials -- both outputs, hi only,
// norms only -- and poly_pointwise (12 B per coefficient) over the same
// coefficients; time and achieved bytes/s of each.
// Leg (b), n <= 2048: poly_mul_ntt_kl_round (l = 2) against poly_mul_ntt_kl
// into a temporary followed by poly_round over batch * k polynomials; the
// outputs of the two paths are compared on the first and last 256 polynomials.
static int run_round(const Opts &o)
{
    uint32_t n, q;
    NTT_CALL(ntt_param_info(o.ps, &n, &q, nullptr, nullptr, nullptr, nullptr));
    const int d = o.d > 0 ? o.d : o.ps <= NTT_PARAM_P_I ? 22 : 24;
    const size_t row = (size_t)n * 4;
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    hipEvent_t ev[5];
    for (auto &e : ev) HIP_OK(hipEventCreate(&e));
    auto stats = [](std::vector<double> v, double *lo, double *hi) {
        std::sort(v.begin(), v.end());
        *lo = v.front();
        *hi = v.back();
        return v[v.size() / 2];
    };
    int ok = 1;
    if (o.leg != 'b') {
        const size_t coeffs = o.batch * n;
        uint32_t *d_w, *d_b, *d_c, *d_norms;
        uint8_t *d_hi;
        HIP_OK(hipMalloc(&d_w, coeffs * 4));
        HIP_OK(hipMalloc(&d_b, coeffs * 4));
        HIP_OK(hipMalloc(&d_c, coeffs * 4));
        HIP_OK(hipMalloc(&d_hi, coeffs));
        HIP_OK(hipMalloc(&d_norms, o.batch * 8));
        NTT_CALL(ntt_fill_uniform(d_w, o.batch, o.ps, o.seed ^ 0x1111, 0, s));
        NTT_CALL(ntt_fill_uniform(d_b, o.batch, o.ps, o.seed ^ 0x2222, 0, s));
        auto path = [&](int which) {
            switch (which) {
            case 0: NTT_CALL(poly_round(d_hi, d_norms, d_w, o.batch, d, o.ps, s)); break;
            case 1: NTT_CALL(poly_round(d_hi, nullptr, d_w, o.batch, d, o.ps, s)); break;
            case 2: NTT_CALL(poly_round(nullptr, d_norms, d_w, o.batch, d, o.ps, s)); break;
            default: NTT_CALL(poly_pointwise(d_c, d_w, d_b, o.batch, o.ps, s)); break;
            }
        };
        for (int w = 0; w < 3; w++)
            for (int p = 0; p < 4; p++) path(p);
        HIP_OK(hipStreamSynchronize(s));
        const int inner = coeffs < (1u << 24) ? 20 : 1;   // small batches: launches per timed rep (event resolution)
        std::vector<double> t[4];
        for (int r = 0; r < o.reps; r++) {
            HIP_OK(hipEventRecord(ev[0], s));
            for (int p = 0; p < 4; p++) {
                for (int i = 0; i < inner; i++) path(p);
                HIP_OK(hipEventRecord(ev[p + 1], s));
            }
            HIP_OK(hipEventSynchronize(ev[4]));
            for (int p = 0; p < 4; p++) {
                float ms = 0.f;
                HIP_OK(hipEventElapsedTime(&ms, ev[p], ev[p + 1]));
                t[p].push_back(ms / inner);
            }
        }
        const char *name[4] = {"poly_round hi+norms", "poly_round hi      ", "poly_round norms   ", "poly_pointwise     "};
        const double bytes[4] = {5.0 * coeffs + 8.0 * o.batch, 5.0 * coeffs, 4.0 * coeffs + 8.0 * o.batch, 12.0 * coeffs};
        printf("\n========================\npoly_round GPU. Batch Size is %zu, d = %d\n========================\n", o.batch, d);
        for (int p = 0; p < 4; p++) {
            double lo, hi;
            const double m = stats(t[p], &lo, &hi);
            printf("%s : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.4e bytes, %.3f TB/s\n", name[p], m, lo,
                   hi, o.reps, bytes[p], bytes[p] / m / 1e9);
        }
        HIP_OK(hipFree(d_w));
        HIP_OK(hipFree(d_b));
        HIP_OK(hipFree(d_c));
        HIP_OK(hipFree(d_hi));
        HIP_OK(hipFree(d_norms));
    }
    if (o.leg != 'a' && n <= 2048) {
        const int k = o.k > 0 ? o.k : o.ps == NTT_PARAM_REF ? 1 : o.ps == NTT_PARAM_P_I ? 4 : 5;
        const size_t npoly = o.batch * k;
        uint32_t *d_z, *d_c, *d_at, *d_tmp, *d_nf, *d_nc;
        uint8_t *d_hf, *d_hc;
        HIP_OK(hipMalloc(&d_z, o.batch * row));
        HIP_OK(hipMalloc(&d_c, o.batch * row));
        HIP_OK(hipMalloc(&d_at, 2 * k * row));   // [k][2][n]
        HIP_OK(hipMalloc(&d_tmp, npoly * row));
        HIP_OK(hipMalloc(&d_hf, npoly * n));
        HIP_OK(hipMalloc(&d_hc, npoly * n));
        HIP_OK(hipMalloc(&d_nf, npoly * 8));
        HIP_OK(hipMalloc(&d_nc, npoly * 8));
        NTT_CALL(ntt_fill_uniform(d_z, o.batch, o.ps, o.seed ^ 0x3333, 0, s));
        NTT_CALL(ntt_fill_uniform(d_c, o.batch, o.ps, o.seed ^ 0x4444, 0, s));
        NTT_CALL(ntt_fill_uniform(d_at, 2 * k, o.ps, o.seed ^ 0x5555, 0, s));
        const uint32_t *ys[2] = {d_z, d_c};
        auto fused = [&]() { NTT_CALL(poly_mul_ntt_kl_round(d_hf, d_nf, ys, d_at, nullptr, o.batch, k, 2, d, o.ps, s)); };
        auto comp = [&]() {
            NTT_CALL(poly_mul_ntt_kl(d_tmp, ys, d_at, nullptr, o.batch, k, 2, o.ps, s));
            NTT_CALL(poly_round(d_hc, d_nc, d_tmp, npoly, d, o.ps, s));
        };
        for (int w = 0; w < 3; w++) { fused(); comp(); }
        HIP_OK(hipStreamSynchronize(s));
        const int inner = npoly * n < (1u << 24) ? 20 : 1;
        std::vector<double> tf, tc;
        for (int r = 0; r < o.reps; r++) {
            HIP_OK(hipEventRecord(ev[0], s));
            for (int i = 0; i < inner; i++) fused();
            HIP_OK(hipEventRecord(ev[1], s));
            for (int i = 0; i < inner; i++) comp();
            HIP_OK(hipEventRecord(ev[2], s));
            HIP_OK(hipEventSynchronize(ev[2]));
            float a = 0.f, b = 0.f;
            HIP_OK(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_OK(hipEventElapsedTime(&b, ev[1], ev[2]));
            tf.push_back(a / inner);
            tc.push_back(b / inner);
        }
        double flo, fhi, clo, chi;
        const double fm = stats(tf, &flo, &fhi), cm = stats(tc, &clo, &chi);
        const size_t chk = (o.batch < 256 ? o.batch : 256) * k;   // polynomials at the head and at the tail
        std::vector<uint8_t> hf(chk * n), hc(chk * n);
        std::vector<uint32_t> nf(chk * 2), nc(chk * 2);
        for (int part = 0; part < 2 && ok; part++) {
            const size_t p0 = part ? npoly - chk : 0;
            HIP_OK(hipMemcpy(hf.data(), d_hf + p0 * n, chk * n, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(hc.data(), d_hc + p0 * n, chk * n, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(nf.data(), d_nf + p0 * 2, chk * 8, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(nc.data(), d_nc + p0 * 2, chk * 8, hipMemcpyDeviceToHost));
            ok = memcmp(hf.data(), hc.data(), chk * n) == 0 && memcmp(nf.data(), nc.data(), chk * 8) == 0;
        }
        printf("\n========================\npoly_mul_ntt_kl_round GPU. Batch Size is %zu, k = %d, l = 2, d = %d\n========================\n",
               o.batch, k, d);
        printf("poly_mul_ntt_kl_round        : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e rows/s\n", fm,
               flo, fhi, o.reps, (double)npoly / fm * 1e3);
        printf("poly_mul_ntt_kl + poly_round : median %.4f ms (min %.4f, max %.4f), %.3e rows/s\n", cm, clo, chi,
               (double)npoly / cm * 1e3);
        printf("composition / fused          : %.3f\n", cm / fm);
        printf("fused == poly_mul_ntt_kl + poly_round (hi and norms, first and last %zu polynomials): %s\n", chk,
               ok ? "Identical." : "Incorrect result.");
        HIP_OK(hipFree(d_z));
        HIP_OK(hipFree(d_c));
        HIP_OK(hipFree(d_at));
        HIP_OK(hipFree(d_tmp));
        HIP_OK(hipFree(d_hf));
        HIP_OK(hipFree(d_hc));
        HIP_OK(hipFree(d_nf));
        HIP_OK(hipFree(d_nc));
    }
    for (auto &e : ev) HIP_OK(hipEventDestroy(e));
    HIP_OK(hipStreamDestroy(s));
    return ok ? 0 : 1;
}

// -speedgpu 16: the two hashes round a verification.  -speedgpu 15's protocol:
// inputs from the device generator, HIP events on one stream, 3 warm-up
// rounds, median with (min - max) over the repetitions.
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
    uint32_t n, q;
    NTT_CALL(ntt_param_info(o.ps, &n, &q, nullptr, nullptr, nullptr, nullptr));
    if (n > 2048) {
        fprintf(stderr, "-speedgpu 16: qTESLA's H shapes are defined for n = 1024 / 2048\n");
        return -1;
    }
    const int k = o.k > 0 ? o.k : o.ps == NTT_PARAM_REF ? 1 : o.ps == NTT_PARAM_P_I ? 4 : 5;
    const int d = o.d > 0 ? o.d : o.ps <= NTT_PARAM_P_I ? 22 : 24;
    const int algo = n == 1024 ? NTT_XOF_SHAKE128 : NTT_XOF_SHAKE256, h = n == 1024 ? 25 : 40;
    const size_t row = (size_t)n * 4, hlen = (size_t)k * n, glen = 64, outlen = 32;
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    hipEvent_t ev[5];
    for (auto &e : ev) HIP_OK(hipEventCreate(&e));
    auto stats = [](std::vector<double> v, double *lo, double *hi) {
        std::sort(v.begin(), v.end());
        *lo = v.front();
        *hi = v.back();
        return v[v.size() / 2];
    };
    // the generator fills whole polynomials: byte buffers are rounded up to n words
    auto polys = [&](size_t bytes) { return (bytes + row - 1) / row; };
    uint32_t *d_z, *d_c, *d_at, *d_g, *d_pos, *d_val, *d_dense;
    uint8_t *d_hi, *d_out;
    HIP_OK(hipMalloc(&d_z, o.batch * row));
    HIP_OK(hipMalloc(&d_c, o.batch * row));
    HIP_OK(hipMalloc(&d_at, 2 * k * row));
    HIP_OK(hipMalloc(&d_hi, polys(o.batch * hlen) * row));
    HIP_OK(hipMalloc(&d_g, polys(o.batch * glen) * row));
    HIP_OK(hipMalloc(&d_out, o.batch * outlen));
    HIP_OK(hipMalloc(&d_pos, o.batch * h * 4));
    HIP_OK(hipMalloc(&d_val, o.batch * h * 4));
    HIP_OK(hipMalloc(&d_dense, o.batch * row));
    NTT_CALL(ntt_fill_uniform(d_z, o.batch, o.ps, o.seed ^ 0x6666, 0, s));
    NTT_CALL(ntt_fill_uniform(d_c, o.batch, o.ps, o.seed ^ 0x7777, 0, s));
    NTT_CALL(ntt_fill_uniform(d_at, 2 * k, o.ps, o.seed ^ 0x8888, 0, s));
    NTT_CALL(ntt_fill_uniform((uint32_t *)d_hi, polys(o.batch * hlen), o.ps, o.seed ^ 0x9999, 0, s));
    NTT_CALL(ntt_fill_uniform(d_g, polys(o.batch * glen), o.ps, o.seed ^ 0xAAAA, 0, s));
    const uint32_t *ys[2] = {d_z, d_c};
    auto product = [&]() { NTT_CALL(poly_mul_ntt_kl_round(d_hi, nullptr, ys, d_at, nullptr, o.batch, k, 2, d, o.ps, s)); };
    auto hash = [&]() { NTT_CALL(ntt_xof(d_out, outlen, d_hi, hlen, (const uint8_t *)d_g, glen, o.batch, algo, -1, s)); };
    auto chal = [&]() { NTT_CALL(poly_challenge(d_pos, d_val, d_out, outlen, o.batch, h, o.ps, s)); };
    auto scat = [&]() { NTT_CALL(poly_scatter(d_dense, d_pos, d_val, o.batch, h, o.ps, s)); };
    for (int w = 0; w < 3; w++) { product(); hash(); chal(); scat(); }
    HIP_OK(hipStreamSynchronize(s));
    const int inner = o.batch <= 4096 ? 5 : 1;   // small batches: launches per timed rep (event resolution)
    std::vector<double> t[4];
    for (int r = 0; r < o.reps; r++) {
        HIP_OK(hipEventRecord(ev[0], s));
        for (int i = 0; i < inner; i++) product();
        HIP_OK(hipEventRecord(ev[1], s));
        for (int i = 0; i < inner; i++) hash();
        HIP_OK(hipEventRecord(ev[2], s));
        for (int i = 0; i < inner; i++) chal();
        HIP_OK(hipEventRecord(ev[3], s));
        for (int i = 0; i < inner; i++) scat();
        HIP_OK(hipEventRecord(ev[4], s));
        HIP_OK(hipEventSynchronize(ev[4]));
        for (int p = 0; p < 4; p++) {
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ev[p], ev[p + 1]));
            t[p].push_back(ms / inner);
        }
    }
    double lo[4], hi[4], m[4];
    for (int p = 0; p < 4; p++) m[p] = stats(t[p], &lo[p], &hi[p]);
    uint8_t first[32];
    HIP_OK(hipMemcpy(first, d_out, 32, hipMemcpyDeviceToHost));
    const double in_bytes = (double)o.batch * (hlen + glen);
    if (o.leg != 'b') {
        printf("\n========================\nntt_xof GPU. Batch Size is %zu, %s over %zu + %zu bytes, %zu bytes out\n========================\n",
               o.batch, algo == NTT_XOF_SHAKE128 ? "SHAKE128" : "SHAKE256", hlen, glen, outlen);
        printf("ntt_xof                : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e messages/s, %.2f GB/s in\n",
               m[1], lo[1], hi[1], o.reps, (double)o.batch / m[1] * 1e3, in_bytes / m[1] / 1e6);
        printf("poly_mul_ntt_kl_round  : median %.4f ms (min %.4f, max %.4f), k = %d, l = 2, d = %d\n", m[0], lo[0], hi[0], k, d);
        printf("ntt_xof / product      : %.3f\n", m[1] / m[0]);
        printf("out[0]                 : ");
        for (int i = 0; i < 32; i++) printf("%02x", first[i]);
        printf("\n");
    }
    if (o.leg != 'a') {
        printf("\n========================\npoly_challenge GPU. Batch Size is %zu, seed 32 bytes, h = %d\n========================\n",
               o.batch, h);
        printf("poly_challenge         : median %.4f ms (min %.4f, max %.4f over %d reps) per launch, %.3e seeds/s\n", m[2], lo[2],
               hi[2], o.reps, (double)o.batch / m[2] * 1e3);
        printf("poly_scatter           : median %.4f ms (min %.4f, max %.4f)\n", m[3], lo[3], hi[3]);
        printf("challenge + scatter    : %.4f ms\n", m[2] + m[3]);
    }
    for (void *p : {(void *)d_z, (void *)d_c, (void *)d_at, (void *)d_hi, (void *)d_g, (void *)d_out, (void *)d_pos, (void *)d_val,
                    (void *)d_dense})
        HIP_OK(hipFree(p));
    for (auto &e : ev) HIP_OK(hipEventDestroy(e));
    HIP_OK(hipStreamDestroy(s));
    return 0;
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
    switch (o.option) {
    case 4: report_polymul(o, "CT-CT", false); break;
    case 6: report_polymul(o, "CT-GS", false); break;
    case 7: report_polymul(o, "fused", true); break;
    case 8:
        for (int i = 0; i < 5; i++) report_polymul(o, "CT-GS", false);
        for (int i = 0; i < 5; i++) report_polymul(o, "fused", true);
        break;
    case 9: {
        int ok = 0;
        const double ms = run_fwdinv(o, &ok);
        printf("fwd+inv n=%u: %.4f ms per batch of %zu -> %.3e pairs/s, %.1f GB/s algorithmic; round trip %s\n", n, ms,
               o.batch, o.batch / ms * 1e3, o.batch * 16.0 * n / ms / 1e6, ok ? "Identical." : "Incorrect result.");
        return ok ? 0 : 1;
    }
    case 10: {
        int kat = -1;
        const double ms = run_polymul_host(o, &kat);
        printf("\n========================\ntest_NTT_negacyclic fused host->host (pipelined PCIe). Batch Size is %zu"
               "\n========================\n", o.batch);
        printf("Performance GPU fused host->host \n Time\t\t: % .4f ms. \nThroughput\t: %.2f Multiplications per second\n",
               ms, (double)o.batch / ms * 1000.0);
        if (kat >= 0) printf("all-ones KAT z[k] = 2k+2-n mod q: %s\n", kat ? "Identical." : "Incorrect result.");
        return kat == 0 ? 1 : 0;
    }
    case 11: {
        int kat = 0;
        const double ms = run_nussbaumer(o, &kat);
        printf("\n========================\ntest_nussbaumer GPU (mod 2^32-1). Batch Size is %zu\n========================\n",
               o.batch);
        printf("Performance GPU Nussbaumer \n Time\t\t: % .4f ms. \nThroughput\t: %.2f Multiplications per second\n", ms,
               (double)o.batch / ms * 1000.0);
        printf("all-ones KAT z[k] = 2k+2-n mod 2^32-1: %s\n", kat ? "Identical." : "Incorrect result.");
        return kat ? 0 : 1;
    }
    case 12: return run_latency(o);
    case 13: return run_mul_ntt_k(o);
    case 14: return run_mul_ntt_kl(o);
    case 15: return run_round(o);
    case 16: return run_xof(o);
    default: help_message(); return -1;
    }
    return 0;
}
