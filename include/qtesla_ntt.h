/*
 * qtesla_ntt.h -- C ABI of the MI355X (gfx950) batched negacyclic NTT engine.
 *
 * Drop-in boundary for the reference benlwk/ntt-gpu-qTESLA (NTT.cu).  The
 * reference has no library API: its "launch signature" is a family of
 * per-stage __global__ kernels launched <<<BATCH, T>>> by its test drivers
 * over caller-allocated, poly-major device buffers [BATCH][NTTSIZE] of
 * uint32 coefficients in [0,q).  Each entry point below replaces one whole
 * kernel sequence of those drivers (file:line cited per function) with one
 * launch of a hand-written CDNA4 kernel.
 *
 * Conventions (all entry points):
 *   - device pointers, poly-major [batch][n] uint32, coefficients in [0,q);
 *     the caller owns the memory, the library never allocates on the hot path;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are
 *     asynchronous on that stream, reentrant across streams and devices;
 *   - return 0 on success, a negative NTT_ERR_* code otherwise (never abort);
 *   - `twiddleFactor` is accepted and ignored, exactly like the reference
 *     kernels' dead parameter (NTT.cu:1436 etc. read __constant__ tables).
 *   - inputs >= q are a contract violation (the reference silently returns
 *     non-congruent values for them).  This library tolerates inputs in
 *     [0, 2q): the output is then the exact canonical result for the input
 *     reduced mod q (DESIGN.md "lazy reduction bounds").  Outputs are
 *     always canonical, in [0, q).
 */
#ifndef QTESLA_NTT_H
#define QTESLA_NTT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- parameter sets ---------------------------------------------------- */
/* reference set: qTESLA-III-speed (round 1), main.cuh:13-21 + constants.h   */
#define NTT_PARAM_REF 0   /* n = 1024, q = 8404993,   psi = 2083362          */
#define NTT_PARAM_P_I 1   /* n = 1024, q = 343576577, psi = 3^((q-1)/2n)    */
#define NTT_PARAM_P_III 2 /* n = 2048, q = 856145921, psi = 3^((q-1)/2n)    */
/* Larger transforms over p-III's prime (q - 1 = 2^14 * 52255 admits
 * negacyclic n up to 8192), for the reference's n > 2048 dataflows (its
 * Stockham / CT2 kernels, NTT.cu:1085-1153, 1268-1337, 667-951): one wave
 * per polynomial (the n = 8192 products: a multi-wave four-step kernel).
 * For these sets every entry point is accepted except
 * poly_mul_nussbaumer (NTT_ERR_PARAM: its split is defined for n = 1024 /
 * 2048).  poly_mul / poly_mul_ntt are one fused launch; poly_bitrev_copy,
 * poly_ntt_bitrev and poly_invntt_bitrev are one launch each. */
#define NTT_PARAM_N4096 3 /* n = 4096, q = 856145921, psi = 3^((q-1)/2n)    */
#define NTT_PARAM_N8192 4 /* n = 8192, q = 856145921, psi = 3^((q-1)/2n)    */

/* ---- error codes ------------------------------------------------------- */
#define NTT_OK 0
#define NTT_ERR_PARAM (-1)   /* unknown param_set                              */
#define NTT_ERR_NULL (-2)    /* NULL device pointer with batch > 0             */
#define NTT_ERR_ALIGN (-3)   /* device pointer not 4-byte aligned (16-byte for  */
                             /* poly_pointwise and poly_mul_nussbaumer)        */
#define NTT_ERR_HIP (-4)     /* HIP runtime / launch error (ntt_last_hip_error)*/
#define NTT_ERR_SIZE (-5)    /* batch too large (at most 2^31 - 1 polynomials) */
#define NTT_ERR_ALIAS (-6)   /* forbidden partial overlap of in/out buffers    */

/* Parameter query: any out pointer may be NULL.
 * Replaces the compile-time macros P / NTTSIZE (main.cuh:14-16) and the root
 * constants fg0 / ig0 / Ni (main.cu:26). */
int ntt_param_info(int param_set, uint32_t *n, uint32_t *q, uint32_t *psi,
                   uint32_t *omega, uint32_t *omega_inv, uint32_t *n_inv);

/* Host copies of the constants.h-equivalent tables, n entries each (any
 * pointer may be NULL): bitrev_tbl (constants.h:3), Phi = psi^i (:11),
 * invPhi = n^-1 psi^-i (:19), tf0 = omega^i (:29), ti0 = omega^-i (:33).
 * For NTT_PARAM_REF they are bit-identical to constants.h. */
int ntt_get_tables(int param_set, uint32_t *bitrev_tbl, uint32_t *Phi,
                   uint32_t *invPhi, uint32_t *tf0, uint32_t *ti0);

/* Forward negacyclic NTT, in place, natural order in -> natural order out:
 *   X[k] = sum_i x_i psi^{(2k+1) i} mod q.
 * Replaces bit_reverse_copy_tbl_Phi_gpu + radix2NTT_gpu0 x5 + radix2NTT_gpu1 x5
 * (NTT.cu:2388-2400; kernels :502-509, :1436-1470) -- 12 launches -> 1. */
int poly_ntt(uint32_t *d_poly, const uint32_t *twiddleFactor, size_t batch,
             int param_set, void *stream);

/* Inverse negacyclic NTT, in place, natural -> natural (includes n^-1 and
 * psi^-i, i.e. invPhi):  x_i = n^-1 psi^-i sum_k X[k] omega^-ik.
 * Replaces GS_radix2INTT_gpu0 x5 + GS_radix2INTT_gpu2 x5 +
 * bit_reverse_copy_tbl_invPhi_gpu (NTT.cu:2415-2425; kernels :1224-1240,
 * :1033-1056, :494-500) -- 11 launches -> 1. */
int poly_invntt(uint32_t *d_poly, const uint32_t *twiddleFactor, size_t batch,
                int param_set, void *stream);

/* Out-of-place variants (d_out may equal d_in; partial overlap rejected).
 * Unlike bit_reverse_copy_tbl_Phi_gpu (NTT.cu:506) the input is never
 * clobbered when d_out != d_in. */
int poly_ntt_oop(uint32_t *d_out, const uint32_t *d_in, size_t batch,
                 int param_set, void *stream);
int poly_invntt_oop(uint32_t *d_out, const uint32_t *d_in, size_t batch,
                    int param_set, void *stream);

/* Transforms with the NTT domain in bit-reversed order (out of place; d_out
 * may equal d_in, partial overlap rejected), for callers that keep the
 * reference's CT-CT ordering:
 *   poly_ntt_bitrev:    out[t] = X[brv(t)]  (= poly_ntt then poly_bitrev_copy)
 *   poly_invntt_bitrev: input in[t] = X[brv(t)], natural-order output; this
 *     is the CT inverse on bit-reversed input radix2INTT_gpu0 x5 + gpu1 x4 +
 *     gpu2 with its x invPhi (NTT.cu:2240-2249, kernels :1374-1433) -- 10
 *     launches -> 1; poly_bitrev_copy then poly_invntt_bitrev = poly_invntt.
 * Each costs one more LDS transpose per polynomial than the natural-order
 * transform (the bit-reversed side is not lane-contiguous in the pass-2
 * register layout). */
int poly_ntt_bitrev(uint32_t *d_out, const uint32_t *d_in, size_t batch,
                    int param_set, void *stream);
int poly_invntt_bitrev(uint32_t *d_out, const uint32_t *d_in, size_t batch,
                       int param_set, void *stream);

/* Bit-reversal permutation, out[b*n + t] = in[b*n + brv(t)] (log2 n bits),
 * any 32-bit words.  Replaces bit_reverse_copy_tbl_gpu (NTT.cu:487-492), used
 * by the CT-CT pipeline (:2239) to feed radix2INTT with bit-reversed input.
 * d_out may equal d_in (in place); partial overlap is rejected. */
int poly_bitrev_copy(uint32_t *d_out, const uint32_t *d_in, size_t batch,
                     int param_set, void *stream);

/* Fused negacyclic product c = a * b mod (x^n + 1, q), natural order.
 * Replaces the whole CT-GS pipeline of test_NTT_CT_GS_nega_gpu
 * (NTT.cu:2388-2425, 34 launches) and CT-CT (NTT.cu:2213-2249) with one
 * launch; d_c may alias d_a or d_b. */
int poly_mul(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b,
             size_t batch, int param_set, void *stream);

/* Fused product with the second operand already in the NTT domain:
 *   c = a * b mod (x^n + 1, q)  where  d_bhat = poly_ntt(b)  (natural order,
 *   this library's psi, entries < 2q).
 * qTESLA samples its public polynomial directly in the NTT domain; this is
 * the CT-GS driver (NTT.cu:2388-2425) with the second forward transform
 * (:2402-2411) dropped: two transforms of work per product instead of three.
 * d_c may alias d_a or d_bhat. */
int poly_mul_ntt(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_bhat,
                 size_t batch, int param_set, void *stream);

/* Shared NTT-domain rows times a batch, one launch -- qTESLA's
 * t_i = a_i * y (+ e_i) over its k public polynomials, which it samples
 * directly in the NTT domain (k = 1 / 4 / 5 for ref / p-I / p-III):
 *   out[b][i] = a_i * y_b (+ add[b][i])  mod (x^n + 1, q),  0 <= i < k
 *   d_y    [batch][n]      natural order, entries < 2q
 *   d_ahat [k][n]          a_i-hat = poly_ntt(a_i), natural order, entries < 2q;
 *                          shared by the whole batch
 *   d_add  NULL, or [batch][k][n] entries < 2q (may equal d_out: accumulate in place)
 *   d_out  [batch][k][n]   canonical, in [0, q)
 * Each y_b is read and transformed once: k + 1 transforms of work per y_b
 * where k poly_mul_ntt calls over a materialised broadcast of a_i-hat take
 * 2k.  n = 1024 / 2048 sets only (NTT_ERR_PARAM otherwise, and for k outside
 * 1 .. NTT_MUL_K_MAX).  d_out must not overlap d_y or d_ahat, and d_add may
 * overlap d_out only by being equal to it (NTT_ERR_ALIAS); d_add may overlap
 * the inputs. */
#define NTT_MUL_K_MAX 8
int poly_mul_ntt_k(uint32_t *d_out, const uint32_t *d_y, const uint32_t *d_ahat,
                   const uint32_t *d_add, size_t batch, int k, int param_set, void *stream);
/* Launch shape of poly_mul_ntt_k (either out pointer may be NULL).
 * *split_max_batch: the largest batch at which the k rows of each polynomial
 * are spread over k workgroups (each recomputes the forward transform of
 * y_b; 0 = never); larger batches run one work unit per y_b.  Both give
 * identical results; the threshold is the measured crossover of their launch
 * times.  *waves_per_workgroup: work units (one n = 2048 polynomial, or two
 * n = 1024 polynomials) a workgroup processes side by side. */
int ntt_mul_k_shape(int param_set, size_t *split_max_batch, int *waves_per_workgroup);

/* A k x l matrix of shared NTT-domain polynomials times l batches, summed in
 * the NTT domain, one launch -- qTESLA's verification w_i = a_i * z - t_i * c
 * (l = 2: inputs [z, c], row i = [a_i-hat, q - t_i-hat]):
 *   out[b][i] = sum_{j<l} a_ij * y_j[b]  (+ add[b][i])   mod (x^n + 1, q),  0 <= i < k
 *   d_y     HOST array of l device pointers, each [batch][n], natural order,
 *           entries < 2q.  The array is read during the call only; the l
 *           batches are used where they lie (no interleaving copy)
 *   d_ahat  [k][l][n]   a_ij-hat = poly_ntt(a_ij), natural order, entries < 2q;
 *           shared by the whole batch
 *   d_add   NULL, or [batch][k][n] entries < 2q (may equal d_out: accumulate in place)
 *   d_out   [batch][k][n] canonical, in [0, q)
 * There is no subtracting form: a caller that needs - t_i * c stores the
 * negated row q - t_i-hat (entrywise, 0 stays 0 or becomes q: both < 2q), once
 * per key.  The NTT is linear, so the l products of a row share one inverse
 * transform: k + l transforms of work per b where two poly_mul_ntt_k launches
 * take 2(k + 1), and no addend round trip through memory.  l = 1 is
 * poly_mul_ntt_k.  n = 1024 / 2048 sets only (NTT_ERR_PARAM otherwise, and
 * for k outside 1 .. NTT_MUL_K_MAX or l outside 1 .. NTT_MUL_L_MAX).  d_out
 * must not overlap any d_y[j] or d_ahat (k*l*n words), and d_add may overlap
 * d_out only by being equal to it (NTT_ERR_ALIAS); the d_y[j] may overlap each
 * other and d_add freely (d_y[0] == d_y[1] gives (a_i0 + a_i1) * y). */
#define NTT_MUL_L_MAX 2
int poly_mul_ntt_kl(uint32_t *d_out, const uint32_t *const *d_y, const uint32_t *d_ahat,
                    const uint32_t *d_add, size_t batch, int k, int l, int param_set, void *stream);
/* Launch shape of poly_mul_ntt_kl for l inputs, as ntt_mul_k_shape (l = 1:
 * exactly that; NTT_ERR_PARAM for l outside 1 .. NTT_MUL_L_MAX). */
int ntt_mul_kl_shape(int param_set, int l, size_t *split_max_batch, int *waves_per_workgroup);

/* Sparse to dense: out[b][pos[b][j]] = val[b][j] mod q for j < h, every other
 * coefficient 0 -- qTESLA's challenge c, h positions and signs (+1 -> 1,
 * -1 -> q - 1) out of the hash, as the dense polynomial every entry point
 * above takes.
 *   d_pos, d_val [batch][h] uint32; val < 2q; d_out [batch][n] canonical,
 *   every word written.
 * Entries with pos >= n are ignored.  Positions within one polynomial are
 * distinct (if not, one of the values wins).  1 <= h <= n (NTT_ERR_PARAM
 * otherwise).  All five parameter sets.  d_out must not overlap d_pos or
 * d_val (NTT_ERR_ALIAS). */
int poly_scatter(uint32_t *d_out, const uint32_t *d_pos, const uint32_t *d_val,
                 size_t batch, int h, int param_set, void *stream);

/* qTESLA's rounding [.]_M and the two norm maxima its signer tests, per
 * polynomial.  For a coefficient x < 2q and the bit count d:
 *   x' = x mod q
 *   c  = x' > (q-1)/2 ? x' - q : x'               centred, |c| <= (q-1)/2
 *   lo = c mod+- 2^d  in (-2^(d-1), 2^(d-1)]      (c & (2^d - 1), minus 2^d if > 2^(d-1))
 *   hi = (c - lo) >> d                             = (c + 2^(d-1) - 1) >> d, arithmetic shift
 *   d_w     [batch][n]   entries < 2q, only read ([B][k][n]: pass batch = B*k)
 *   d_hi    NULL, or [batch][n] bytes: hi, two's complement (the hash's input)
 *   d_norms NULL, or [batch][2] uint32: { max |c|, max |lo| } of each polynomial
 * Whichever output is NULL is neither computed nor touched; both NULL with
 * batch > 0 is NTT_ERR_NULL.  The library keeps no scheme constants: d is the
 * caller's (qTESLA: 22 / 22 / 24 for ref / p-I / p-III), and the caller
 * compares the maxima with its own B - S (test_rejection, on z) and
 * floor(q/2) - E, 2^(d-1) - E (test_correctness, on w_i).  1 <= d <= 30, and
 * with d_hi the largest hi, ((q-1)/2 + 2^(d-1) - 1) >> d, must fit a signed
 * byte (<= 127: d >= 16 / 21 / 22 for ref / p-I / p-III's prime),
 * NTT_ERR_PARAM otherwise.  d_w and d_hi 16-byte aligned, d_norms 8-byte
 * (NTT_ERR_ALIGN); no two of the three buffers overlap (NTT_ERR_ALIAS).  All
 * five parameter sets. */
int poly_round(uint8_t *d_hi, uint32_t *d_norms, const uint32_t *d_w,
               size_t batch, int d, int param_set, void *stream);

/* poly_mul_ntt_kl with poly_round as its store epilogue: the verifier's
 * w_i = a_i * z - t_i * c is rounded where it is computed and the full-width
 * w never reaches memory.  Bit-identical to poly_mul_ntt_kl into a temporary
 * followed by poly_round over batch * k polynomials:
 *   d_hi    NULL, or [batch][k][n] bytes
 *   d_norms NULL, or [batch][k][2] uint32
 * d_y, d_ahat, d_add, k, l and the n = 1024 / 2048 restriction are
 * poly_mul_ntt_kl's, the inputs may overlap each other as there; d, NULL
 * outputs, their alignment and the byte-range rule are poly_round's.  The
 * outputs overlap no input (d_add included) and not each other
 * (NTT_ERR_ALIAS).  l = 1 is served by the same kernel: the signer's
 * w_i = v_i - e_i * c with d_add = v, where only d_norms is wanted.  The
 * launch shape is ntt_mul_kl_shape(param_set, 2, ...)'s for both l. */
int poly_mul_ntt_kl_round(uint8_t *d_hi, uint32_t *d_norms, const uint32_t *const *d_y,
                          const uint32_t *d_ahat, const uint32_t *d_add, size_t batch,
                          int k, int l, int d, int param_set, void *stream);

/* poly_mul_ntt_kl and poly_mul_ntt_kl_round over many keys, one launch: every
 * message of the batch names the key whose rows it is multiplied by -- a
 * verifier's batch of signatures made under different public keys, or (l = 1,
 * d_key NULL) a key-generation batch's t_b = a_b * s_b + e_b with one a per key.
 *   d_ahat  [nkeys][k][l][n]  key j's block is exactly the [k][l][n] the unkeyed
 *           entry point takes, entries < 2q; there is no stride between keys.
 *           l = 2: poly_gen_a(batch = nkeys, pstride = 2n) fills slot 0 of all
 *           keys in one call; l = 1: poly_gen_a's dense output is d_ahat as it lies
 *   d_key   NULL, or [batch] uint32: message b uses key
 *               min(d_key ? d_key[b] : b, nkeys - 1)
 *           The minimum is the definition, not an error path: the device cannot
 *           return an error, and no index makes the kernel read outside d_ahat.
 *           An index >= nkeys is the caller's bug, and its result is the last
 *           key's.  With d_key NULL and nkeys >= batch, message b is under key b.
 * Everything else -- d_y, d_add, d_out / d_hi / d_norms, k, l, d, the n = 1024 /
 * 2048 restriction, NULL outputs and the byte-range rule of d -- is as in the
 * unkeyed entry point of the same name; with every index equal to j the result
 * is bit-identical to that call on key j's block.  Both l run the same kernel,
 * in the launch shape of ntt_mul_kl_shape(param_set, 2, ...).
 * The checks follow the unkeyed entry point's order, with
 *   NTT_ERR_PARAM  also for nkeys == 0 (an empty batch is NTT_OK after that)
 *   NTT_ERR_ALIGN  d_key not 4-byte aligned (NULL is accepted)
 *   NTT_ERR_SIZE   also for nkeys > NTT_MUL_KEYS_MAX = 2^31 - 1
 *   NTT_ERR_ALIAS  an output overlaps d_key's batch words or any of d_ahat's
 *                  nkeys*k*l*n words; d_key may overlap the other inputs. */
#define NTT_MUL_KEYS_MAX 2147483647
int poly_mul_ntt_kl_keyed(uint32_t *d_out, const uint32_t *const *d_y, const uint32_t *d_ahat,
                          const uint32_t *d_key, size_t nkeys, const uint32_t *d_add,
                          size_t batch, int k, int l, int param_set, void *stream);
int poly_mul_ntt_kl_round_keyed(uint8_t *d_hi, uint32_t *d_norms, const uint32_t *const *d_y,
                                const uint32_t *d_ahat, const uint32_t *d_key, size_t nkeys,
                                const uint32_t *d_add, size_t batch, int k, int l, int d,
                                int param_set, void *stream);

/* SHAKE128 / SHAKE256 / qTESLA's cshake*_simple over a batch, one launch --
 * qTESLA's H and G on the device, so that the hi bytes poly_mul_ntt_kl_round
 * writes never leave it:
 *   message b = in0[b][0 .. len0) || in1[b][0 .. len1),   out[b] = outlen bytes
 *   d_in0 [batch][len0] bytes, d_in1 [batch][len1] bytes, d_out [batch][outlen]
 * The two segments are used where they lie (qTESLA's c'' = H([w]_M || G(m)):
 * the hi bytes [batch][k n] and the digests [batch][64] are different buffers;
 * no interleaving copy).  Either length may be 0, and a pointer whose length
 * is 0 is not looked at (it may be NULL, misaligned, anywhere).
 *   algo   NTT_XOF_SHAKE128 (rate 168) or NTT_XOF_SHAKE256 (rate 136)
 *   cstm   -1: plain SHAKE, domain/pad byte 0x1F.
 *          0 .. 65535: cshake128_simple / cshake256_simple, i.e. NIST cSHAKE
 *          with an empty function name N and the customization string S = the
 *          two bytes of cstm, little-endian: the first absorbed block is
 *          01 <rate> 01 00 01 10 lo hi (<rate> = A8 / 88) and zeros up to the
 *          rate, one permutation, then the message with domain byte 0x04.
 * len0 and len1 are multiples of 8 with len0 + len1 < 2^32 (a message ends on
 * a 64-bit lane of the sponge); outlen is a multiple of 8 with
 * 8 <= outlen <= NTT_XOF_OUT_MAX.  There is no param_set: the library keeps
 * no scheme constants.  Checks, in this order (the first defect decides):
 *   NTT_ERR_PARAM  unknown algo, cstm outside -1 .. 65535, a bad len0 / len1 /
 *                  outlen
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_out, or a segment of non-zero length
 *   NTT_ERR_ALIGN  any of the three pointers not 8-byte aligned
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_out overlaps an input (the inputs may overlap each other)
 * Two kernel families give the same bytes: one message per lane, whose
 * throughput comes from the batch, and two messages per wave (the sponge's
 * state spread over the lanes), whose chain of permutations is shorter.
 * ntt_xof runs the second for batch <= ntt_xof_small_batch_max(algo, 0, .) and
 * the first above; ntt_xof_path takes the choice as an argument.
 *
 * ntt_xof_path is ntt_xof with the kernel family named: NTT_XOF_PATH_AUTO is
 * ntt_xof itself, NTT_XOF_PATH_LANE and NTT_XOF_PATH_WAVE run one family at
 * every batch.  All three give identical bytes for every legal input.  A path
 * outside 0 .. 2 is NTT_ERR_PARAM, with the first check; every other check,
 * its order and its code are ntt_xof's.
 * ntt_xof_small_batch_max: the largest batch at which NTT_XOF_PATH_AUTO runs
 * the wave kernels (0: never), for ntt_xof (ragged = 0) or ntt_xof_ragged
 * (ragged = 1).  NTT_ERR_PARAM for an unknown algo or a ragged outside 0 / 1,
 * then NTT_ERR_NULL for a NULL max_batch. */
#define NTT_XOF_SHAKE128 0   /* rate 168 */
#define NTT_XOF_SHAKE256 1   /* rate 136 */
#define NTT_XOF_OUT_MAX 512
#define NTT_XOF_PATH_AUTO 0   /* what ntt_xof / ntt_xof_ragged do */
#define NTT_XOF_PATH_LANE 1   /* one message per lane (k_xof, k_xof_ragged) */
#define NTT_XOF_PATH_WAVE 2   /* two messages per wave */
int ntt_xof(uint8_t *d_out, size_t outlen, const uint8_t *d_in0, size_t len0,
            const uint8_t *d_in1, size_t len1, size_t batch, int algo, int cstm, void *stream);
int ntt_xof_path(uint8_t *d_out, size_t outlen, const uint8_t *d_in0, size_t len0,
                 const uint8_t *d_in1, size_t len1, size_t batch, int algo, int cstm, int path,
                 void *stream);
/* largest batch at which PATH_AUTO runs the wave kernels (0 = never) */
int ntt_xof_small_batch_max(int algo, int ragged, size_t *max_batch);

/* ntt_xof's hash over messages of any byte length, each its own, one launch --
 * qTESLA's G(m), the 64-byte digest of every message of a batch, from the
 * messages as they arrive:
 *   d_msg [msg_bytes] bytes    all messages back to back (CSR style)
 *   d_off [batch + 1] uint64   their byte offsets, in device memory
 *   d_out [batch][outlen]
 * Message b is d_msg[begin_b .. end_b) with
 *   begin_b = min(d_off[b], msg_bytes)
 *   end_b   = min(max(d_off[b + 1], begin_b), msg_bytes)
 * The minimum and the maximum are the definition, not an error path (the
 * device cannot return an error; poly_mul_ntt_kl_keyed treats its key index the
 * same way): no offset makes the kernel read outside d_msg.  For a well-formed
 * table -- non-decreasing, ending at or below msg_bytes -- message b is simply
 * [d_off[b], d_off[b + 1]).  Any length is legal, 0 included, and a message
 * may start at any byte.  Offsets and lengths are 64-bit throughout.
 *   algo, cstm, outlen   exactly ntt_xof's: NTT_XOF_SHAKE128 / NTT_XOF_SHAKE256;
 *          cstm -1 plain SHAKE (domain byte 0x1F), 0 .. 65535 cshake*_simple
 *          (the prefix block, one permutation, then domain byte 0x04); outlen a
 *          multiple of 8 with 8 <= outlen <= NTT_XOF_OUT_MAX.
 * Padding, with L = end_b - begin_b and r = L mod rate: the full rate blocks
 * are absorbed; the last block gets the r remaining bytes, the domain byte at
 * byte r and 0x80 at byte rate - 1.  For r = rate - 1 both land on the same
 * byte (0x9F for SHAKE, 0x84 for cSHAKE); for r = 0 the last block is padding
 * only.
 * Read range: msg_bytes is a multiple of 8 -- the caller pads the buffer --
 * and d_msg is 8-byte aligned.  The kernel reads d_msg only in aligned 8-byte
 * words that contain at least one byte of some message's [begin_b, end_b), so
 * never outside [d_msg, d_msg + msg_bytes); bytes that are not message b's never
 * influence d_out[b].  msg_bytes == 0 is legal: every message is then empty and
 * d_msg is not looked at (it may be NULL, misaligned, anywhere).
 * Checks, in this order (the first defect decides; all before any GPU work):
 *   NTT_ERR_PARAM  unknown algo, cstm outside -1 .. 65535, a bad outlen,
 *                  msg_bytes not a multiple of 8
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_out, d_off, or d_msg with msg_bytes > 0
 *   NTT_ERR_ALIGN  any of the three pointers not 8-byte aligned (d_msg counts
 *                  only with msg_bytes > 0)
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_out's batch * outlen bytes overlap d_msg's msg_bytes or
 *                  d_off's 8 (batch + 1) bytes (the two inputs may overlap each
 *                  other)
 * One launch for every batch size.  With one message per lane a wave of 64
 * consecutive messages costs its longest message's serial chain of
 * permutations, and with two messages per wave the pair costs the longer
 * one's: a caller with very uneven lengths should sort or bucket the messages
 * by length.  There is no cooperative path for one huge message.
 * ntt_xof_ragged runs two messages per wave for batch <=
 * ntt_xof_small_batch_max(algo, 1, .) and one message per lane above;
 * ntt_xof_ragged_path takes the choice as an argument, as ntt_xof_path does:
 * identical bytes on every path, a path outside 0 .. 2 is NTT_ERR_PARAM with
 * the first check, everything else is ntt_xof_ragged's. */
int ntt_xof_ragged(uint8_t *d_out, size_t outlen, const uint8_t *d_msg, size_t msg_bytes,
                   const uint64_t *d_off, size_t batch, int algo, int cstm, void *stream);
int ntt_xof_ragged_path(uint8_t *d_out, size_t outlen, const uint8_t *d_msg, size_t msg_bytes,
                        const uint64_t *d_off, size_t batch, int algo, int cstm, int path,
                        void *stream);

/* qTESLA's Enc(c'): a seed to the h positions and signs of the challenge,
 * exactly the lists poly_scatter takes.
 *   d_seed [batch][seedlen] bytes; d_pos, d_val [batch][h] uint32
 * Each seed on its own, with n and q of param_set (encode_c, restated):
 *   dmsp = 0;  r = cSHAKE128_simple(168 bytes, cstm = dmsp++, seed);  cnt = 0;  i = 0
 *   while i < h:
 *       if cnt > 168 - 3:  r = cSHAKE128_simple(168 bytes, cstm = dmsp++, seed);  cnt = 0
 *       pos = ((r[cnt] << 8) | r[cnt+1]) & (n - 1)
 *       if pos not yet taken:  d_pos[i] = pos;  d_val[i] = (r[cnt+2] & 1) ? q - 1 : 1;  i++
 *       cnt += 3
 * A block of 168 bytes gives 56 draws.  The loop runs for at most
 * NTT_CHALLENGE_BLOCKS_MAX blocks (no unbounded loop on the device); with
 * h <= 128 and n >= 1024 a draw is accepted with probability >= 7/8, so hash
 * outputs never come near the bound.  Were it reached, the entries not yet
 * drawn get pos = 0xFFFFFFFF, which poly_scatter ignores, and val = 0.
 * 1 <= h <= NTT_CHALLENGE_H_MAX; seedlen is a multiple of 8 with
 * 8 <= seedlen <= 160 (one absorb block; qTESLA: 32).  All five parameter
 * sets.  Checks, in this order: NTT_ERR_PARAM (param_set, h, seedlen),
 * batch == 0 (NTT_OK), NTT_ERR_NULL, NTT_ERR_ALIGN (all three pointers 8-byte
 * aligned), NTT_ERR_SIZE, NTT_ERR_ALIAS (the outputs overlap neither the seeds
 * nor each other). */
#define NTT_CHALLENGE_H_MAX 128
#define NTT_CHALLENGE_BLOCKS_MAX 64
int poly_challenge(uint32_t *d_pos, uint32_t *d_val, const uint8_t *d_seed,
                   size_t seedlen, size_t batch, int h, int param_set, void *stream);

/* qTESLA's masking polynomial: one seed and a nonce to the n coefficients of
 * y, canonical in [0, q), centred in [-B, B] with B = 2^(bits-1) - 1 -- the
 * signer's first step, so that v = a y, [v]_M, H, Enc(c') and z = y + s c all
 * start from device memory.
 *   d_y     [batch][n] uint32, every word written
 *   d_seed  [batch][seedlen] bytes
 *   d_nonce NULL, or [batch] uint32: one attempt counter per message, so that
 *           a batch whose messages are at different attempts is one launch
 * Message b uses nonce_b = ((d_nonce ? d_nonce[b] : 0) + nonce) & 0xFF.
 * `bits` is qTESLA's B_BITS + 1 (20 for p-I, 22 for p-III) and the hash is the
 * caller's (the library keeps no scheme constants); n and q are param_set's.
 * Each seed on its own, with rate = 168 / 136 and ntt_xof's cshake*_simple
 * (sample_y of qTESLA round 2, restated from memory -- a first call of 3 n
 * bytes, then single-rate-block refills with the customisation counted up,
 * and the (nonce << 8) domain separation; this statement, not the upstream
 * file, is what the tests bind):
 *   mask = 2^bits - 1;  B = 2^(bits-1) - 1;  cstm = (nonce_b << 8) & 0xFFFF
 *   buf = cshake_simple(algo, seed, outlen = 3 n, cstm);  limit = 3 n;  pos = 0;  r = 0;  i = 0
 *   while i < n:
 *       if pos >= limit:
 *           r += 1;  buf = cshake_simple(algo, seed, outlen = rate, (cstm + r) & 0xFFFF)
 *           limit = 3 * (rate / 3);  pos = 0         (56 draws; 45 draws, byte 135 unused)
 *       v = (buf[pos] | buf[pos+1] << 8 | buf[pos+2] << 16) & mask;  pos += 3
 *       if v != mask:  y[i] = (v - B) mod q;  i += 1      (v == mask would be 2^(bits-1))
 * A draw is always three bytes; bits below 17 is outside qTESLA but legal.
 * Refills are bounded, r <= NTT_SAMPLE_Y_REFILLS_MAX (no unbounded loop on the
 * device, and cstm + r stays inside this nonce's range); with bits >= 2 a draw
 * is accepted with probability >= 3/4 and 255 refills add >= 11 475 draws, so
 * hash outputs never come near the bound.  Were it reached, the coefficients
 * not yet drawn get 0.
 * algo is NTT_XOF_SHAKE128 or NTT_XOF_SHAKE256.  All five parameter sets.
 * Checks, in this order (the first defect decides):
 *   NTT_ERR_PARAM  param_set; algo; bits outside 2 .. 24; nonce > 255; seedlen
 *                  not a multiple of 8 or outside 8 .. rate - 8 (one absorb
 *                  block: 160 / 128)
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_y, d_seed
 *   NTT_ERR_ALIGN  d_y 16-byte, d_seed 8-byte, d_nonce 4-byte when not NULL
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_y overlaps d_seed or d_nonce
 * One seed per lane, as ntt_xof: the throughput comes from the batch. */
#define NTT_SAMPLE_Y_REFILLS_MAX 255
int poly_sample_y(uint32_t *d_y, const uint8_t *d_seed, size_t seedlen,
                  const uint32_t *d_nonce, uint32_t nonce, size_t batch,
                  int bits, int algo, int param_set, void *stream);

/* qTESLA's GenA: seed_a to the k public polynomials a_1 .. a_k, so that a
 * verifier that holds only public-key bytes, and a key-generation batch, make
 * their rows on the device.  qTESLA samples a directly in the NTT domain: the
 * output is exactly the d_ahat that poly_mul_ntt_k / _kl / _kl_round take.
 *   d_seed [batch][seedlen] bytes
 *   d_a    polynomial i of key b starts at word (b * k + i) * pstride; its n
 *          words are each written exactly once, by plain vector stores; the
 *          pstride - n words after it are never written.  pstride = n is the
 *          dense [batch][k][n] of poly_mul_ntt_k; pstride = 2 n writes slot 0
 *          of poly_mul_ntt_kl's [k][2][n] rows in place, beside q - t-hat.
 * Each seed on its own.  q and n are param_set's, qbits is the bit length of
 * q, nbytes = (qbits + 7) / 8, mask = 2^qbits - 1, and cshake128_simple is
 * ntt_xof's, with rate 168 (poly_uniform of qTESLA round 2, restated from
 * memory; this statement, not the upstream file, is what the tests bind):
 *   buf = cshake128_simple(seed, outlen = 168 * nblocks, cstm = 0);  nb = nblocks;  pos = 0;  dmsp = 1;  i = 0
 *   while i < k * n:
 *       if pos > 168 * nb - 4 * nbytes:
 *           nb = 1;  buf = cshake128_simple(seed, outlen = 168, cstm = dmsp);  dmsp += 1;  pos = 0
 *       four times:  v = le32(buf + pos) & mask;  pos += nbytes
 *                    if v < q and i < k * n:  a[i / n][i % n] = v;  i += 1
 * Flat draw stream: a call of nb blocks gives 4 * floor(168 * nb / (4 * nbytes))
 * draws; for nbytes = 4 a refill block is 40 draws with words 40 and 41 unused,
 * and an odd nblocks also leaves its last two words unused.
 * The values are the plain v, canonical in [0, q), in natural order.  Upstream
 * multiplies each by a Montgomery constant of its own NTT, which is
 * representation and not scheme.
 * nblocks is the caller's (the library keeps no scheme constants; qTESLA's
 * PARAM_GEN_A is 108 for p-I and 180 for p-III), 1 <= nblocks <=
 * NTT_GEN_A_BLOCKS_MAX.
 * Refills are bounded: refills_max(k, n) = min(65535, 4 * ceil(k n / 40)) (no
 * unbounded loop on the device, and cstm never leaves 16 bits).  q >=
 * 2^(qbits-1), so a draw is accepted with probability >= 1/2 and the bound
 * allows at least twice the draws the worst prime needs on average: hash
 * outputs cannot reach it.  Were it reached, the coefficients not yet drawn
 * get 0.
 * Parameter sets: those with nbytes = 4 (p-I, p-III, p-III-4096, p-III-8192),
 * where every draw is one whole 32-bit word of the squeezed state.  `ref` has
 * a 24-bit prime, would need three-byte draws and is not a qTESLA set:
 * NTT_ERR_PARAM.
 * Checks, in this order (the first defect decides):
 *   NTT_ERR_PARAM  unknown param_set, or ref; k outside 1 .. NTT_MUL_K_MAX;
 *                  nblocks outside 1 .. 256; seedlen not a multiple of 8 or
 *                  outside 8 .. 160 (one absorb block; qTESLA: 32);
 *                  pstride < n or not a multiple of 4
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_a, d_seed
 *   NTT_ERR_ALIGN  d_a 16-byte, d_seed 8-byte
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_a's extent, ((batch k - 1) pstride + n) words, overlaps
 *                  the seeds
 * One seed per lane, as ntt_xof: the throughput comes from the batch. */
#define NTT_GEN_A_BLOCKS_MAX 256
int poly_gen_a(uint32_t *d_a, size_t pstride, const uint8_t *d_seed, size_t seedlen,
               size_t batch, int k, int nblocks, int param_set, void *stream);

/* qTESLA's Gaussian sampler: one seed and a nonce to the n coefficients of a
 * secret polynomial (s, e_1 .. e_k), each a constant-time count over a
 * cumulative distribution table -- key generation's first step, so that no
 * secret coefficient is ever produced on the host.
 *   d_out   [batch][n] uint32, every word written once
 *   d_seed  [batch][seedlen] bytes, one seed per polynomial
 *   d_nonce NULL, or [batch] uint32: one restart counter per polynomial
 *   d_cdt   [rows][cols] uint32, the table, most significant limb first; only
 *           the low 31 bits of a word are used
 * Polynomial b uses nonce_b = ((d_nonce ? d_nonce[b] : 0) + nonce) & 0xFF,
 * exactly as poly_sample_y.  The table is the caller's (the library keeps no
 * scheme constants), as is the hash; n and q are param_set's.  Row j is the
 * integer
 *   T_j = sum_k (cdt[j][k] & 0x7FFFFFFF) * 2^(31 (cols - 1 - k))
 * and every row is compared: a qTESLA caller passes its table from row 1 on,
 * because upstream's row 0 is zero and skipped.  A polynomial is n / 512
 * chunks (n is a multiple of 512 in all five parameter sets, at most 16
 * chunks), each chunk a cSHAKE call of its own with ntt_xof's cshake*_simple
 * (sample_gauss_poly of qTESLA round 2, restated from memory; this statement,
 * not the upstream file, is what the tests bind):
 *   for ch in 0 .. n / 512 - 1:
 *       buf = cshake_simple(algo, seed_b, outlen = 512 * cols * 4,
 *                           cstm = ((nonce_b << 8) + ch) & 0xFFFF)
 *       for i in 0 .. 511:
 *           W_k  = le32(buf + 4 * (i * cols + k))            for k < cols
 *           R    = sum_k (W_k & 0x7FFFFFFF) * 2^(31 (cols - 1 - k))
 *           m    = #{ j < rows : R >= T_j }
 *           sign = W_0 >> 31
 *           out[b][512 * ch + i] = (sign && m) ? q - m : m
 * The value is canonical in [0, q): "-0" is 0, never q.  There is no
 * rejection and no refill: the stream positions of every sample are fixed.
 * Constant time: the outputs and their source words are secret.  On the
 * device no branch, loop bound, memory address or LDS address depends on R, m
 * or sign; the count always runs over all `rows` rows, and a comparison is a
 * flag, not a jump.  (This rule is kept by construction and verified by
 * reading csrc/ntt_gauss.hpp; no test can observe it.)
 * 1 <= rows <= NTT_GAUSS_ROWS_MAX, 1 <= cols <= NTT_GAUSS_COLS_MAX (qTESLA:
 * cols 2 for p-I, 4 for p-III); algo is NTT_XOF_SHAKE128 or NTT_XOF_SHAKE256.
 * All five parameter sets.  Checks, in this order (the first defect decides):
 *   NTT_ERR_PARAM  param_set; algo; rows outside 1 .. 128; cols outside 1 .. 4;
 *                  nonce > 255; seedlen not a multiple of 8 or outside
 *                  8 .. rate - 8 (one absorb block: 160 / 128)
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_out, d_seed, d_cdt
 *   NTT_ERR_ALIGN  d_out 16-byte, d_seed 8-byte, d_cdt 4-byte, d_nonce 4-byte
 *                  when not NULL
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_out overlaps the seeds, the nonces or the table
 * One chunk per lane: a batch gives batch * n / 512 lanes, and the throughput
 * comes from the batch. */
#define NTT_GAUSS_CHUNK 512
#define NTT_GAUSS_ROWS_MAX 128
#define NTT_GAUSS_COLS_MAX 4
int poly_sample_gauss(uint32_t *d_out, const uint8_t *d_seed, size_t seedlen,
                      const uint32_t *d_nonce, uint32_t nonce,
                      const uint32_t *d_cdt, int rows, int cols,
                      size_t batch, int algo, int param_set, void *stream);

/* qTESLA's check_ES: the sum of the h largest |coefficients| of a polynomial,
 * which key generation compares with L_S / L_E and which bounds |s c| and
 * |e c| in the signer's tests.
 *   d_w   [batch][n] uint32, entries < 2q
 *   d_sum [batch] uint64
 * With c_i the centred value of coefficient i exactly as poly_round defines
 * it (x' = x mod q, c = x' - q if x' > (q-1)/2, else x'), d_sum[b] is the sum
 * of the h largest |c_i| of polynomial b; equal values are counted as often
 * as they occur (the sum of the first h entries of |c| sorted downwards).
 * The output is 64-bit because h (q-1)/2 exceeds 32 bits.  1 <= h <= n.  The
 * input is secret: control flow and addresses do not depend on it.
 * All five parameter sets.  Checks, in this order (the first defect decides):
 *   NTT_ERR_PARAM  param_set; h outside 1 .. n
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_sum, d_w
 *   NTT_ERR_ALIGN  d_w 16-byte, d_sum 8-byte
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_sum overlaps d_w */
int poly_hsum(uint64_t *d_sum, const uint32_t *d_w, size_t batch, int h,
              int param_set, void *stream);

/* qTESLA's wire formats: coefficients to bit-packed rows and back -- a
 * signature's z as n fields of B_BITS + 1 bits (p-I: 20, p-III: 22), a public
 * key's t as k n fields of ceil(log2 q) bits (29 / 30) -- so that signature
 * and key bytes go to and come from the device as they are on the wire.  Both
 * calls are general in the field width, in signed or unsigned fields and in k
 * polynomials per row; the library keeps no scheme constants.  (encode_sig /
 * decode_sig / encode_pk / decode_pk of qTESLA round 2, bit layout restated
 * from memory; this statement, not the upstream file, is what the tests bind.)
 * Let q and n be param_set's, qbits the bit length of q (24 for ref, 29 for
 * p-I, 30 for p-III and the larger sets) and b = bits.
 *   Bit stream.  A polynomial's packed form is n b / 8 bytes.  Field i
 *     occupies stream bits [i b, (i+1) b); stream bit j is bit j mod 8 of byte
 *     j / 8, equivalently bit j mod 32 of little-endian dword j / 32.  For
 *     b = 20 this is qTESLA's pt[0] = (z0 & m) | (z1 << 20),
 *     pt[1] = (z1 >> 12) | (z2 << 8) | (z3 << 28), and so on.  n is a multiple
 *     of 1024, so a polynomial is a multiple of 128 bytes.
 *   Rows.  Row r of the byte side starts at r * stride and holds k
 *     polynomials back to back, k n b / 8 bytes.  Bytes [k n b / 8, stride) of
 *     a row belong to the caller (c', seed_a): poly_pack never writes them,
 *     poly_unpack never reads them.  The coefficient side is dense
 *     [batch][k][n] uint32.
 *   poly_pack.  An input word x is < 2q, as for poly_round; x' = x mod q.
 *     sgn = 1:  c = x' - q if x' > (q-1)/2, else x'; the field is c mod 2^b,
 *               the two's-complement low b bits.
 *     sgn = 0:  the field is x' mod 2^b.
 *     A value outside the field's range is truncated: keeping values in range
 *     is the caller's responsibility (a signer packs only a z that has passed
 *     its norm test).
 *   poly_unpack.  Let f be the field.
 *     sgn = 1:  s is the sign extension of f; the output is s if s >= 0, else
 *               s + q; the maximum is max |s| over the polynomial, so a field
 *               of -2^(b-1) reports 2^(b-1).
 *     sgn = 0:  the output is f if f < q, else f - q (always canonical:
 *               b <= qbits gives f < 2q); the maximum is max f, the raw field,
 *               so the caller sees a malformed key as a maximum >= q.
 *     d_max is NULL or [batch][k] uint32; with it, decoding and the verifier's
 *     max |z| test read the signature once.
 *   Limits.  8 <= bits <= qbits - 1 when signed, 8 <= bits <= qbits when
 *     unsigned; 1 <= k <= NTT_MUL_K_MAX; stride a multiple of 16 and
 *     >= k n bits / 8.  With the signed limit 2^(b-1) <= (q-1)/2, hence
 *       poly_pack(poly_unpack(bytes)) == bytes   for every byte string, and
 *       poly_unpack(poly_pack(w)) == w mod q     whenever w's centred values
 *                                                fit b bits;
 *     unsigned, the byte round trip holds exactly when every f < q.
 * All five parameter sets; asynchronous on `stream`; every output word is
 * written once by a plain vector store.  Checks, in this order (the first
 * defect decides):
 *   NTT_ERR_PARAM  param_set; k; sgn not 0 or 1; bits; stride
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_out / d_w / d_in (d_max may be NULL)
 *   NTT_ERR_ALIGN  byte side and coefficient side 16-byte, d_max 4-byte
 *   NTT_ERR_SIZE   batch * k > 2^31 - 1
 *   NTT_ERR_ALIAS  an output overlaps the input, or d_max overlaps d_w; the
 *                  byte side's extent is (batch - 1) * stride + k n bits / 8 */
int poly_pack(uint8_t *d_out, size_t stride, const uint32_t *d_w, size_t batch,
              int k, int bits, int sgn, int param_set, void *stream);
int poly_unpack(uint32_t *d_w, uint32_t *d_max /* [batch][k] or NULL */, const uint8_t *d_in,
                size_t stride, size_t batch, int k, int bits, int sgn, int param_set, void *stream);

/* Packed rows straight to NTT-domain polynomials, one launch: poly_unpack,
 * poly_ntt and, with neg, the entrywise negation, without the two full-width
 * temporaries between them -- a public key's t to slot 1 of the verification
 * rows (q - t-hat), a signer's s and e_i from its key bytes to s-hat and
 * q - e-hat_i.
 *   Byte side.  Exactly poly_unpack's: rows `stride` bytes apart, k
 *     polynomials of n b / 8 bytes back to back, the bit stream, the field
 *     layout and sgn as defined there.  Bytes [k n b / 8, stride) of a row are
 *     never read.
 *   Value.  Let x be the canonical polynomial poly_unpack gives for a
 *     polynomial's bytes and X = poly_ntt(x): natural order, this library's
 *     psi.  The result is X when neg = 0 and (q - X) mod q entrywise when
 *     neg = 1, so 0 stays 0.  Either way it is canonical, in [0, q), and
 *     bit-identical to poly_unpack into a temporary followed by poly_ntt
 *     (neg = 1: followed by the entrywise negation mod q).
 *   Placement.  Polynomial i of row r is written to words
 *     [(r k + i) pstride, (r k + i) pstride + n) of d_out, every one of them
 *     once by a plain vector store; the pstride - n words after a polynomial
 *     are never written.  pstride = n is dense [batch][k][n]; pstride = 2n with
 *     d_out = d_at + n fills slot 1 of [nkeys][k][2][n] verification rows in
 *     place, beside poly_gen_a's slot 0.
 *   Maxima.  d_max is poly_unpack's, NULL or [batch][k] uint32: signed fields
 *     give max |s|, unsigned fields the largest raw field, so a malformed key
 *     shows as a maximum >= q.  With d_max NULL nothing is computed for it.
 *   Secret input.  With sgn = 1 the bytes may be a signer's key.  On the
 *     device no branch, loop bound, global or LDS address depends on a field's
 *     value: addresses are functions of the lane, the register index, b and the
 *     polynomial's index; sign extension, reduction and maximum are selects.
 *     (Kept by construction and verified by reading csrc/ntt_unpack_ntt.hpp;
 *     no test can observe it.)
 * Parameter sets: ref, p-I, p-III (n = 1024 / 2048, as for poly_mul_ntt_k).
 * One kernel and one launch serve every batch size.  Asynchronous on `stream`.
 * Checks, in this order (the first defect decides; all of them run before any
 * GPU work):
 *   NTT_ERR_PARAM  param_set (unknown, or n > 2048); k outside
 *                  1 .. NTT_MUL_K_MAX; sgn or neg not 0 or 1; bits outside
 *                  poly_unpack's range for that sgn; stride not a multiple of
 *                  16 or < k n bits / 8; pstride < n or not a multiple of 4
 *   batch == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_out, d_in (d_max may be NULL)
 *   NTT_ERR_ALIGN  d_out and d_in 16-byte, d_max 4-byte when not NULL
 *   NTT_ERR_SIZE   batch * k > 2^31 - 1
 *   NTT_ERR_ALIAS  d_out's extent, ((batch k - 1) pstride + n) words, overlaps
 *                  the byte side's extent, (batch - 1) stride + k n bits / 8;
 *                  or d_max's batch k words overlap either.  Only extents are
 *                  compared: an output that lies in the gaps of another
 *                  pstride-strided buffer overlaps that buffer's extent, which
 *                  is not an operand and is not looked at. */
int poly_unpack_ntt(uint32_t *d_out, size_t pstride, uint32_t *d_max /* [batch][k] or NULL */,
                    const uint8_t *d_in, size_t stride, size_t batch, int k, int bits, int sgn,
                    int neg, int param_set, void *stream);

/* The logic between the steps of a chain, on the device: row tests, selection
 * and row moves.  With them a restart loop reruns only its rejected messages:
 * test the attempt's norms into flags (ntt_rows_over), list the accepted rows
 * and move their results out (ntt_select want 0, ntt_rows_move), list the
 * rejected rows, raise their nonces and gather their inputs into the next,
 * smaller batch (ntt_select want 1 with d_bump, ntt_rows_move) -- every other
 * entry point already takes any batch size and per-message nonces and keys.
 * The four know no parameter set and no scheme.  Indices and counts are data,
 * as d_key and d_off are: no value of either makes the device read or write
 * outside the extents stated below.  All four are asynchronous on `stream`,
 * never allocate, use no atomics, write every output word with a plain store
 * of the one thread that owns it, and no workgroup waits on another.
 * Checks, in this order unless an entry says otherwise (the first defect
 * decides; all before any GPU work): NTT_ERR_PARAM; batch == 0 (count == 0)
 * NTT_OK, nothing else is looked at and nothing is written; NTT_ERR_NULL;
 * NTT_ERR_ALIGN; NTT_ERR_SIZE (more than 2^31 - 1 rows); NTT_ERR_ALIAS.
 *
 * ntt_rows_over: a row of maxima against a row of bounds.
 *   d_vals [batch][m] uint32 (width 32) or uint64 (width 64); d_flag [batch]
 *   bounds [m] uint64 in HOST memory, read during the call (not kept)
 *   f_b = OR_j (d_vals[b][j] > bounds[j]), 0 or 1;
 *   d_flag[b] = accumulate ? d_flag[b] | f_b : f_b
 * A bound at or above the type's maximum never flags: that is how a column is
 * skipped (poly_round's norms are [batch][2]; the signer tests column 0 of z's,
 * and both columns of w's [batch][k][2] as m = 2 k with alternating bounds).
 * Width 64 is poly_hsum's sums.  With accumulate the other bits of d_flag[b]
 * are kept; a flag is "set" when it is not 0.
 *   NTT_ERR_PARAM  width not 32 / 64, m outside 1 .. NTT_ROWS_M_MAX, accumulate
 *                  not 0 / 1
 *   NTT_ERR_NULL   d_flag, d_vals, bounds
 *   NTT_ERR_ALIGN  d_flag 4-byte, d_vals width / 8
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_flag's batch words overlap d_vals' batch m width / 8 bytes */
#define NTT_ROWS_M_MAX 16
int ntt_rows_over(uint32_t *d_flag, const void *d_vals, int width, int m,
                  const uint64_t *bounds /* HOST, m entries, read during the call */,
                  int accumulate, size_t batch, void *stream);

/* ntt_rows_differ: the verifier's c'' == c' test.  f_b = 1 iff the row_bytes
 * bytes at d_a + b a_stride and at d_b + b b_stride differ anywhere, 0
 * otherwise; d_flag[b] as ntt_rows_over's, with the same accumulate.  The
 * strides let a field be read where it lies -- c' at d_sig + zlen with stride
 * zlen + 32 -- and bytes [row_bytes, stride) of a row are never read.
 *   NTT_ERR_PARAM  row_bytes not a multiple of 4 or below 4; a stride not a
 *                  multiple of 4 or below row_bytes; accumulate not 0 / 1
 *   NTT_ERR_NULL   d_flag, d_a, d_b
 *   NTT_ERR_ALIGN  any of the three not 4-byte aligned
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  d_flag's batch words overlap either input's extent,
 *                  (batch - 1) stride + row_bytes (the two inputs may overlap
 *                  each other) */
int ntt_rows_differ(uint32_t *d_flag, const uint8_t *d_a, size_t a_stride,
                    const uint8_t *d_b, size_t b_stride, size_t row_bytes,
                    int accumulate, size_t batch, void *stream);

/* ntt_select: flags to an ascending index list.  d_idx[0 .. c) is every b <
 * batch with (d_flag[b] != 0) == want, in ascending order, and d_count[0] = c;
 * the words d_idx[c .. batch) are not written.  d_bump is NULL or [batch]
 * uint32: d_bump[b] += 1 for exactly the selected b, in the same launch (the
 * rejected messages' nonces).  Ascending order is the contract: what a chain
 * computes for a message then does not depend on which other messages are
 * live.  One workgroup walks the flags and carries the running offset, so
 * there is no scratch memory and nothing to wait for; at 2^20 flags it streams
 * 4 MB through one compute unit (the time is in DESIGN.md section 5r).
 * batch == 0 writes nothing, d_count included.
 *   NTT_ERR_PARAM  want not 0 / 1
 *   NTT_ERR_NULL   d_idx, d_count, d_flag (d_bump may be NULL)
 *   NTT_ERR_ALIGN  any pointer not 4-byte aligned
 *   NTT_ERR_SIZE   batch > 2^31 - 1
 *   NTT_ERR_ALIAS  any two of d_idx's batch words, d_count's one word, d_flag's
 *                  batch words and d_bump's batch words overlap */
int ntt_select(uint32_t *d_idx, uint32_t *d_count, const uint32_t *d_flag,
               int want, uint32_t *d_bump, size_t batch, void *stream);

/* ntt_rows_move: gather and scatter whole rows by index, the count on the
 * device.  For i < min(count, d_count ? d_count[0] : count), with
 * si = d_src_idx ? d_src_idx[i] : i and di = d_dst_idx ? d_dst_idx[i] : i:
 * if si < src_rows and di < dst_rows, the row_bytes bytes at d_src + si
 * src_stride are copied to d_dst + di dst_stride; otherwise row i is skipped.
 * The skip is the definition, not an error path: no index and no count makes
 * the device read or write outside the two extents (rows - 1) stride +
 * row_bytes, and bytes [row_bytes, stride) of a d_dst row are never written.
 * Distinct di are the caller's duty (ntt_select's lists are distinct); with
 * equal di which row ends up there is not defined.  The launch is sized by the
 * host's count and trimmed by the device's, so a sub-batch moves before the
 * host knows its size.  With both index lists NULL it is a strided row copy.
 * Rows move in 16-byte accesses when both bases, both strides and row_bytes
 * are multiples of 16, in dwords otherwise.
 *   NTT_ERR_PARAM  row_bytes not a multiple of 4 or below 4; a stride not a
 *                  multiple of 4 or below row_bytes
 *   count == 0     NTT_OK, nothing else is looked at
 *   NTT_ERR_NULL   d_dst, d_src (each of d_dst_idx, d_src_idx, d_count may be
 *                  NULL)
 *   NTT_ERR_ALIGN  any pointer not 4-byte aligned
 *   NTT_ERR_SIZE   count, dst_rows or src_rows > 2^31 - 1
 *   NTT_ERR_ALIAS  d_dst's extent overlaps d_src's extent, an index list's count
 *                  words or d_count's word (compaction ping-pongs two buffers) */
int ntt_rows_move(uint8_t *d_dst, size_t dst_stride, const uint32_t *d_dst_idx, size_t dst_rows,
                  const uint8_t *d_src, size_t src_stride, const uint32_t *d_src_idx, size_t src_rows,
                  size_t row_bytes, const uint32_t *d_count, size_t count, void *stream);

/* Nussbaumer negacyclic product (the paper's alternate algorithm): the
 * reference's single-polynomial CPU routine nussbaumer_fft (NTT.cu:167-277,
 * driver test_nussbaumer :1987-2005), batched on the GPU and extended from
 * n = 1024 to n = param_set's n (1024 or 2048; split m = 32, r = n/32).
 *   ring NTT_RING_M32: coefficients mod 2^32 - 1, the reference's ring
 *                      (NTT.cu:102-134); any 32-bit input, 0xFFFFFFFF is
 *                      read as zero, outputs canonical in [0, 2^32 - 1).
 *   ring NTT_RING_Q:   coefficients mod param_set's q, inputs < 2q, outputs
 *                      canonical -- bit-identical to poly_mul.
 * d_c may alias d_a or d_b.  All three pointers must be 16-byte aligned. */
#define NTT_RING_Q 0
#define NTT_RING_M32 1
int poly_mul_nussbaumer(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b,
                        size_t batch, int param_set, int ring, void *stream);

/* Pointwise product c[i] = a[i] * b[i] mod q over batch*n coefficients.
 * Replaces pointwise_mult (NTT.cu:1155-1160).  Inputs < 2q, canonical output;
 * all three pointers must be 16-byte aligned; d_c may alias d_a or d_b. */
int poly_pointwise(uint32_t *d_c, const uint32_t *d_a, const uint32_t *d_b,
                   size_t batch, int param_set, void *stream);

/* Device-side counter-based generator: coefficient i of poly p gets
 * splitmix64(seed + (idx+1)*0x9E3779B97F4A7C15) mapped to [0,q) by
 * multiply-high, idx = (first_poly + p) * n + i.  Lets benchmarks build
 * multi-GiB inputs on the device; any poly can be regenerated on the host. */
int ntt_fill_uniform(uint32_t *d_poly, size_t batch, int param_set,
                     uint64_t seed, uint64_t first_poly, void *stream);

/* ---- host-buffer (streamed) operation --------------------------------- */
/* The reference times its GPU pipelines host -> host: synchronous H2D, the
 * kernel sequence and D2H on the default stream (NTT.cu:2384-2428; SURVEY.md
 * §8(f) row 4).  A context pipelines that in chunks of `chunk_polys`
 * polynomials (0 -> 4096) over three event-chained HIP queues (H2D copies,
 * kernels, D2H copies) and `nslots` buffer slots (0 -> 3, at most 8):
 * chunk i's D2H, chunk i+1's kernel and chunk i+2's H2D overlap.  Each slot
 * owns 3 device and 3 pinned host buffers of chunk_polys*n words, on the
 * device that is current at creation.  Pinned host buffers (ntt_host_alloc,
 * hipHostMalloc, registered memory) are DMA'd directly; pageable ones are
 * staged through the slots' pinned buffers by host memcpy.  The calls are
 * synchronous: on return the outputs are in host memory.  h_out may equal
 * an input (in place); other overlaps are undefined.  A context serves one
 * host thread at a time. */
typedef struct ntt_host_ctx ntt_host_ctx;
int ntt_host_ctx_create(ntt_host_ctx **ctx, int param_set, size_t chunk_polys, int nslots);
int ntt_host_ctx_destroy(ntt_host_ctx *ctx);
/* host -> host forward / inverse transform (poly_ntt_oop / poly_invntt_oop) */
int poly_ntt_host(ntt_host_ctx *ctx, uint32_t *h_out, const uint32_t *h_in, size_t batch);
int poly_invntt_host(ntt_host_ctx *ctx, uint32_t *h_out, const uint32_t *h_in, size_t batch);
/* host -> host fused negacyclic product (poly_mul) */
int poly_mul_host(ntt_host_ctx *ctx, uint32_t *h_c, const uint32_t *h_a, const uint32_t *h_b, size_t batch);
/* pinned host memory for the calls above (NULL on failure) */
void *ntt_host_alloc(size_t bytes);
void ntt_host_free(void *p);

/* Last HIP error code seen by this thread (hipError_t as int), and a
 * static string for an NTT_ERR_* code. */
int ntt_last_hip_error(void);
const char *ntt_strerror(int code);

/* Diagnostic: on the current device, the number of bounded waits of the
 * n = 8192 fused products' per-polynomial barriers that expired since the
 * library was loaded (synchronises the device; every other kernel runs one
 * wave per polynomial and has none).  Always 0 unless the hardware schedule
 * broke the barrier; a launch that raised it produced invalid output. */
int ntt_sync_expiries(uint32_t *count);

/* Small-batch switch: writes to *max_batch the largest batch for which
 * entry point `op` (NTT_OP_*) of `param_set` runs the small-batch kernels
 * (one polynomial per workgroup; 0 = never); larger batches
 * run the batch kernels.  All give identical results; the thresholds are the
 * measured crossovers of their launch times, per (n, op).  The reference
 * has one launch shape for every batch (<<<BATCH, T>>>, NTT.cu:2216). */
#define NTT_OP_FWD 0     /* poly_ntt (in place; also poly_ntt_oop with d_out == d_in) */
#define NTT_OP_INV 1     /* poly_invntt (in place; also poly_invntt_oop, d_out == d_in) */
#define NTT_OP_FWD_BR 2  /* poly_ntt_bitrev                                           */
#define NTT_OP_INV_BR 3  /* poly_invntt_bitrev                                        */
#define NTT_OP_MUL 4     /* poly_mul                                                  */
#define NTT_OP_MUL_NTT 5 /* poly_mul_ntt                                              */
#define NTT_OP_FWD_OOP 6 /* poly_ntt_oop, distinct buffers                            */
#define NTT_OP_INV_OOP 7 /* poly_invntt_oop, distinct buffers                         */
int ntt_small_batch_max(int param_set, int op, size_t *max_batch);
/* Which kernel family entry point `op` of `param_set` runs at `batch`
 * polynomials: *radix = 4 / 8 / 16 for the one-polynomial-per-workgroup
 * kernels with radix-4 / 8 / 16 passes, 0 for the batch
 * kernels.  Diagnostic; every family gives identical results. */
int ntt_small_batch_radix(int param_set, int op, size_t batch, int *radix);

/* Library / kernel description for reports, ending in "src=<16 hex>" (a hash
 * of the library sources): writes at most len bytes, returns the length. */
int ntt_build_info(char *buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* QTESLA_NTT_H */
