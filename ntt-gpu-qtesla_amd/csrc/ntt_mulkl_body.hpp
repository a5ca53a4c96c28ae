// ntt_mulkl_body.hpp -- the body of k_poly_mul_kl, k_poly_mul_kl_round and
// their keyed forms (ntt_mulkl.hpp), included into the four function
// definitions; not a header of its own.  It is text and not a function template because the code generated
// for k_poly_mul_kl depends on the names of the symbols inside it (the LDS
// array, the closure that inv_last_stage is instantiated with): moved into a
// shared device function, or with a fourth template parameter on the kernel,
// the same instructions come out in another order with other registers
// (DESIGN.md 5h).  Included like this, the existing kernels' assembly is
// unchanged.
//
// Expects in scope: PS, L, ADD (template parameters); in, ahat, add, npoly, k,
// ppw (kernel parameters); constexpr bool RND; uint32_t *out (RND off) and
// const RoundOut ro (RND on), the other one a dummy; constexpr bool KEYED and
// const KeySel ks (a dummy with KEYED off).
//
// KEYED: ahat is [nkeys][k][L][n] and the rows of a message are its key's, the
// index read once per work unit.  n = 2048: a wave is one message, the index is
// wave-uniform and stays in scalar registers.  n = 1024: the two half-waves are
// two messages and each lane takes its own polynomial's index; the invalid half
// of an odd batch's last unit takes the first polynomial's (Lane::load_poly), so
// no word of ks.key at or past npoly is read.  Either way the index is clamped
// to ks.last: no value of it takes a row load outside ahat.
//
// RND off: the row's canonical values are stored to `out`.  RND on: they are
// rounded where they are computed (round_coeff, ntt_round.hpp) and never reach
// memory.  A lane's 32 values lie S apart, so their hi bytes are staged through
// the wave's own transpose buffer -- free once lds_p2_to_p1 has read it, and
// touched by no other wave -- and leave as two 16-byte stores per lane; the two
// maxima are reduced across the wave (n = 2048) or the half-wave (n = 1024)
// that holds the polynomial, and its first lane stores the pair.  A row belongs
// to one wave in either launch shape, so every output byte and word is written
// once, by a plain vector store.
    using P = typename PSel<PS>::T;
    using LT = Lane<P>;
    constexpr int SWO = TW2_ENTRIES * 64;   // bit-5 pairs' offset (pairs)
    __shared__ __attribute__((aligned(16))) uint32_t lds[MULKL_LDS_WORDS];
    uint2 *ftw2 = reinterpret_cast<uint2 *>(lds + MULKL_WAVES * XPOSE_WORDS);
    uint2 *itw2 = ftw2 + TW2_WORDS / 2;
    fill_tw2<PS, false, MULKL_WG>(ftw2);
    fill_tw2<PS, true, MULKL_WG>(itw2);
    __syncthreads();
    const LT Ln;
    uint32_t *buf = lds + (threadIdx.x >> 6) * XPOSE_WORDS;

    const uint32_t nunits = (npoly + LT::UPW - 1) / LT::UPW;
    const uint32_t kn = k * P::N;   // words between two polynomials of out / add (<= 2^14)
    uint32_t u = blockIdx.x * (MULKL_WAVES * ppw) + wave_id();
    // KEYED, n = 1024: the index is per lane, so ks is kept in vector registers
    // for the whole walk -- three scalar registers more across the unit loop
    // spill one (ADD, RND off), and there are vector registers to spare
    [[maybe_unused]] KeySel kv = ks;
    if constexpr (KEYED && !LT::BIG) asm volatile("" : "+v"(kv.key), "+v"(kv.last));
#pragma unroll 1
    for (uint32_t it = 0; it < ppw; ++it, u += MULKL_WAVES) {   // dispatch-ordered chunk (see chunk_loop)
        if (u >= nunits) break;
        const bool valid = LT::BIG || Ln.poly(u) < npoly;
        uint32_t yh[L][32];
#pragma unroll
        for (int t = 0; t < L; ++t) {
            load32(yh[t], in.y[t] + LT::unit_base(u) + Ln.col_load(u, npoly), [](int j) { return LT::S * j; });
            fwd_pass1<PS, P>(yh[t], Ln.h, ftw2 + SWO + opaque_zero());
            // transpose addresses recomputed from an opaque lane here and in the
            // row loop: kept live across the unit they pin ~25 VGPRs (n = 2048: 7 spilled)
            lds_p1_to_p2<P>(yh[t], buf, LT(opaque_lane()));
            fwd_pass2<P>(yh[t], ftw2 + opaque_zero(), Ln.lane);
#pragma unroll
            for (int j = 0; j < 32; ++j) yh[t][j] = csub<P::Q2>(yh[t][j]);   // [0, 4q) -> [0, 2q), once for all rows
        }
        // out / add addressing as in k_poly_mul_k
        const size_t ubase = (size_t)u * LT::UPW * kn;
        const uint32_t ooff = LT::BIG ? Ln.brl : Ln.h * kn + Ln.brl;
        const uint32_t aoff = valid ? ooff : Ln.brl;
        size_t koff = 0;   // KEYED: words from ahat to the key's [k][L][n] block
        if constexpr (KEYED) {
            const uint32_t b = Ln.load_poly(u, npoly);   // < npoly
            uint32_t key = kv.key != nullptr ? kv.key[b] : b;
            if constexpr (LT::BIG) key = __builtin_amdgcn_readfirstlane(key);
            koff = (size_t)min(key, kv.last) * ((size_t)kn * L);
        }
#pragma unroll 1
        for (uint32_t i = blockIdx.y; i < k; i += gridDim.y) {
            const uint32_t *pa = ahat + (size_t)i * (L * P::N) + Ln.brl;   // row i: a_i0-hat .. a_i(L-1)-hat, n words each
            if constexpr (KEYED) pa += koff;
            uint32_t r[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                uint32_t yv[L], av[L];
#pragma unroll
                for (int t = 0; t < L; ++t) {
                    yv[t] = yh[t][j];
                    av[t] = csub<P::Q2>(pa[t * P::N + LT::S * brv5(j)]);   // a-hat < 2q
                }
                r[j] = mont_dot<P, L>(yv, av);
            }
            inv_pass2<P>(r, itw2 + opaque_zero(), Ln.lane);
            lds_p2_to_p1<P>(r, buf, LT(opaque_lane()));
            const size_t rbase = ubase + (size_t)i * P::N;
            uint32_t ad[ADD ? 32 : 1];
            if constexpr (ADD) load32(ad, add + rbase + aoff, [](int j) { return LT::S * j; });
            uint32_t *po = out + rbase + ooff;
            // RND: the polynomial's byte j * S + (lane in polynomial), the two
            // polynomials of an n = 1024 unit n bytes apart
            uint8_t *pb = reinterpret_cast<uint8_t *>(buf) + (LT::BIG ? Ln.lane : Ln.h * P::N + Ln.brl);
            uint32_t mc = 0, ml = 0;
            // stores interleaved with the last stage; with an addend the last
            // stage leaves [0, 2q) and the sum (< 4q) is reduced here
            auto emit = [&](int j, uint32_t v) {
                if constexpr (ADD) v = canon4<P>(v + ad[j]);
                if constexpr (RND) {
                    int32_t hi;
                    uint32_t ac, al;
                    round_coeff<P>(v, ro.d, hi, ac, al);
                    pb[LT::S * j] = (uint8_t)hi;
                    mc = max(mc, ac);
                    ml = max(ml, al);
                } else {
                    if (valid) st_out(po + LT::S * j, v);
                }
            };
            inv_pass1_head<P>(r, Ln.h, tw_base<PS, true>(), itw2 + SWO + opaque_zero());
            inv_last_scaled<P, !ADD, P::NINV_R, P::C1_R>(r, emit);
            if constexpr (RND) {
                // bytes [16 pl, 16 pl + 16) of each half of the polynomial; hi
                // is addressed like out, a byte per word
                const uint32_t pl = LT::BIG ? Ln.lane : Ln.brl;
                const uint32_t hoff = (LT::BIG ? 0u : Ln.h * P::N) + 16 * pl;
                compiler_fence();
                const uint8_t *sb = reinterpret_cast<const uint8_t *>(buf) + hoff;
                const uint4 b0 = *reinterpret_cast<const uint4 *>(sb);
                const uint4 b1 = *reinterpret_cast<const uint4 *>(sb + P::N / 2);
                compiler_fence();   // read before the next row's transpose overwrites it
                if (ro.hi != nullptr && valid) {
                    uint8_t *ph = ro.hi + rbase + (LT::BIG ? 0u : Ln.h * kn) + 16 * pl;
                    *reinterpret_cast<uint4 *>(ph) = b0;
                    *reinterpret_cast<uint4 *>(ph + P::N / 2) = b1;
                }
                if (ro.norms != nullptr) {
                    mc = lanes_max<LT::BIG ? 6 : 5>(mc);
                    ml = lanes_max<LT::BIG ? 6 : 5>(ml);
                    if (valid && pl == 0) ro.norms[(size_t)Ln.poly(u) * k + i] = make_uint2(mc, ml);
                }
            }
        }
    }
