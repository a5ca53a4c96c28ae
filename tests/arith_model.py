"""Model of the device arithmetic primitives of csrc/ntt_device.hpp,
ntt_mulkl.hpp and ntt_round.hpp, shared by tests/test_device_arith.py (CPU)
and tests/test_gpu_device_arith.py (the same primitives run on the GPU by
lib/libqtesla_ntt_arith.so, tools/arith_probe.hip).

Three things live here:

  * the scalar helpers (Python ints masked to 32 / 64 bits) that
    test_device_arith.py has always used, unchanged;
  * `model(prim, q, inputs, variant, mutant)`: every primitive restated
    instruction by instruction over numpy uint64 arrays that hold 32-bit words
    (64-bit sums wrap as the device's do), and the mutants the CPU tests use
    to show that the operand grid has teeth;
  * `grid(prim, q, variant, tw)`, the operand set (identical on CPU and GPU),
    and `check(prim, q, inputs, outputs, variant)`, the mathematical claim of
    each primitive (congruence mod q and the output interval its callers rely
    on) in exact integer arithmetic.

Operands and results are structure-of-arrays: a list of NIN / NOUT columns,
one entry per element, in the order the probe library takes them.
"""
import zlib

import numpy as np

PRIMES = {"ref": 8404993, "p-I": 343576577, "p-III": 856145921}
# (q, n, psi) of the three sets (csrc/pset.hpp; the n = 4096 / 8192 sets share p-III's prime)
SETS = {"ref": (8404993, 1024, 2083362),
        "p-I": (343576577, 1024, pow(3, (343576577 - 1) // 2048, 343576577)),
        "p-III": (856145921, 2048, pow(3, (856145921 - 1) // 4096, 856145921))}
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
MUL_LOGR = 3   # ntt_device.hpp


# --------------------------------------------------------------------------
# scalar helpers (Python ints), as test_device_arith.py has always had them
# --------------------------------------------------------------------------
def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def shoup(w, q):
    return (w << 32) // q


def centred(w, q):
    """csigned_tw (pset.hpp): ws in (-q/2, q/2], wps = floor(ws 2^32 / q)."""
    ws = w if w <= q // 2 else w - q
    return ws, (ws << 32) // q   # Python // floors, as the device constant does


def madlo32(a, b, c):
    return (a * b + c) & M32


def umulhi(a, b):
    return ((a & M32) * (b & M32)) >> 32


def sq_quot(y, wps):
    """e = floor((d * wps - 2^31) / 2^32), d and wps signed (v_mad_i64_i32)."""
    return ((s32(y) * s32(wps) - (1 << 31)) >> 32) & M32


def ct_bfly_t(x, y, w, q, red, xs, ys, yos):
    """ntt_device.hpp ct_bfly_t with the twiddle w in [0, q): returns (x', y')
    as 32-bit words.  Unsigned y: (2^32 - w, w'); signed y: (-ws, ws')."""
    if not red:
        a = x
    elif xs:
        a = min(x, (x + 2 * q) & M32)
    else:
        a = min(x, (x - 2 * q) & M32)
    if ys:
        ws, wps = centred(w, q)
        qe = sq_quot(y, wps & M32)
        tn = madlo32(qe, q, (y * ((-ws) & M32)) & M32)
    else:
        qe = umulhi(y, shoup(w, q))
        tn = madlo32(qe, q, (y * ((-w) & M32)) & M32)
    xo = (a - tn) & M32
    yo = (a + tn) & M32 if yos else (a + tn + 2 * q) & M32
    return xo, yo


def value(word, s):
    """the integer a word stands for: S form is signed"""
    return s32(word) if s else word


def samples(q, s, rng, k=400):
    """edge and random words of a U ([0, 4q)) or S ((-2q, 2q)) operand"""
    if s:
        edge = [0, 1, -1, q - 1, -(q - 1), q, -q, 2 * q - 1, -(2 * q - 1)]
        rnd = [rng.randrange(-2 * q + 1, 2 * q) for _ in range(k)]
    else:
        edge = [0, 1, q - 1, q, 2 * q - 1, 2 * q, 4 * q - 1]
        rnd = [rng.randrange(0, 4 * q) for _ in range(k)]
    return [v & M32 for v in edge + rnd]


def fwd_signed_table(q, psi, logn):
    """FwdSignedTw<P>: (-ws mod 2^32, wps) of psi^brv(k), k < 32"""
    out = []
    for k in range(32):
        e = int(format(k, f"0{logn}b")[::-1], 2)
        ws, wps = centred(pow(psi, e, q), q)
        out.append(((-ws) & M32, wps & M32))
    return out


def redc(c, q, qneg):
    m = (c * qneg) & M32
    return ((m * q + c) >> 32)


# --------------------------------------------------------------------------
# constants (pset.hpp, BaseMul's static bounds), from the definitions
# --------------------------------------------------------------------------
def set_of(q):
    return next(v for v in SETS.values() if v[0] == q)


def consts(q):
    """The per-set constants of PSet<> and the flags and bounds of
    BaseMul<P, MUL_LOGR>, in exact integer arithmetic.  The header computes
    the flags in double; none of the three primes is near a threshold."""
    _, n, psi = set_of(q)
    D = 1 << MUL_LOGR
    R = (1 << 32) % q
    ninv = pow(n, -1, q)
    c1 = ninv * pow(psi, -(n // 2), q) % q
    c = dict(Q=q, N=n, PSI=psi, QNEG=(-pow(q, -1, 1 << 32)) & M32, R=R, NINV=ninv, C1=c1,
             NINV_R=ninv * R % q, C1_R=c1 * R % q)
    c["NINV_R_SHORT"] = D * c["NINV_R"] % q   # ninv_r<MUL_LOGR>()
    c["C1_R_SHORT"] = D * c["C1_R"] % q       # c1_r<MUL_LOGR>()
    # CZ = (D + q / 2^32) q^2; OUT_CSUB_Z: CZ / 2^32 + q >= 2q
    c["CZ_NUM"] = (D * (1 << 32) + q) * q * q          # CZ * 2^32
    c["OUT_CSUB_Z"] = c["CZ_NUM"] >= q << 64
    c["AH"] = c["OUT_CSUB_Z"]
    # CZH = 2 D q^2, OUTH = CZH / 2^32 + q, WH = OUTH (- 2q when OUTH >= 2q)
    c["CZH"] = 2 * D * q * q
    c["OUT_CSUB_H"] = c["CZH"] >= q << 32
    c["WIDE"] = c["AH"] and c["CZH"] >= 3 * q << 32
    wh_num = c["CZH"] + (q << 32) - ((2 * q << 32) if c["OUT_CSUB_H"] else 0)   # WH * 2^32
    # BaseMul::run's outputs stay below max(2q, WH): the first inverse stage's domain
    c["WB_NUM"] = max(2 * q << 32, wh_num)
    c["WB"] = -(-c["WB_NUM"] >> 32)   # ceil: words below WB are exactly those below max(2q, WH)
    # REDC inputs the static_asserts admit: below CZ, or CZH with the half-canonical a
    c["C_ADMIT"] = max(-(-c["CZ_NUM"] >> 32), c["CZH"] if c["AH"] else 0)
    assert c["C_ADMIT"] + M32 * q <= M64
    return c


# --------------------------------------------------------------------------
# the primitives: name -> (probe id, NIN, NOUT, variants)
# --------------------------------------------------------------------------
CT_FORMS = [(False, False, False, True), (True, True, True, True), (True, True, True, False), (True, False, False, True),
            (True, False, False, False), (True, True, False, True), (True, True, False, False)]   # (RED, XS, YS, YOS)
PRIMS = {
    "csub_q": (0, 1, 1, 1), "csub_2q": (1, 1, 1, 1), "canon4": (2, 1, 1, 1), "bm_canon": (3, 1, 1, 2),
    "bm_half": (4, 1, 1, 2), "shoup_mul": (5, 3, 1, 1), "sshoup_mul": (6, 3, 1, 1), "ct_bfly_t": (7, 4, 2, len(CT_FORMS)),
    "gs_bfly": (8, 4, 2, 1), "mont_mul": (9, 2, 1, 1), "mont_dot1": (10, 2, 1, 1), "mont_dot2": (11, 4, 1, 1),
    "redc": (12, 2, 1, 1), "bm_run": (13, 66, 32, 2), "inv_wide0": (14, 34, 32, 1), "inv_last": (15, 32, 64, 4),
    "round_coeff": (16, 2, 3, 1),
}
CASES = [(p, v) for p, spec in PRIMS.items() for v in range(spec[3])]
MUTANTS = {   # mutant -> a (primitive, variant) on which check must reject it
    "mont_carry_one": [("mont_mul", 0), ("mont_dot1", 0), ("mont_dot2", 0)],
    "squot_floor": [("sshoup_mul", 0), ("gs_bfly", 0), ("ct_bfly_t", 1)],
    "shoup_minus_one": [("shoup_mul", 0)],
    "xs_unsigned": [("ct_bfly_t", 1), ("ct_bfly_t", 5)],
    "no_bias": [("ct_bfly_t", 2), ("ct_bfly_t", 4), ("ct_bfly_t", 6)],
    "round_centre_ge": [("round_coeff", 0)],
    "round_tie_ge": [("round_coeff", 0)],
}

U64 = np.uint64
_M32 = U64(M32)


def _w(a):
    """words as uint64"""
    return np.asarray(a).astype(U64) & _M32


def _i(a):
    """words as int64 (unsigned value)"""
    return np.asarray(a).astype(np.int64) & np.int64(M32)


def _s(a):
    """words as int64, read as signed 32-bit values"""
    v = _i(a)
    return (v ^ np.int64(1 << 31)) - np.int64(1 << 31)


def _c(v):
    return U64(v & M32)


# ---- vector model: 32-bit words in uint64 ----------------------------------
def v_add(a, b):
    return (a + b) & _M32


def v_sub(a, b):
    return (a - b) & _M32   # uint64 wraps mod 2^64, the mask leaves the difference mod 2^32


def v_mullo(a, b):
    return (a * b) & _M32   # a, b < 2^32: the product is exact in 64 bits


def v_umulhi(a, b):
    return (a * b) >> U64(32)


def v_madlo32(a, b, c):
    return (a * b + c) & _M32   # (2^32 - 1)^2 + 2^32 - 1 < 2^64


def v_csub(x, C):
    return np.minimum(x, v_sub(x, _c(C)))


def v_squot(d, wps, mutant=None):
    p = _s(d) * _s(wps)   # |.| < 2^62
    if mutant != "squot_floor":
        p = p - np.int64(1 << 31)
    return (p >> np.int64(32)).astype(U64) & _M32


def v_shoup_mul(a, w, wp, q, mutant=None):
    if mutant == "shoup_minus_one":
        wp = v_sub(wp, U64(1))
    return v_madlo32(v_umulhi(a, wp), _c(-q), v_mullo(a, w))


def v_sshoup_mul(d, ws, wps, q, mutant=None):
    return v_madlo32(v_squot(d, wps, mutant), _c(-q), v_mullo(d, ws))


def v_ct_bfly_t(x, y, wn, wp, q, red, xs, ys, yos, mutant=None):
    if not red:
        a = x
    elif xs and mutant != "xs_unsigned":
        a = np.minimum(x, v_add(x, _c(2 * q)))
    else:
        a = v_csub(x, 2 * q)
    qe = v_squot(y, wp, mutant) if ys else v_umulhi(y, wp)
    tn = v_madlo32(qe, _c(q), v_mullo(y, wn))
    xo = v_sub(a, tn)
    yo = v_add(a, tn)
    if not yos and mutant != "no_bias":
        yo = v_add(yo, _c(2 * q))
    return xo, yo


def v_gs_bfly(x, y, ws, wps, q, mutant=None):
    return v_csub(v_add(x, y), 2 * q), v_sshoup_mul(v_sub(x, y), ws, wps, q, mutant)


def _mont_tail(hi, lo, q, qneg, mutant):
    m = v_mullo(lo, _c(qneg))
    carry = U64(1) if mutant == "mont_carry_one" else (lo != 0).astype(U64)
    return (hi + v_umulhi(m, _c(q)) + carry) & _M32


def v_mont_mul(a, b, q, qneg, mutant=None):
    return _mont_tail(v_umulhi(a, b), v_mullo(a, b), q, qneg, mutant)


def v_mont_dot(ys, as_, q, qneg, mutant=None):
    L = len(ys)
    t = ys[0] * as_[0]
    for k in range(1, L):
        t = t + ys[k] * as_[k]   # static_assert: the sum fits 64 bits
    v = _mont_tail(t >> U64(32), t & _M32, q, qneg, mutant)
    return v if 4 * L * q < 1 << 32 else v_csub(v, 2 * q)


def v_redc(c, q, qneg):
    """c: uint64, the full 64-bit value; (m q + c) wraps as the device's does"""
    m = v_mullo(c & _M32, _c(qneg))
    return (m * U64(q) + c) >> U64(32)


def v_canon4(x, q):
    return v_csub(v_csub(x, 2 * q), q)


def v_bm_canon(s, x, q):
    return v_csub(np.minimum(x, v_add(x, _c(2 * q))), q) if s else v_canon4(x, q)


def v_bm_half(s, x, q):
    return np.minimum(x, v_add(x, _c(2 * q))) if s else v_csub(x, 2 * q)


def v_bm_run(ra, rb, wn, wp, q, odd_s):
    """BaseMul<P, MUL_LOGR>::run_zsplit; both residue pairs read the same (wn, wp)"""
    C = consts(q)
    D, R, qneg = 1 << MUL_LOGR, C["R"], C["QNEG"]
    tn = v_madlo32(v_umulhi(_c(R), wp), _c(q), v_mullo(_c(R), wn))
    zr = (np.minimum(v_sub(U64(0), tn), v_sub(_c(-q), tn)), np.minimum(v_add(tn, _c(q)), v_add(tn, _c(2 * q))))
    out = [None] * 32
    out_csub = C["OUT_CSUB_H"] if C["AH"] else C["OUT_CSUB_Z"]
    for g in range(32 // D):
        s = odd_s and bool(g & 1)
        z = zr[g & 1]
        a = [(v_bm_half if C["AH"] else v_bm_canon)(s, ra[D * g + i], q) for i in range(D)]
        b = [v_bm_canon(s, rb[D * g + i], q) for i in range(D)]
        for k in range(D):
            c = np.zeros_like(a[0])
            for i in range(k + 1):
                c = c + a[i] * b[k - i]
            if k < D - 1:
                hs = np.zeros_like(a[0])
                for i in range(k + 1, D):
                    hs = hs + a[i] * b[k + D - i]
                c = c + z * v_redc(hs, q, qneg)
            r = v_redc(c, q, qneg) & _M32
            out[D * g + k] = v_csub(r, 2 * q) if out_csub else r
    return out


def v_inv_wide0(r, ws, wps, q):
    """inv_pass2<P, 4, true>: the stage on pos bit 4, pairs (j, j + 16), WIDE0 form"""
    out = [None] * 32
    for j in range(16):
        x, y = r[j], r[j + 16]
        sm = v_add(x, y)
        out[j] = np.minimum(np.minimum(sm, v_sub(sm, _c(2 * q))), v_sub(sm, _c(4 * q)))
        out[j + 16] = v_sshoup_mul(v_sub(x, y), ws, wps, q)
    return out


def inv_last_consts(q, variant):
    """(S0, S1, CANON) of inv_last_stage's probe variant: CANON = bit 0, bit 1
    selects the constants of the inverse that runs MUL_LOGR stages short"""
    C = consts(q)
    short = bool(variant & 2)
    return (C["NINV_R_SHORT"] if short else C["NINV_R"]), (C["C1_R_SHORT"] if short else C["C1_R"]), bool(variant & 1)


def v_inv_last(r, q, variant):
    s0, s1, canon = inv_last_consts(q, variant)
    s0p = shoup(s0, q)
    s1w, s1p = centred(s1, q)
    out = [None] * 32
    for j in range(16):
        x, y = r[j], r[j + 16]
        a = v_shoup_mul(v_add(x, y), _c(s0), _c(s0p), q)
        b = v_sshoup_mul(v_sub(x, y), _c(s1w), _c(s1p), q)
        out[j] = v_csub(a, q) if canon else a
        out[j + 16] = v_csub(b, q) if canon else b
    return out + out   # the registers, then what the emit callback saw


def v_round_coeff(x, d, q, mutant=None):
    H = (q - 1) // 2
    over = (x >= U64(H)) if mutant == "round_centre_ge" else (x > U64(H))
    c = np.where(over, v_sub(x, _c(q)), x)
    two_d = (U64(1) << d) & _M32
    t = c & v_sub(two_d, U64(1))
    bias = two_d >> U64(1) if mutant == "round_tie_ge" else v_sub(two_d >> U64(1), U64(1))
    hi = ((_s(c) + _s(bias)) >> d.astype(np.int64)).astype(U64) & _M32
    return hi, np.minimum(x, v_sub(_c(q), x)), np.minimum(t, v_sub(two_d, t))


def model(prim, q, inputs, variant=0, mutant=None):
    """The primitive's result words (a list of NOUT uint64 columns), as the
    device code computes them; `mutant` names one deliberate error."""
    a = [_w(c) for c in inputs]
    qneg = consts(q)["QNEG"]
    with np.errstate(over="ignore"):
        if prim == "csub_q":
            return [v_csub(a[0], q)]
        if prim == "csub_2q":
            return [v_csub(a[0], 2 * q)]
        if prim == "canon4":
            return [v_canon4(a[0], q)]
        if prim == "bm_canon":
            return [v_bm_canon(bool(variant), a[0], q)]
        if prim == "bm_half":
            return [v_bm_half(bool(variant), a[0], q)]
        if prim == "shoup_mul":
            return [v_shoup_mul(a[0], a[1], a[2], q, mutant)]
        if prim == "sshoup_mul":
            return [v_sshoup_mul(a[0], a[1], a[2], q, mutant)]
        if prim == "ct_bfly_t":
            return list(v_ct_bfly_t(a[0], a[1], a[2], a[3], q, *CT_FORMS[variant], mutant))
        if prim == "gs_bfly":
            return list(v_gs_bfly(a[0], a[1], a[2], a[3], q, mutant))
        if prim == "mont_mul":
            return [v_mont_mul(a[0], a[1], q, qneg, mutant)]
        if prim == "mont_dot1":
            return [v_mont_dot(a[:1], a[1:], q, qneg, mutant)]
        if prim == "mont_dot2":
            return [v_mont_dot(a[:2], a[2:], q, qneg, mutant)]
        if prim == "redc":
            return [v_redc(a[0] | (a[1] << U64(32)), q, qneg) & _M32]
        if prim == "bm_run":
            return v_bm_run(a[:32], a[32:64], a[64], a[65], q, bool(variant))
        if prim == "inv_wide0":
            return v_inv_wide0(a[:32], a[32], a[33], q)
        if prim == "inv_last":
            return v_inv_last(a, q, variant)
        if prim == "round_coeff":
            return list(v_round_coeff(a[0], a[1], q, mutant))
    raise KeyError(prim)


# --------------------------------------------------------------------------
# the operand grid
# --------------------------------------------------------------------------
NRANDOM = 1 << 18      # random tuples per primitive
# The edge tuples meet every twiddle, the whole Phi / invPhi tables included
# (the largest case, a typed butterfly of p-III, is 729 edge pairs x 4167
# twiddles = 3.0 M tuples, well under a second on either side).  Only the
# register-set forms, whose element is 32 or 64 coefficients, keep the fixed
# twiddles and a seeded sample of TABLE_SAMPLE table entries.
TABLE_SAMPLE = 256
PRODUCT_MAX = 1 << 22


def _rng(prim, q, variant, salt=0):
    return np.random.default_rng([zlib.crc32(prim.encode()), q, variant, salt])


def boundaries(q, lo, hi):
    """the interval ends every lazy bound is made of, mirrored for a signed (S-form) domain"""
    pts = [0, q, 2 * q, 3 * q, 4 * q, 1 << 31, 1 << 32]
    if lo < 0:
        pts += [-p for p in pts]
    return pts


def edge_values(q, lo, hi):
    """every value within +-2 of a boundary that lies in [lo, hi), and (q -+ 1) / 2"""
    pts = boundaries(q, lo, hi)
    mids = [(q - 1) // 2, (q + 1) // 2]
    if lo < 0:
        mids += [-m for m in mids]
    vals = {p + d for p in pts for d in range(-2, 3)} | set(mids)
    return np.array(sorted(v for v in vals if lo <= v < hi), dtype=np.int64)


def random_values(rng, q, lo, hi, k):
    """k values of [lo, hi): half uniform, half within +-64 of a boundary"""
    uni = rng.integers(lo, hi, k // 2, dtype=np.int64)
    pts = np.array([p for p in boundaries(q, lo, hi) if lo - 64 <= p <= hi + 64], dtype=np.int64)
    near = rng.choice(pts, k - k // 2) + rng.integers(-64, 65, k - k // 2, dtype=np.int64)
    near = np.where(near < lo, 2 * lo - 1 - near, near)   # mirrored into the domain, not piled up on its ends
    near = np.where(near >= hi, 2 * hi - 1 - near, near)
    out = np.concatenate([uni, np.clip(near, lo, hi - 1)])
    return out[rng.permutation(k)]


def words(v):
    return (np.asarray(v, dtype=np.int64) & np.int64(M32)).astype(U64)


def twiddle_set(q, phi, invphi):
    """{'fixed': the named twiddles and 64 seeded random ones, 'table': every
    entry of the library's Phi and invPhi tables}, values in [0, q)"""
    fixed = [1, 2, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2, (q + 3) // 2]
    rnd = np.random.default_rng([q, 0x7717]).integers(0, q, 64, dtype=np.int64)
    table = np.unique(np.concatenate([np.asarray(phi, dtype=np.int64), np.asarray(invphi, dtype=np.int64)]))
    assert table.min() >= 0 and table.max() < q
    return {"fixed": np.concatenate([np.array(fixed, dtype=np.int64), rnd]), "table": table}


def model_tables(q):
    """Phi[i] = psi^i and invPhi[i] = n^-1 psi^-i of ntt_get_tables, from the
    definitions (test_device_arith.py checks them against the library's)"""
    _, n, psi = set_of(q)
    ninv, ipsi = pow(n, -1, q), pow(psi, -1, q)
    phi, inv, a, b = [], [], 1, ninv
    for _ in range(n):
        phi.append(a)
        inv.append(b)
        a, b = a * psi % q, b * ipsi % q
    return np.array(phi, dtype=np.int64), np.array(inv, dtype=np.int64)


def _tw_values(tw, nedge, rng):
    """the twiddles the edge tuples are multiplied with: all of them, or, where
    that product would pass PRODUCT_MAX tuples, the fixed ones and a seeded
    sample of TABLE_SAMPLE table entries (never fewer edges)"""
    table = tw["table"]
    if nedge * (len(tw["fixed"]) + len(table)) > PRODUCT_MAX:
        table = rng.choice(table, TABLE_SAMPLE, replace=False)
    return np.concatenate([tw["fixed"], table])


def tw_pair(w, q, kind):
    """twiddle values -> the (x, y) words of the device's pair:
    'shoup' (w, w'), 'fwd' (-w, w'), 'signed' (ws, ws'), 'fwd_signed' (-ws, ws')"""
    w = np.asarray(w, dtype=np.int64)
    if kind in ("shoup", "fwd"):
        wp = (w.astype(U64) << U64(32)) // U64(q)
        return (words(w) if kind == "shoup" else words(-w)), wp
    ws = np.where(w <= q // 2, w, w - q)
    wps = (ws << np.int64(32)) // np.int64(q)   # |ws| < 2^29: exact in int64; // floors
    return (words(ws) if kind == "signed" else words(-ws)), words(wps)


def _product(*cols):
    mesh = np.meshgrid(*cols, indexing="ij")
    return [m.ravel() for m in mesh]


def _domains(prim, q, variant):
    """[lo, hi) of each word operand"""
    if prim == "csub_q":
        return [(0, 2 * q)]
    if prim in ("csub_2q", "canon4"):
        return [(0, 4 * q)]
    if prim in ("bm_canon", "bm_half"):
        return [(-2 * q + 1, 2 * q) if variant else (0, 4 * q)]
    if prim == "shoup_mul":
        return [(0, 1 << 32)]
    if prim == "sshoup_mul":
        return [(-(1 << 31) + 1, 1 << 31)]
    if prim == "ct_bfly_t":
        red, xs, ys, _ = CT_FORMS[variant]
        dx = (0, 2 * q) if not red else (-2 * q + 1, 2 * q) if xs else (0, 4 * q)
        return [dx, (-2 * q + 1, 2 * q) if ys else (0, 4 * q)]
    if prim in ("gs_bfly", "mont_mul", "mont_dot1", "inv_last"):
        return [(0, 2 * q)] * 2
    if prim == "mont_dot2":
        return [(0, 2 * q)] * 4
    if prim == "inv_wide0":
        return [(0, consts(q)["WB"])] * 2
    raise KeyError(prim)


TW_KIND = {"shoup_mul": "shoup", "sshoup_mul": "signed", "gs_bfly": "signed", "inv_wide0": "signed", "bm_run": "fwd"}


def _tw_kind(prim, variant):
    if prim == "ct_bfly_t":
        return "fwd_signed" if CT_FORMS[variant][2] else "fwd"
    return TW_KIND.get(prim)


def mont_zero_low(q):
    """non-zero pairs (a, b) below 2q whose product is 0 mod 2^32"""
    a, b = [], []
    for k in range(8, 25):            # 2^k 2^(32-k), both below 2^24 < 2q of every prime
        for u, v in ((1, 1), (3, 1), (1, 5), (3, 7)):
            if u << k < 2 * q and v << (32 - k) < 2 * q:
                a.append(u << k)
                b.append(v << (32 - k))
    for u in (1, 2, 3, 127, 255):     # u 2^16 times v 2^16
        for v in (1, 5, 128, 255):
            a.append(u << 16)
            b.append(v << 16)
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)


def dot2_zero_low(q):
    """(y0, y1, a0, a1) below 2q, non-zero, with y0 a0 + y1 a1 = 0 mod 2^32 and
    neither product 0 mod 2^32: u 2^16 * v + 2^16 * (2^16 - u v mod 2^16)"""
    rows = []
    for u in range(1, 256, 7):
        for v in (1, 3, 0x1235, 0xFFFF, 0x10001, 0x7FFFFF):
            rest = (-(u * v)) % (1 << 16)
            if rest:
                rows.append((u << 16, 1 << 16, v, rest))
    za, zb = mont_zero_low(q)   # and both products 0 mod 2^32
    rows += [(int(za[i]), int(za[-1 - i]), int(zb[i]), int(zb[-1 - i])) for i in range(len(za))]
    r = np.array(rows, dtype=np.int64)
    assert r.max() < 2 * q and ((r[:, 0] * r[:, 2] + r[:, 1] * r[:, 3]) % (1 << 32) == 0).all()
    return [r[:, c] for c in range(4)]


def aim_twiddles(q, tw):
    """the fixed twiddles and those whose Shoup companion truncates most and
    least: beta = w 2^32 mod q in {q-1 .. q-4, 1 .. 4}"""
    rinv = pow((1 << 32) % q, -1, q)
    return [int(w) for w in tw["fixed"]] + [b * rinv % q for b in (q - 1, q - 2, q - 3, q - 4, 1, 2, 3, 4)]


def aimed_unsigned(q, ws, top):
    """(a, w) with a < top at which the lazy Shoup product sits as high in [0, 2q)
    as can be arranged: with beta = w 2^32 mod q, floor(a w' / 2^32) is one below
    floor(a w / q) exactly when a w mod q < a beta / 2^32, and then the product
    is (a w mod q) + q.  For r just below (top - q) beta / 2^32 and the largest
    a < top with a w = r (mod q) (so a >= top - q) that holds, and the product
    is r + q, within q beta / 2^32 of the most any a < top can reach."""
    out = []
    for w in ws:
        if w == 0:
            continue
        beta, winv = (w << 32) % q, pow(w, -1, q)
        for delta in range(3):
            r = ((top - q) * beta >> 32) - 1 - delta
            if r >= 0:
                a0 = r * winv % q
                out.append((a0 + (top - 1 - a0) // q * q, w))
    return out


def aimed_signed(q, ws, top):
    """(d, w) with |d| < top at which the signed Shoup product sits near the two
    ends of (0, 2q).  d ws = k q + r, gamma = ws 2^32 mod q: the quotient is k - 1
    (product r + q) when r < q / 2 + d gamma / 2^32 and k (product r) otherwise.
    High end: d near top, r just below q / 2 + (top - q) gamma / 2^32; low end:
    d near -top, r just above q / 2 - (top - q) gamma / 2^32."""
    out = []
    for w in ws:
        cs, _ = centred(w, q)
        if cs == 0:
            continue
        gamma, winv = (cs << 32) % q, pow(cs % q, -1, q)
        for delta in range(3):
            r = min((q * (1 << 31) + (top - q) * gamma >> 32) - 1, q - 1) - delta
            if 0 < r:
                d0 = r * winv % q
                out.append((d0 + (top - 1 - d0) // q * q, w))
            r = -(((top - q) * gamma - q * (1 << 31)) >> 32) + delta
            if 0 < r < q:
                d0 = r * winv % q
                out.append((d0 - (d0 + top - 1) // q * q, w))
    return out


def _aimed_columns(prim, q, variant, tw, edges):
    """the aimed tuples of a primitive as operand columns and twiddle values, or None"""
    ws = aim_twiddles(q, tw)
    if prim == "shoup_mul":
        a, w = zip(*aimed_unsigned(q, ws, 1 << 32))
        return [np.array(a, dtype=np.int64)], np.array(w, dtype=np.int64)
    if prim == "sshoup_mul":
        d, w = zip(*aimed_signed(q, ws, 1 << 31))
        return [np.array(d, dtype=np.int64)], np.array(w, dtype=np.int64)
    if prim == "gs_bfly":     # d = x - y with x, y in [0, 2q), from both ends of the square
        d, w = (np.array(c, dtype=np.int64) for c in zip(*aimed_signed(q, ws, 2 * q)))
        x = np.concatenate([np.maximum(d, 0), np.minimum(d, 0) + 2 * q - 1])
        y = np.concatenate([np.maximum(-d, 0), np.minimum(d, 0) + 2 * q - 1 - d])
        return [x, y], np.concatenate([w, w])
    if prim == "ct_bfly_t":   # the aimed y with every edge word of x
        ys = CT_FORMS[variant][2]
        y, w = (np.array(c, dtype=np.int64) for c in zip(*(aimed_signed(q, ws, 2 * q) if ys else aimed_unsigned(q, ws, 4 * q))))
        xi, yi = _product(np.arange(len(edges[0])), np.arange(len(y)))
        return [edges[0][xi], y[yi]], w[yi]
    return None


def _pack_sets(cols, per_set, fill=0):
    """flat per-tuple columns -> [len(cols)][per_set] columns of register sets,
    the last set padded with `fill`"""
    n = len(cols[0])
    nset = -(-n // per_set)
    out = []
    for c in cols:
        p = np.full(nset * per_set, fill, dtype=np.int64)
        p[:n] = c
        out.append(p.reshape(nset, per_set))
    return out


def _grid_pairs_sets(prim, q, variant, tw, rng):
    """inv_wide0 / inv_last: register sets whose 16 pairs (j, j + 16) carry the
    edge pairs (per twiddle) and NRANDOM random pairs"""
    (lo, hi), _ = _domains(prim, q, variant)
    e = edge_values(q, lo, hi)
    ex, ey = _product(e, e)
    X, Y = _pack_sets([ex, ey], 16)                     # [nset][16]
    nrand = NRANDOM // 16
    rx = random_values(rng, q, lo, hi, NRANDOM).reshape(nrand, 16)
    ry = random_values(rng, q, lo, hi, NRANDOM).reshape(nrand, 16)
    if prim == "inv_last":
        regs = np.concatenate([np.concatenate([X, Y], axis=1), np.concatenate([rx, ry], axis=1)])
        return [words(regs[:, j]) for j in range(32)]
    tws = _tw_values(tw, len(ex), rng)
    nset = X.shape[0]
    regs = np.concatenate([np.tile(np.concatenate([X, Y], axis=1), (len(tws), 1)), np.concatenate([rx, ry], axis=1)])
    w = np.concatenate([np.repeat(tws, nset), rng.choice(np.concatenate([tw["fixed"], tw["table"]]), nrand)])
    return [words(regs[:, j]) for j in range(32)] + list(tw_pair(w, q, "signed"))


def _grid_bm_run(q, variant, tw, rng):
    """register sets of BaseMul::run: constant fills, S-form extremes in the odd
    residues when ODD_S, single non-zero entries, each with every zeta of the
    (sampled) twiddle set, and NRANDOM / 32 random sets with random zeta"""
    odd_s = bool(variant)
    D = 1 << MUL_LOGR
    odd = (np.arange(32) // D) & 1 == 1
    sets_a, sets_b = [], []

    def fill(ve, vo, we=None, wo=None):
        sets_a.append(np.where(odd, vo, ve))
        sets_b.append(np.where(odd, vo if wo is None else wo, ve if we is None else we))

    for v in (0, 1, q - 1, q, 2 * q - 1, 2 * q, 4 * q - 1):
        fill(v, (v if v < 2 * q else 2 * q - 1) if odd_s else v)
    if odd_s:
        for v in (-1, -(q - 1), -q, -(2 * q - 1)):
            fill(4 * q - 1, v)
            fill(4 * q - 1, v, 2 * q - 1, 2 * q - 1)   # b of the other sign
    fill(4 * q - 1, 2 * q - 1 if odd_s else 4 * q - 1, q - 1, q - 1)
    for i in range(D):
        for j in range(D):
            for v in ((q - 1,) if not odd_s else (q - 1, -(q - 1))):
                a, b = np.zeros(32, dtype=np.int64), np.zeros(32, dtype=np.int64)
                a[i::D] = q - 1
                b[j::D] = q - 1
                a[odd], b[odd] = np.where(a[odd] != 0, v, 0), np.where(b[odd] != 0, -v if odd_s else v, 0)
                sets_a.append(a)
                sets_b.append(b)
    A, B = np.array(sets_a), np.array(sets_b)
    tws = _tw_values(tw, PRODUCT_MAX, rng)   # always the sample: a set is 32 coefficients
    nrand = NRANDOM // 32
    ra = random_values(rng, q, 0, 4 * q, nrand * 32).reshape(nrand, 32)
    rb = random_values(rng, q, 0, 4 * q, nrand * 32).reshape(nrand, 32)
    if odd_s:
        ra[:, odd] = random_values(rng, q, -2 * q + 1, 2 * q, nrand * 16).reshape(nrand, 16)
        rb[:, odd] = random_values(rng, q, -2 * q + 1, 2 * q, nrand * 16).reshape(nrand, 16)
    ra = np.concatenate([np.tile(A, (len(tws), 1)), ra])
    rb = np.concatenate([np.tile(B, (len(tws), 1)), rb])
    w = np.concatenate([np.repeat(tws, len(A)), rng.choice(np.concatenate([tw["fixed"], tw["table"]]), nrand)])
    return [words(ra[:, j]) for j in range(32)] + [words(rb[:, j]) for j in range(32)] + list(tw_pair(w, q, "fwd"))


def _grid_round(q, rng):
    ds = np.arange(1, 31, dtype=np.int64)
    xs, dd = _product(edge_values(q, 0, q), ds)
    H = (q - 1) // 2
    ex, ed = [], []
    for d in range(1, 31):
        h = 1 << (d - 1)
        for c in (h, -h, h + 1, -(h + 1), h - 1, -(h - 1), H, -H, 3 * h, -3 * h, 3 * h + 1, -(3 * h - 1)):
            if abs(c) <= H:
                ex.append(c % q)
                ed.append(d)
    rx = random_values(rng, q, 0, q, NRANDOM)
    rd = rng.integers(1, 31, NRANDOM, dtype=np.int64)
    # half of the random x: a multiple of 2^d plus the tie, within +-2
    k = NRANDOM // 2
    hd = np.int64(1) << (rd[:k] - 1)
    c = (rng.integers(-H, H + 1, k, dtype=np.int64) >> rd[:k] << rd[:k]) + hd + rng.integers(-2, 3, k, dtype=np.int64)
    rx[:k] = np.where(np.abs(c) <= H, c % q, rx[:k])
    return [words(np.concatenate([xs, np.array(ex, dtype=np.int64), rx])),
            words(np.concatenate([dd, np.array(ed, dtype=np.int64), rd]))]


def _grid_redc(q, rng):
    C = consts(q)
    top = C["C_ADMIT"]
    pts = [0, 1 << 32, q << 32, top - 1, top >> 1, q * q, 4 * q * q, (1 << 63) if top > 1 << 63 else top >> 2]
    vals = {p + d for p in pts for d in range(-2, 3)}
    vals |= {(h << 32) + lo for h in (0, 1, q - 1, q, top >> 32) for lo in (0, 1, M32 - 1, M32)}
    vals = sorted(v for v in vals if 0 <= v < top)
    hi_top = top >> 32
    rh = rng.integers(0, hi_top, NRANDOM, dtype=np.int64)          # below top whatever the low word
    rl = rng.integers(0, 1 << 32, NRANDOM, dtype=np.int64)
    rl[: NRANDOM // 4] = np.clip(rng.integers(-64, 65, NRANDOM // 4), 0, None)          # low word near 0
    rl[NRANDOM // 4: NRANDOM // 2] = M32 - np.clip(rng.integers(-64, 65, NRANDOM // 4), 0, None)   # near 2^32
    lo = np.concatenate([np.array([v & M32 for v in vals], dtype=np.int64), rl])
    hi = np.concatenate([np.array([v >> 32 for v in vals], dtype=np.int64), rh])
    return [words(lo), words(hi)]


def grid(prim, q, variant=0, tw=None):
    """The operand columns (uint64 holding 32-bit words) of a primitive: the
    edge words of its domain in full Cartesian product with each other and with
    the twiddles, the primitive's own coincidences (a zero low word, the
    rounding's ties, operands aimed at the ends of a lazy product's interval),
    and NRANDOM seeded random tuples, half uniform over the domain and half
    near its boundaries.  `tw`:
    twiddle_set(...) of the library's tables (default: model_tables)."""
    rng = _rng(prim, q, variant)
    if tw is None:
        tw = twiddle_set(q, *model_tables(q))
    if prim == "round_coeff":
        return _grid_round(q, rng)
    if prim == "redc":
        return _grid_redc(q, rng)
    if prim == "bm_run":
        return _grid_bm_run(q, variant, tw, rng)
    if prim in ("inv_wide0", "inv_last"):
        return _grid_pairs_sets(prim, q, variant, tw, rng)
    doms = _domains(prim, q, variant)
    edges = [edge_values(q, lo, hi) for lo, hi in doms]
    if prim == "mont_dot2":
        # (y0, y1, a0, a1): the full product of the edges in (y0, a0) while (y1, a1) walk the same edges out of
        # step; the same product in (y1, a1) beside a zero first term; the sums that are 0 mod 2^32
        y0, a0 = _product(edges[0], edges[0])
        zero = np.zeros_like(y0)
        parts = [(y0, np.roll(y0, 7), a0, np.roll(a0[::-1], 3)), (zero, y0, zero, a0), dot2_zero_low(q)]
        cols = [np.concatenate([p[c] for p in parts]) for c in range(4)]
    else:
        cols = _product(*edges)
        if prim in ("mont_mul", "mont_dot1"):
            za, zb = mont_zero_low(q)
            cols = [np.concatenate([cols[0], za, zb]), np.concatenate([cols[1], zb, za])]
    rnd = [random_values(rng, q, lo, hi, NRANDOM) for lo, hi in doms]
    kind = _tw_kind(prim, variant)
    if kind is None:
        return [words(np.concatenate([c, r])) for c, r in zip(cols, rnd)]
    tws = _tw_values(tw, len(cols[0]), rng)
    idx, tidx = _product(np.arange(len(cols[0])), np.arange(len(tws)))
    w = np.concatenate([tws[tidx], rng.choice(np.concatenate([tw["fixed"], tw["table"]]), NRANDOM)])
    cols = [np.concatenate([c[idx], r]) for c, r in zip(cols, rnd)]
    aimed = _aimed_columns(prim, q, variant, tw, edges)
    if aimed is not None:
        cols = [np.concatenate([c, a]) for c, a in zip(cols, aimed[0])]
        w = np.concatenate([w, aimed[1]])
    return [words(c) for c in cols] + list(tw_pair(w, q, kind))


# --------------------------------------------------------------------------
# the claims
# --------------------------------------------------------------------------
def _tw_value(x, kind):
    """the twiddle (an integer congruent to w) a pair's first word stands for"""
    return {"shoup": _i, "fwd": lambda v: _i(-_s(v)), "signed": _s, "fwd_signed": lambda v: -_s(v)}[kind](x)


def violations(prim, q, inputs, outputs, variant=0):
    """Boolean array: the tuples whose outputs break the primitive's claim.
    Exact integers in int64; each product's size is argued where it is formed
    (q < 2^30, words < 2^32, signed words |.| < 2^31)."""
    a = [_i(c) for c in inputs]
    o = [_i(c) for c in outputs]
    Q = np.int64(q)
    C = consts(q)
    R = np.int64(C["R"])   # 2^32 mod q: r = c 2^-32  <=>  r R = c (mod q)
    bad = np.zeros(len(a[0]), dtype=bool)

    def congruent(x, y):
        return (x - y) % Q == 0

    if prim in ("csub_q", "canon4", "bm_canon"):
        v = _s(inputs[0]) if (prim == "bm_canon" and variant) else a[0]
        return o[0] != v % Q
    if prim in ("csub_2q", "bm_half"):
        v = _s(inputs[0]) if (prim == "bm_half" and variant) else a[0]
        return o[0] != v % (2 * Q)
    if prim == "shoup_mul":      # a w < 2^32 2^30
        return ~congruent(o[0], a[0] * a[1]) | (o[0] >= 2 * Q)
    if prim == "sshoup_mul":     # |d ws| < 2^31 2^29
        d = _s(inputs[0])
        return ~congruent(o[0], d * _s(inputs[1])) | (o[0] <= 0) | (o[0] >= 2 * Q) | ((d == 0) & (o[0] != Q))
    if prim == "ct_bfly_t":
        red, xs, ys, yos = CT_FORMS[variant]
        X = _s(inputs[0]) if (red and xs) else a[0]
        Y = _s(inputs[1]) if ys else a[1]
        t = _tw_value(inputs[2], "fwd_signed" if ys else "fwd") * Y   # |w| < 2^30, |Y| < 2^32
        yo = _s(outputs[1]) if yos else o[1]
        bad |= (o[0] >= 4 * Q) | ~congruent(o[0], X + t) | ~congruent(yo, X - t)
        bad |= ((yo <= -2 * Q) | (yo >= 2 * Q)) if yos else (yo >= 4 * Q)
        return bad
    if prim == "gs_bfly":
        d = a[0] - a[1]          # |d| < 2q, |ws| < q / 2
        return (o[0] != (a[0] + a[1]) % (2 * Q)) | ~congruent(o[1], d * _s(inputs[2])) | (o[1] <= 0) | (o[1] >= 2 * Q)
    if prim in ("mont_mul", "mont_dot1", "mont_dot2"):
        L = 2 if prim == "mont_dot2" else 1
        want = sum((a[t] % Q) * (a[L + t] % Q) % Q for t in range(L))   # each factor < 2^30
        return ~congruent(o[0] * R, want) | (o[0] >= 2 * Q)            # r R < 2^32 2^30
    if prim == "redc":           # c = hi 2^32 + lo = hi R + lo (mod q); r < c / 2^32 + q
        return ~congruent(o[0] * R, (a[1] % Q) * R + a[0]) | (o[0] > a[1] + Q)
    if prim == "bm_run":
        D = 1 << MUL_LOGR
        w = _tw_value(inputs[64], "fwd") % Q
        for g in range(32 // D):
            s = bool(variant) and bool(g & 1)
            val = _s if s else _i
            A = [val(inputs[D * g + i]) % Q for i in range(D)]          # < 2^30: a product < 2^60, reduced at once
            B = [val(inputs[32 + D * g + i]) % Q for i in range(D)]
            zeta = (Q - w) % Q if g & 1 else w
            for k in range(D):
                lo = sum(A[i] * B[k - i] % Q for i in range(k + 1))
                hs = sum(A[i] * B[k + D - i] % Q for i in range(k + 1, D)) % Q
                r = o[D * g + k]
                # r < max(2q, WH): r 2^32 < WB_NUM, i.e. r < ceil(WB_NUM / 2^32) for an integer r
                bad |= ~congruent(r * R, lo + zeta * hs) | (r >= np.int64(C["WB"]))
        return bad
    if prim == "inv_wide0":
        ws = _s(inputs[32])
        for j in range(16):
            x, y = a[j], a[j + 16]   # < 3q: |x - y| < 2^31 (BaseMul's static_assert), |ws| < q / 2
            bad |= (o[j] != (x + y) % (2 * Q)) | ~congruent(o[j + 16], (x - y) * ws) | (o[j + 16] <= 0) | (o[j + 16] >= 2 * Q)
        return bad
    if prim == "inv_last":
        s0, s1, canon = inv_last_consts(q, variant)
        top = Q if canon else 2 * Q
        for j in range(16):
            x, y = a[j], a[j + 16]   # x + y < 4q < 2^32, S0, S1 < q
            bad |= ~congruent(o[j], (x + y) * np.int64(s0)) | ~congruent(o[j + 16], (x - y) * np.int64(s1))
            bad |= (o[j] >= top) | (o[j + 16] >= top)
        for j in range(32):
            bad |= o[32 + j] != o[j]   # the emit callback saw the same words
        return bad
    if prim == "round_coeff":
        import round_model
        bad = np.zeros(len(a[0]), dtype=bool)
        for d in range(1, 31):
            m = a[1] == d
            c, lo, hi = round_model.split(a[0][m], q, d)
            bad[m] = (_s(outputs[0])[m] != hi) | (o[1][m] != np.abs(c)) | (o[2][m] != np.abs(lo))
        return bad | (a[1] < 1) | (a[1] > 30)
    raise KeyError(prim)


def check(prim, q, inputs, outputs, variant=0):
    """Assert the claim of `prim` over all tuples; reports the first failing one."""
    bad = violations(prim, q, inputs, outputs, variant)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(
            f"{prim} (variant {variant}, q = {q}): {int(bad.sum())} of {len(bad)} tuples break the claim; first at {i}: "
            f"in = {[hex(int(c[i])) for c in inputs]}, out = {[hex(int(c[i])) for c in outputs]}")
