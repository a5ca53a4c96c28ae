"""CPU model of the device arithmetic of csrc/ntt_device.hpp, instruction by
instruction with 32-bit wrap-around (Python ints masked to 32 / 64 bits):
the lazy CT butterfly, the typed "lazy-bias" CT butterfly of poly_mul
(ct_bfly_t: S-form values in (-2q, 2q), signed Shoup quotients with centred
twiddles), the signed Shoup product and BaseMul's zeta-split residue
products.  Checks congruence mod q and the output ranges the kernels rely on,
over edge values and random samples, for every prime.  The GPU parity tests
check the kernels themselves; this pins the bounds the static_asserts and
comments state.

The model lives in tests/arith_model.py, which also restates every other
inlined primitive (numpy, word-exact), builds the operand grid and states each
primitive's claim; tests/test_gpu_device_arith.py runs the device functions
over that grid and compares them with the claims and with the model word for
word.  The second half of this module keeps the CPU side of that honest: the
model satisfies every claim over the whole grid, the library's constant
builders equal their definitions, and the grid rejects seven deliberate errors."""
import random

import numpy as np
import pytest

import arith_model as AM
from arith_model import M32, M64, PRIMES, centred, ct_bfly_t, fwd_signed_table, madlo32, redc, s32, samples, shoup, sq_quot, umulhi, value


@pytest.mark.parametrize("name", list(PRIMES))
@pytest.mark.parametrize("xs,ys,yos", [(False, False, False), (False, False, True), (True, True, True),
                                       (True, True, False), (True, False, True), (True, False, False)])
def test_typed_ct_butterfly(name, xs, ys, yos):
    q = PRIMES[name]
    rng = random.Random(hash((name, xs, ys, yos)) & 0xFFFF)
    ws = [0, 1, q - 1, q // 2, q // 2 + 1] + [rng.randrange(q) for _ in range(40)]
    for w in ws:
        for x, y in zip(samples(q, xs, rng), samples(q, ys, rng)):
            xo, yo = ct_bfly_t(x, y, w, q, True, xs, ys, yos)
            X, Y = value(x, xs), value(y, ys)
            assert 0 <= xo < 4 * q
            assert (xo - (X + w * Y)) % q == 0
            Yv = value(yo, yos)
            assert ((-2 * q < Yv < 2 * q) if yos else (0 <= Yv < 4 * q))
            assert (Yv - (X - w * Y)) % q == 0


@pytest.mark.parametrize("name", list(PRIMES))
def test_canonical_stage0_and_s_canon(name):
    """stage 0 of fwd_pass1_lz: canonical inputs, no reduction, S output; and
    BaseMul::canon: (-2q, 2q) -> [0, q) by
    min(x, x + 2q) then one conditional subtraction of q"""
    q = PRIMES[name]
    rng = random.Random(7)
    for _ in range(2000):
        x, y, w = rng.randrange(q), rng.randrange(q), rng.randrange(q)
        xo, yo = ct_bfly_t(x, y, w, q, False, False, False, True)
        assert 0 <= xo < 4 * q and -2 * q < s32(yo) < 2 * q
        a = min(yo, (yo + 2 * q) & M32)
        c = min(a, (a - q) & M32)
        assert c == (x - w * y) % q


@pytest.mark.parametrize("name", list(PRIMES))
def test_signed_shoup_range(name):
    """sshoup_mul: |d| < 2^31, centred twiddle -> d ws - e q in (0, 2q)"""
    q = PRIMES[name]
    rng = random.Random(3)
    for _ in range(3000):
        d = rng.randrange(-(1 << 31) + 1, 1 << 31)
        w = rng.randrange(q)
        ws, wps = centred(w, q)
        e = sq_quot(d & M32, wps & M32)
        t = ((d & M32) * (ws & M32) - e * q) & M32
        assert 0 < t < 2 * q
        assert (t - d * w) % q == 0


def test_fwd_signed_table_is_the_fwd_table_centred(ntt):
    """the compile-time signed pass-1 twiddles name the same psi^brv(k) as the
    library's tables (ntt_get_tables Phi[i] = psi^i)"""
    for name in ("ref", "p-I", "p-III"):
        info = ntt.param_info(name)
        q, n = info["q"], info["n"]
        phi = ntt.tables(name)["Phi"]
        logn = n.bit_length() - 1
        tab = fwd_signed_table(q, info["psi"], logn)
        for k in range(2, 32):
            w = int(phi[int(format(k, f"0{logn}b")[::-1], 2)])
            ws, wps = centred(w, q)
            assert tab[k] == ((-ws) & M32, wps & M32)


@pytest.mark.parametrize("name", list(PRIMES))
def test_zeta_split_residue_product(name):
    """BaseMul::run_zsplit: c_k = L_k + zR * REDC(H_k) fits 64 bits, its REDC
    lands in [0, 2q) after one conditional subtraction, and equals the
    product mod x^8 - zeta times 2^-32"""
    q = PRIMES[name]
    qinv = pow(q, -1, 1 << 32)
    qneg = (-qinv) & M32
    R = (1 << 32) % q
    rinv = pow(R, -1, q)
    rng = random.Random(11)
    cases = [([q - 1] * 8, [q - 1] * 8, q - 1)] + \
        [([rng.randrange(q) for _ in range(8)], [rng.randrange(q) for _ in range(8)], rng.randrange(q))
         for _ in range(300)]
    for a, b, zeta in cases:
        # device: one negated Shoup product of R by the pair's twiddle w, then
        # the two-candidate min for the +w and the -w residue -> [0, q]
        w = zeta
        tn = madlo32(umulhi(R, shoup(w, q)), q, (R * ((-w) & M32)) & M32)
        for sign in (1, -1):
            if sign == 1:
                zr = min((-tn) & M32, ((-q) - tn) & M32)
            else:
                zr = min((tn + q) & M32, (tn + 2 * q) & M32)
            z = w if sign == 1 else q - w   # the residue's zeta
            assert 0 <= zr <= q and (zr - z * R) % q == 0
            for k in range(8):
                L = sum(a[i] * b[k - i] for i in range(k + 1))
                c = L
                if k < 7:
                    H = sum(a[i] * b[k + 8 - i] for i in range(k + 1, 8))
                    assert H + M32 * q <= M64
                    c += zr * redc(H, q, qneg)
                assert c + M32 * q <= M64, "REDC input fits 64 bits"
                r = redc(c, q, qneg)
                assert r < 4 * q
                r = min(r, (r - 2 * q) & M32)
                assert 0 <= r < 2 * q
                want = (L + z * sum(a[i] * b[k + 8 - i] for i in range(k + 1, 8))) * rinv % q
                assert r % q == want


@pytest.mark.parametrize("name", list(PRIMES))
def test_half_canonical_residue_product_and_wide_first_stage(name):
    """BaseMul::AH, the half-canonical a (p-III, where the z-split output
    needs its csub anyway):
    a in [0, 2q), b canonical -> c_k < 16 q^2 fits 64 bits with the REDC's
    m q; the REDC output after one csub lies below 2.19 q (p-III), and the
    inverse's first GS stage (inv_pass2 WIDE0) maps such x, y to
    (x + y) mod 2q by a three-candidate min, with |x - y| < 2^31"""
    q = PRIMES[name]
    qneg = (-pow(q, -1, 1 << 32)) & M32
    R = (1 << 32) % q
    rinv = pow(R, -1, q)
    rng = random.Random(5)
    cases = [([2 * q - 1] * 8, [q - 1] * 8, q - 1)] + \
        [([rng.randrange(2 * q) for _ in range(8)], [rng.randrange(q) for _ in range(8)], rng.randrange(q))
         for _ in range(300)]
    outs = []
    for a, b, z in cases:
        zr = z * R % q
        for k in range(8):
            L = sum(a[i] * b[k - i] for i in range(k + 1))
            H = sum(a[i] * b[k + 8 - i] for i in range(k + 1, 8))
            c = L + (zr * redc(H, q, qneg) if k < 7 else 0)
            assert c < 16 * q * q and c + M32 * q <= M64
            r = redc(c, q, qneg)
            assert r < 16 * q * q / 2 ** 32 + q
            r = min(r, (r - 2 * q) & M32)
            assert (r - (L + z * H) * rinv) % q == 0
            outs.append(r)
    wh = max(16 * q * q / 2 ** 32 + q - 2 * q, 2 * q)
    assert max(outs) < wh and wh < 3 * q and wh < 2 ** 31
    for _ in range(2000):
        x, y = rng.choice(outs), rng.choice(outs)
        sm = (x + y) & M32
        xo = min(sm, (sm - 2 * q) & M32, (sm - 4 * q) & M32)
        assert xo == (x + y) % (2 * q)
        assert abs(x - y) < 2 ** 31


# --------------------------------------------------------------------------
# arith_model: the vector model, the operand grid and the claims that
# tests/test_gpu_device_arith.py runs against the device functions themselves
# --------------------------------------------------------------------------
CASE_IDS = [f"{p}-v{v}" for p, v in AM.CASES]


@pytest.fixture(scope="module")
def twiddles(ntt):
    """the grid's twiddle sets, from the library's own Phi / invPhi tables,
    which are what arith_model.model_tables restates"""
    out = {}
    for name, q in PRIMES.items():
        t = ntt.tables(name)
        phi, inv = AM.model_tables(q)
        assert np.array_equal(t["Phi"], phi) and np.array_equal(t["invPhi"], inv)
        out[name] = AM.twiddle_set(q, t["Phi"], t["invPhi"])
    return out


@pytest.mark.parametrize("name", list(PRIMES))
def test_vector_model_is_the_scalar_model(name):
    """the numpy model (what the GPU outputs are compared with word for word)
    and the scalar helpers above agree on every typed butterfly form"""
    q = PRIMES[name]
    rng = random.Random(17)
    for form in AM.CT_FORMS:
        red, xs, ys, yos = form
        xw = samples(q, xs, rng, 60) if red else [rng.randrange(2 * q) for _ in range(60)]
        yw = samples(q, ys, rng, len(xw) - (9 if ys else 7))
        ws = [rng.randrange(q) for _ in xw]
        wn, wp = AM.tw_pair(ws, q, "fwd_signed" if ys else "fwd")
        got = AM.v_ct_bfly_t(AM.words(xw), AM.words(yw), wn, wp, q, *form)
        want = [ct_bfly_t(x, y, w, q, *form) for x, y, w in zip(xw, yw, ws)]
        assert [(int(a), int(b)) for a, b in zip(*got)] == want


@pytest.mark.parametrize("name", list(PRIMES))
@pytest.mark.parametrize("prim,variant", AM.CASES, ids=CASE_IDS)
def test_model_stays_inside_every_claim(twiddles, name, prim, variant):
    """check() accepts the model's outputs over the whole grid: the reference
    of the GPU test satisfies every claim that test makes"""
    q = PRIMES[name]
    inputs = AM.grid(prim, q, variant, twiddles[name])
    assert len(inputs) == AM.PRIMS[prim][1] and len({len(c) for c in inputs}) == 1
    outputs = AM.model(prim, q, inputs, variant)
    assert len(outputs) == AM.PRIMS[prim][2]
    AM.check(prim, q, inputs, outputs, variant)


@pytest.mark.parametrize("name", list(PRIMES))
@pytest.mark.parametrize("mutant", list(AM.MUTANTS))
def test_grid_rejects_mutant(twiddles, name, mutant):
    """the grid has teeth: each deliberate error of the model breaks a claim
    on at least one tuple of the same grid, for every prime"""
    q = PRIMES[name]
    for prim, variant in AM.MUTANTS[mutant]:
        inputs = AM.grid(prim, q, variant, twiddles[name])
        outputs = AM.model(prim, q, inputs, variant, mutant=mutant)
        nbad = int(AM.violations(prim, q, inputs, outputs, variant).sum())
        assert nbad > 0, f"{mutant} passes {prim} v{variant}"
        with pytest.raises(AssertionError, match="first at"):
            AM.check(prim, q, inputs, outputs, variant)


@pytest.fixture(scope="module")
def probe_host(ntt):
    """the probe library's host entry points; they need no device"""
    import arith_probe
    try:
        return arith_probe, arith_probe.load(ntt)
    except OSError as e:
        pytest.skip(f"{arith_probe.path(ntt)} does not load without a device: {e}")


@pytest.mark.parametrize("name", list(PRIMES))
def test_constant_builders(probe_host, name):
    """cshoup, csigned_tw, cqinv_neg and the per-set constants of pset.hpp, as
    the library's own constexpr functions compute them, equal the definitions"""
    AP, L = probe_host
    q, n, psi = AM.SETS[name]
    C = AP.consts(L, name)
    assert (C["Q"], C["N"], C["PSI"], C["MUL_LOGR"]) == (q, n, psi, AM.MUL_LOGR)
    assert C["QNEG"] == (-pow(q, -1, 1 << 32)) & M32 == L.arith_probe_cqinv_neg(q)
    assert C["R"] == (1 << 32) % q
    assert C["NINV"] == pow(n, -1, q) and C["C1"] == pow(n, -1, q) * pow(psi, -(n // 2), q) % q
    assert C["NINV_R"] == C["NINV"] * C["R"] % q and C["C1_R"] == C["C1"] * C["R"] % q
    assert C["NINV_R_SHORT"] == pow(n >> AM.MUL_LOGR, -1, q) * C["R"] % q   # (n / 2^LOGR)^-1 2^32
    assert C["C1_R_SHORT"] == pow(n >> AM.MUL_LOGR, -1, q) * pow(psi, -(n // 2), q) * C["R"] % q
    mine = AM.consts(q)
    for k in AP.CONST_NAMES:
        if k != "MUL_LOGR":
            assert C[k] == int(mine[k]), k
    tw = AM.twiddle_set(q, *AM.model_tables(q))
    ws = [0] + [int(w) for w in tw["fixed"]] + [int(w) for w in tw["table"][:: max(1, len(tw["table"]) // 512)]]
    ws += [q // 2 - 1, q // 2, q // 2 + 1, q // 2 + 2]
    for w in ws:
        assert L.arith_probe_cshoup(w, q) == (w << 32) // q
        cs, cp = centred(w, q)
        assert -q // 2 < cs <= q // 2 and (cs - w) % q == 0
        assert AP.csigned_tw(L, w, q) == (cs & M32, cp & M32)
    a, b = AM.tw_pair(ws, q, "signed")
    assert [(int(x), int(y)) for x, y in zip(a, b)] == [AP.csigned_tw(L, w, q) for w in ws]


@pytest.mark.parametrize("name", list(PRIMES))
def test_aimed_tuples_reach_the_ends(twiddles, name):
    """the grid's aimed operands do what their construction says: the unsigned
    lazy product sits one q above its residue and comes within q^2 / 2^32 of
    2q; the signed one comes that near to both ends of (0, 2q)"""
    q = PRIMES[name]
    ws = AM.aim_twiddles(q, twiddles[name])
    slack = (q * q >> 32) + 4
    a, w = (np.array(c, dtype=np.int64) for c in zip(*AM.aimed_unsigned(q, ws, 1 << 32)))
    out = AM.model("shoup_mul", q, [AM.words(a), *AM.tw_pair(w, q, "shoup")])[0]
    assert [int(o) for o in out] == [int(x) * int(y) % q + q for x, y in zip(a, w)]
    assert 2 * q - slack <= int(out.max()) < 2 * q
    d, w = (np.array(c, dtype=np.int64) for c in zip(*AM.aimed_signed(q, ws, 1 << 31)))
    assert np.abs(d).max() < 1 << 31
    out = AM.model("sshoup_mul", q, [AM.words(d), *AM.tw_pair(w, q, "signed")])[0]
    assert 0 < int(out.min()) <= slack and 2 * q - slack <= int(out.max()) < 2 * q
    d, w = (np.array(c, dtype=np.int64) for c in zip(*AM.aimed_signed(q, ws, 2 * q)))
    assert np.abs(d).max() < 2 * q   # what gs_bfly and an S-form y can hold
