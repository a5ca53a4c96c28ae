"""sample_model.sample_y, the Python statement of poly_sample_y's definition:
its first call against NIST cSHAKE with general N and S, the range of the
output, the nonce's domain separation, the smallest `bits`, and the
rejection / refill statistics of the fixed seeds that the GPU tests rely on."""
import functools

import pytest

import keccak_model as K
import sample_model as M

# one squeeze per (hash, seed, length, customisation) for the whole module
K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)

Q1, Q3 = 343576577, 856145921   # p-I, p-III (tests/test_sample_y_abi.py reads them from the library)


@pytest.mark.parametrize("algo,n", (("shake128", 1024), ("shake256", 1024), ("shake256", 2048)))
@pytest.mark.parametrize("nonce", (0, 1, 255))
def test_first_call_is_nist_cshake(algo, n, nonce):
    seed = K.seeds(1)[0]
    cstm = nonce << 8
    assert K.cshake_simple(algo, seed, 3 * n, cstm) == K.cshake(algo, seed, 3 * n, N=b"", S=cstm.to_bytes(2, "little"))
    # bits = 24: no masking, and a rejection has probability 2^-24 a draw: y is the stream itself
    st = {}
    y = M.sample_y(seed, n, Q3, 24, algo, nonce, st)
    buf = K.cshake_simple(algo, seed, 3 * n, cstm)
    B = (1 << 23) - 1
    assert st == {"rejected": 0, "refills": 0}
    assert y == [(int.from_bytes(buf[3 * j:3 * j + 3], "little") - B) % Q3 for j in range(n)]


@pytest.mark.parametrize("bits", (2, 3, 14, 20, 22, 24))
def test_range(bits):
    B = (1 << (bits - 1)) - 1
    for q, n, algo in ((Q1, 1024, "shake128"), (Q3, 2048, "shake256")):
        y = M.sample_y(K.seeds(2)[1], n, q, bits, algo, 0)
        assert len(y) == n and all(0 <= v < q for v in y)
        centred = [v - q if v > q // 2 else v for v in y]
        assert -B <= min(centred) and max(centred) <= B
        if bits <= 3:   # 3 or 7 values over >= 1024 draws: both ends are reached
            assert min(centred) == -B and max(centred) == B


def test_nonces_differ():
    seed = K.seeds(1)[0]
    ys = [M.sample_y(seed, 1024, Q1, 20, "shake128", nonce) for nonce in (0, 1, 255)]
    assert ys[0] != ys[1] and ys[1] != ys[2] and ys[0] != ys[2]
    assert M.sample_y(seed, 1024, Q1, 20, "shake256", 0) != ys[0]


def test_bits_2_is_ternary():
    st = {}
    y = M.sample_y(K.seeds(1)[0], 1024, Q1, 2, "shake128", 0, st)
    assert set(y) == {Q1 - 1, 0, 1}
    assert st["rejected"] > 0 and st["refills"] > 0


def test_refill_is_one_block_with_the_next_customisation():
    """a rejection in the first call costs one refill: the last coefficient is the first accepted
    draw of cshake_simple(seed, rate, cstm + 1)"""
    n, bits, algo, nonce = 1024, 14, "shake128", 3
    mask, B = (1 << bits) - 1, (1 << (bits - 1)) - 1
    for idx in (19, 29, 44, 69):
        seed = K.seeds(70)[idx]
        st = {}
        y = M.sample_y(seed, n, Q1, bits, algo, 0, st)
        assert st == {"rejected": 1, "refills": 1}
        buf = K.cshake_simple(algo, seed, 168, 1)
        assert y[-1] == ((int.from_bytes(buf[:3], "little") & mask) - B) % Q1
    seed = K.seeds(1)[0]
    st = {}
    y = M.sample_y(seed, n, Q1, 2, algo, nonce, st)
    drawn, r = [], 0
    buf = K.cshake_simple(algo, seed, 3 * n, nonce << 8)
    while len(drawn) < n:
        drawn += [v - 1 for v in ((int.from_bytes(buf[p:p + 3], "little") & 3) for p in range(0, len(buf) - 2, 3)) if v != 3]
        r += 1
        buf = K.cshake_simple(algo, seed, 168, (nonce << 8) + r)
    assert y == [v % Q1 for v in drawn[:n]] and st["refills"] == r - 1


def stats(n, q, bits, algo, count):
    out = []
    for seed in K.seeds(count):
        st = {}
        M.sample_y(seed, n, q, bits, algo, 0, st)
        out.append((st["rejected"], st["refills"]))
    return out


def test_statistics_bits_2():
    """every seed refills, several times: the GPU test's all-blocks-reject case"""
    for n, q, algo, count, rej, refills in ((1024, Q1, "shake128", 4, (287, 388), (6, 7)),
                                            (2048, Q3, "shake256", 3, (641, 700), (15, 16))):
        for rj, rf in stats(n, q, 2, algo, count):
            assert rej[0] <= rj <= rej[1] and refills[0] <= rf <= refills[1], (algo, rj, rf)


def test_statistics_bits_14():
    """batch 70 of the GPU test: one rejection and one refill in a few seeds of both waves, none elsewhere"""
    for n, q, algo, hit in ((1024, Q1, "shake128", (19, 29, 44, 69)), (2048, Q3, "shake256", (8, 14, 27, 35, 54, 64, 65))):
        got = stats(n, q, 14, algo, 70)
        assert [i for i, s in enumerate(got) if s != (0, 0)] == list(hit)
        assert all(got[i] == (1, 1) for i in hit)
        assert any(i < 64 for i in hit) and any(i >= 64 for i in hit)
