"""gen_a_model, the Python statement of poly_gen_a's definition: the literal
loop against the flat draw stream, the draws a call gives, the refill bound,
the range of the output, and the refill counts of the fixed seeds that the GPU
tests and the timing tool rely on."""
import functools

import pytest

import gen_a_model as M
import keccak_model as K

# one squeeze per (hash, seed, length, customisation) for the whole module
K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)

Q1, Q3 = 343576577, 856145921   # p-I, p-III (tests/test_gen_a_abi.py reads them from the library)


def refills(k, n, q, nblocks, count):
    out = []
    for seed in K.seeds(count):
        st = {}
        a = M.gen_a(seed, k, n, q, nblocks, st)
        assert len(a) == k and all(len(p) == n for p in a)
        assert all(0 <= v < q for p in a for v in p)
        out.append(st["refills"])
    return out


@pytest.mark.parametrize("q,n,k,nblocks", ((Q1, 1024, 1, 1), (Q1, 1024, 2, 35), (Q3, 2048, 1, 70), (Q1, 1024, 4, 108)))
def test_literal_loop_is_the_flat_stream(q, n, k, nblocks):
    for seed in K.seeds(2):
        assert M.gen_a(seed, k, n, q, nblocks) == M.gen_a_flat(seed, k, n, q, nblocks)


def test_draws_per_call():
    assert M.nbytes(Q1) == 4 and M.nbytes(Q3) == 4 and M.qbits(Q1) == 29 and M.qbits(Q3) == 30
    assert M.draws_per_call(1) == 40      # words 40 and 41 of a refill block are unused
    assert M.draws_per_call(35) == 1468   # odd: 1470 words, the last two unused
    assert M.draws_per_call(108) == 4536
    assert M.draws_per_call(180) == 7560
    assert M.draws_per_call(2) == 84 and M.draws_per_call(256) == 42 * 256


def test_refills_max():
    assert M.refills_max(1, 1024) == 104
    assert M.refills_max(4, 1024) == 412
    assert M.refills_max(5, 2048) == 1024
    assert M.refills_max(8, 1024) == 820
    assert M.refills_max(8, 8192) == 6556
    assert all(M.refills_max(k, n) <= 65535 for k in range(1, 9) for n in (1024, 2048, 4096, 8192))


def test_first_call_is_customisation_0_and_refills_count_up():
    """k n = 1024 values at nblocks = 1: the first 40 words of cstm 0, then of cstm 1, 2, ..."""
    seed = K.seeds(1)[0]
    st = {}
    a = M.gen_a(seed, 1, 1024, Q1, 1, st)[0]
    mask, drawn, call = (1 << 29) - 1, [], 0
    while len(drawn) < 1024:
        buf = K.cshake_simple("shake128", seed, 168, call)
        drawn += [v for v in (int.from_bytes(buf[4 * j:4 * j + 4], "little") & mask for j in range(40)) if v < Q1]
        call += 1
    assert a == drawn[:1024] and st["refills"] == call - 1


def test_refills_of_qteslas_shapes():
    assert refills(4, 1024, Q1, 108, 8) == [48, 48, 48, 47, 47, 48, 47, 46]
    assert refills(5, 2048, Q3, 180, 4) == [134, 133, 132, 134]


def test_refills_of_the_gpu_tests_shapes():
    """what tests/test_gpu_gen_a.py says about its cases"""
    r = refills(1, 1024, Q1, 1, 67)
    assert min(r) == 37 and max(r) == 41
    r = refills(2, 1024, Q1, 35, 5)
    assert min(r) >= 41 and max(r) <= 45
    assert refills(1, 2048, Q3, 70, 16) == [0] * 16
    assert set(refills(1, 2048, Q3, 61, 16)) == {0, 1, 2}
    assert sorted(refills(1, 8192, Q3, 2, 2)) == [255, 256]   # cstm crosses 255 into its high byte
    assert 321 in refills(8, 1024, Q1, 1, 2)
