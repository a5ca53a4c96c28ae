"""gauss_model without a GPU: the table's shape, hsum against sort-and-sum,
the sampler's first two moments over the fixed seeds, and the recorded digests
that pin the model against drift (they are the model's own output at the time
they were recorded, not an independent reference: none exists here)."""
import hashlib
import json
import math
import os
import random

import pytest

import gauss_model as G
import keccak_model as K

Q1, Q3 = 343576577, 856145921
SHAPES = {"p-I": (1024, Q1, 77, 2, "shake128"), "p-III": (2048, Q3, 110, 4, "shake256")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gauss_kat.json")


@pytest.mark.parametrize("rows,cols", ((77, 2), (110, 4), (30, 1), (90, 3)))
def test_table_shape(rows, cols):
    T = G.cdt_integers("8.5", rows, cols)
    assert len(T) == rows and all(a < b for a, b in zip(T, T[1:]))
    assert 0 < T[0] and T[-1] < 1 << (31 * cols)
    table = G.cdt_table(8.5, rows, cols)
    assert all(len(row) == cols and all(0 <= w < 1 << 31 for w in row) for row in table)
    assert G.row_integers(table, cols) == list(T)
    # P(m = 0) = D(0) = 1 / S; S is within 10^-9 of sigma sqrt(2 pi) at sigma = 8.5
    assert abs(T[0] / (1 << (31 * cols)) - 1 / (8.5 * math.sqrt(2 * math.pi))) < 1e-9


def test_table_ignores_bit_31():
    table = G.cdt_table(8.5, 5, 2)
    marked = [[w | 0x80000000 for w in row] for row in table]
    assert G.row_integers(marked, 2) == G.row_integers(table, 2)


def test_hsum_is_sort_and_sum():
    rng = random.Random(0x6A55)
    for q in (Q1, Q3):
        for trial in range(40):
            n = rng.choice((8, 64, 1024))
            top = rng.choice((3, 40, 2 * q - 1))   # small ranges: many ties
            w = [rng.randint(0, top) for _ in range(n)]
            a = sorted(G.centred_abs(w, q), reverse=True)
            for h in (1, 2, n // 2, n - 1, n):
                assert G.hsum(w, q, h) == sum(a[:h]), (q, n, top, h)
    assert G.centred_abs([0, 1, (Q1 - 1) // 2, (Q1 + 1) // 2, Q1 - 1, Q1, Q1 + 1, 2 * Q1 - 1], Q1) == \
        [0, 1, (Q1 - 1) // 2, (Q1 - 1) // 2, 1, 0, 1, 1]


def test_sign_and_zero():
    """-0 is 0: with a table nothing reaches, every output is 0 whatever the sign bit"""
    n, q = 1024, Q1
    seed = K.seeds(1)[0]
    words = G.sample_words(seed, n, 2, "shake128", 0)
    assert any(w[0] >> 31 for w in words) and not all(w[0] >> 31 for w in words)
    assert G.sample_gauss(seed, n, q, [[G.LIMB, G.LIMB]], 2, "shake128", 0) == [0] * n
    out = G.sample_gauss(seed, n, q, [[0, 0]] * 3, 2, "shake128", 0)
    assert set(out) == {3, q - 3} and [v == q - 3 for v in out] == [bool(w[0] >> 31) for w in words]


def test_chunks_and_nonces_separate():
    """a chunk's stream is cshake(seed, ((nonce << 8) + chunk) & 0xFFFF): chunk 1 at nonce 0 is not chunk 0 at nonce 1"""
    seed = K.seeds(1)[0]
    a = G.sample_words(seed, 1024, 2, "shake128", 0)
    b = G.sample_words(seed, 1024, 2, "shake128", 1)
    assert a[:512] != a[512:] and a[:512] != b[:512] and a[512:] != b[:512]
    buf = K.cshake_simple("shake128", seed, 4096, 0x0101)
    assert b[512] == [int.from_bytes(buf[0:4], "little"), int.from_bytes(buf[4:8], "little")]


def test_moments_over_the_fixed_seeds():
    """16 seeds at p-I's shape, N = 16 384 samples of sigma = 8.5: the mean of N
    independent samples has deviation sigma / sqrt(N), the sample variance of a
    (near) Gaussian sigma^2 sqrt(2 / N); both margins are five of those."""
    n, q, rows, cols, algo = SHAPES["p-I"]
    table = G.cdt_table(8.5, rows, cols)
    xs = []
    for seed in K.seeds(16):
        xs += [v - q if v > q // 2 else v for v in G.sample_gauss(seed, n, q, table, cols, algo, 0)]
    N, sigma = len(xs), 8.5
    assert N == 16 * n and max(abs(x) for x in xs) <= rows
    mean = sum(xs) / N
    var = sum((x - mean) ** 2 for x in xs) / (N - 1)
    assert abs(mean) <= 5 * sigma / math.sqrt(N), mean
    assert abs(var - sigma * sigma) <= 5 * sigma * sigma * math.sqrt(2 / N), var


def kat_digest(ps, idx, nonce):
    n, q, rows, cols, algo = SHAPES[ps]
    out = G.sample_gauss(K.seeds(idx + 1)[idx], n, q, G.cdt_table(8.5, rows, cols), cols, algo, nonce)
    return hashlib.sha256(b"".join(v.to_bytes(4, "little") for v in out)).hexdigest()


def test_recorded_digests():
    with open(GOLDEN) as f:
        kat = json.load(f)
    assert len(kat["cases"]) == 2
    for case in kat["cases"]:
        assert kat_digest(case["param_set"], case["seed_index"], case["nonce"]) == case["sha256"], case
