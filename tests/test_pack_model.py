"""The numpy model of poly_pack / poly_unpack (pack_model.py) against literal
vectors worked out by hand from the definition in include/qtesla_ntt.h, and
the definition's two round-trip identities for the three primes and every
legal field width."""
import numpy as np
import pytest

import pack_model as M

Q_P1 = 343576577
PRIMES = (8404993, 343576577, 856145921)


def test_signed_20_bit_vector():
    """b = 20: pt[0] = z0 | z1 << 20, pt[1] = z1 >> 12 | z2 << 8 | z3 << 28, ..."""
    z = np.array([1, -1, 524287, -524288, 2, -2, 0x12345, -0x12345], dtype=np.int64)
    w = (z % Q_P1).astype(np.uint32)
    want = bytes.fromhex("0100f0ffffffff0700800200e0ffff4523b1cbed")
    got = M.poly_pack(w, Q_P1, 20, True)
    assert got.tobytes() == want
    assert got.view("<u4").tolist() == [0xfff00001, 0x07ffffff, 0x00028000, 0x45ffffe0, 0xedcbb123]
    # words in [q, 2q) pack alike
    assert M.poly_pack(w + np.uint32(Q_P1), Q_P1, 20, True).tobytes() == want
    back, mx = M.poly_unpack(np.frombuffer(want, dtype=np.uint8), 8, Q_P1, 20, True)
    assert np.array_equal(back, w) and int(mx) == 524288


def test_unsigned_29_bit_vector():
    q = Q_P1
    t = np.array([0, 1, q - 1, q, (1 << 29) - 1, 2, 3, 4], dtype=np.int64)
    want = bytes.fromhex("000000200000000040ead100483dfaffffff050000c000000020000000")
    # q and 2^29 - 1 are not packable values (pack reduces mod q first): the bytes come from the raw fields
    assert M.pack_fields(t.astype(np.uint32), 29).tobytes() == want
    back, mx = M.poly_unpack(np.frombuffer(want, dtype=np.uint8), 8, q, 29, False)
    assert back.tolist() == [0, 1, q - 1, 0, 193294334, 2, 3, 4]
    assert int(mx) == 536870911
    # packing the unpacked (canonical) values gives the fields of the values mod q
    again = M.unpack_fields(M.poly_pack(back, q, 29, False), 8, 29)
    assert again.tolist() == [0, 1, q - 1, 0, 193294334, 2, 3, 4]


def test_bit_stream_order():
    """field i at stream bits [i b, (i + 1) b), bit j = bit j mod 8 of byte j / 8"""
    for b in (8, 9, 23, 30):
        for i in (0, 1, 7):
            f = np.zeros(8, dtype=np.uint32)
            f[i] = 1 | (1 << (b - 1))
            by = M.pack_fields(f, b)
            bits = {j for j in range(8 * b) if (by[j // 8] >> (j % 8)) & 1}
            assert bits == {i * b, i * b + b - 1}, (b, i)


@pytest.mark.parametrize("q", PRIMES)
def test_bytes_round_trip_signed(q):
    """poly_pack(poly_unpack(bytes)) == bytes for every byte string, signed"""
    rng = np.random.default_rng(q)
    n = 64
    for b in M.bits_range(q, True):
        assert 1 << (b - 1) <= (q - 1) // 2
        by = rng.integers(0, 256, (3, n * b // 8), dtype=np.uint8)
        by[0, :] = 0xFF
        by[1, :] = np.tile(np.array([0x00, 0x80], dtype=np.uint8), n * b // 16)
        w, mx = M.poly_unpack(by, n, q, b, True)
        assert w.max() < q and mx.max() <= 1 << (b - 1)
        assert np.array_equal(M.poly_pack(w, q, b, True), by), b
        assert np.array_equal(M.poly_pack(w + np.uint32(q), q, b, True), by), b


@pytest.mark.parametrize("q", PRIMES)
@pytest.mark.parametrize("signed", (True, False))
def test_coefficient_round_trip(q, signed):
    """poly_unpack(poly_pack(w)) == w mod q whenever w's values fit b bits"""
    rng = np.random.default_rng(q + signed)
    n = 64
    for b in M.bits_range(q, signed):
        if signed:
            c = rng.integers(-(1 << (b - 1)), 1 << (b - 1), (2, n), dtype=np.int64)
            c[0, :4] = (-(1 << (b - 1)), (1 << (b - 1)) - 1, -1, 0)
        else:
            c = rng.integers(0, min(q, 1 << b), (2, n), dtype=np.int64)
            c[0, :3] = (0, min(q, 1 << b) - 1, 1)
        w = (c % q).astype(np.uint32)
        w[1] += np.uint32(q)   # words in [q, 2q)
        back, mx = M.poly_unpack(M.poly_pack(w, q, b, signed), n, q, b, signed)
        assert np.array_equal(back, w % np.uint32(q)), b
        assert np.array_equal(mx, np.abs(c).max(axis=-1)), b


@pytest.mark.parametrize("q", PRIMES)
def test_unsigned_bytes_round_trip_iff_below_q(q):
    b = M.qbits(q)
    n = 64
    rng = np.random.default_rng(q)
    f = rng.integers(0, q, (1, n), dtype=np.int64).astype(np.uint32)
    by = M.pack_fields(f, b)
    w, mx = M.poly_unpack(by, n, q, b, False)
    assert np.array_equal(M.poly_pack(w, q, b, False), by) and int(mx[0]) < q
    f[0, 5] = q                     # one field >= q: canonical output, bytes differ, the maximum tells
    by = M.pack_fields(f, b)
    w, mx = M.poly_unpack(by, n, q, b, False)
    assert w[0, 5] == 0 and int(mx[0]) == q
    assert not np.array_equal(M.poly_pack(w, q, b, False), by)


def test_truncation():
    """a value outside the field's range keeps its low b bits"""
    q, b = Q_P1, 20
    c = np.array([1 << 19, -(1 << 19) - 1, (1 << 20) + 5, -(1 << 21)], dtype=np.int64)
    f = M.fields((c % q).astype(np.uint32), q, b, True)
    assert f.tolist() == [1 << 19, (1 << 19) - 1, 5, 0]


def test_rows():
    q, b, n, k = PRIMES[2], 30, 64, 5
    rng = np.random.default_rng(1)
    w = rng.integers(0, q, (3, k, n), dtype=np.uint32)
    packed = k * n * b // 8
    gap = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    rows = M.pack_rows(w, q, b, False, packed + 32, gap)
    assert rows.shape == (3, packed + 32) and np.array_equal(rows[:, packed:], gap)
    assert np.array_equal(rows[1, n * b // 8:2 * n * b // 8], M.poly_pack(w[1, 1], q, b, False))
    back, mx = M.unpack_rows(rows, k, n, q, b, False)
    assert np.array_equal(back, w) and np.array_equal(mx, w.max(axis=-1))
