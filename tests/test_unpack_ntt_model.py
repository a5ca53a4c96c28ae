"""The numpy statement of poly_unpack_ntt (unpack_ntt_model.py) against itself:
the two signs cancel and are canonical, and the inverse transform of the
result packs back to the input bytes."""
import numpy as np
import pytest

import pack_model as M
import unpack_ntt_model as U
from conftest import PARAM_SETS

WIDTHS = (8, 9, 20, 22, 23, 24, 29, 30)


def _rows(rng, q, n, batch, k, bits, signed, gap):
    """random fields (unsigned: all < q, so that the bytes round-trip), packed, with a random gap"""
    top = (1 << bits) if signed else min(q, 1 << bits)
    f = rng.integers(0, top, (batch, k, n), dtype=np.uint32)
    rows = np.zeros((batch, k * n * bits // 8 + gap), dtype=np.uint8)
    rows[:, :k * n * bits // 8] = M.pack_fields(f, bits).reshape(batch, -1)
    rows[:, k * n * bits // 8:] = rng.integers(0, 256, (batch, gap), dtype=np.uint8)
    return rows


@pytest.mark.parametrize("signed", (True, False), ids=("signed", "unsigned"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_signs_cancel_and_round_trip(oracle, ps, signed):
    p = oracle.params(ps)
    n, q = p["n"], p["q"]
    rng = np.random.default_rng(0x5107 + n + signed)
    batch, k, gap = 2, 3, 48
    for bits in [b for b in WIDTHS if b in M.bits_range(q, signed)]:
        rows = _rows(rng, q, n, batch, k, bits, signed, gap)
        pos, mx0 = U.unpack_ntt_rows(oracle, rows, ps, k, bits, signed, False)
        neg, mx1 = U.unpack_ntt_rows(oracle, rows, ps, k, bits, signed, True)
        assert pos.shape == neg.shape == (batch, k, n) and np.array_equal(mx0, mx1)
        assert int(pos.max()) < q and int(neg.max()) < q
        assert not ((pos.astype(np.int64) + neg.astype(np.int64)) % q).any()
        assert np.array_equal(neg == 0, pos == 0)          # 0 stays 0, never q
        x = oracle.poly_invntt(pos.reshape(-1, n), ps).reshape(batch, k, n)
        again = M.pack_rows(x, q, bits, signed, rows.shape[1], rows[:, -gap:])
        assert np.array_equal(again, rows), (ps, bits, signed)


def test_zero_and_malformed(oracle):
    """all-zero bytes give all-zero output under either sign; an unsigned field
    >= q enters the transform as f - q and shows in the maximum"""
    ps, k = "p-I", 2
    p = oracle.params(ps)
    n, q = p["n"], p["q"]
    rows = np.zeros((1, k * n * 29 // 8 + 16), dtype=np.uint8)
    rows[:, -16:] = 0xFF
    for neg in (False, True):
        X, mx = U.unpack_ntt_rows(oracle, rows, ps, k, 29, False, neg)
        assert not X.any() and not mx.any()
    f = np.zeros((1, k, n), dtype=np.uint32)
    f[0, 1, 7] = q + 5
    rows = M.pack_fields(f, 29).reshape(1, -1)
    X, mx = U.unpack_ntt_rows(oracle, rows, ps, k, 29, False, False)
    g = f.copy()
    g[0, 1, 7] = 5
    assert np.array_equal(X, oracle.poly_ntt(g.reshape(-1, n), ps).reshape(f.shape))
    assert mx.tolist() == [[0, q + 5]]


def test_place():
    X = np.arange(2 * 3 * 4, dtype=np.uint32).reshape(2, 3, 4)
    flat = U.place(X, 6, 99)
    assert flat.size == 5 * 6 + 4
    assert flat.reshape(-1)[:6].tolist() == [0, 1, 2, 3, 99, 99] and flat[-4:].tolist() == [20, 21, 22, 23]
    assert U.place(X, 4, 99).tolist() == list(range(24))
