"""poly_pack / poly_unpack on the GPU, bit-exact against the numpy model
(pack_model.py).

Every device buffer lies between guard words and every output word starts as
a sentinel; a row's gap bytes (stride beyond the packed length) hold a random
pattern that poly_pack must leave intact and poly_unpack must not look at; the
inputs are checked unchanged afterwards.

Geometry the batches are taken from (csrc/ntt_pack.hpp): a wave owns 1024
coefficients, a workgroup is four waves (eight at n = 8192), so at n = 1024 a
workgroup holds four polynomials and batch 7 is two workgroups, the second
with three of its four waves at work; at n = 2048 batch 3 is two workgroups
with the second half full.  A workgroup walks more than one tile only from
2 * 8 * CUs tiles on (16 389 polynomials of n = 1024 on 256 CUs: 2049
workgroups of two tiles, the last tile holding one polynomial); that case is
test_chunk_walk.
"""
import numpy as np
import pytest
import torch

import pack_model as M
from conftest import LARGE_SETS, PARAM_SETS

pytestmark = pytest.mark.gpu

SETS = PARAM_SETS + LARGE_SETS
WIDTHS = (8, 9, 20, 22, 23, 24, 29, 30)
GUARD = 64           # guard bytes / words on each side: keeps every view 16-byte aligned
SENT8 = 0x5A
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))


def _widths(q, signed):
    legal = M.bits_range(q, signed)
    return [b for b in WIDTHS if b in legal]


def _byte_buf(dev, rows):
    """rows (numpy uint8 [batch, stride]) on the device between guards"""
    buf = torch.full((rows.size + 2 * GUARD,), SENT8, dtype=torch.uint8, device=dev)
    view = buf[GUARD:GUARD + rows.size].view(rows.shape)
    view.copy_(torch.from_numpy(rows).to(dev))
    return buf, view


def _word_buf(dev, shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT32, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, sentinel):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all())


def _gap_rows(rng, batch, packed, gap):
    """rows whose packed part is the sentinel and whose gap is a random pattern"""
    rows = np.full((batch, packed + gap), SENT8, dtype=np.uint8)
    rows[:, packed:] = rng.integers(0, 256, (batch, gap), dtype=np.uint8)
    return rows


def _check_pack(ntt, dev, ps, w, bits, signed, gap, rng, stream=None):
    """poly_pack of the host words w [batch, k, n]; returns the rows it must give"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    batch, k, _ = w.shape
    packed = k * n * bits // 8
    before = _gap_rows(rng, batch, packed, gap)
    want = M.pack_rows(w, q, bits, signed, packed + gap, before[:, packed:])
    obuf, out = _byte_buf(dev, before)
    tw = ntt.from_numpy_u32(w, dev)
    got = ntt.poly_pack(out, tw if k > 1 else tw.view(batch, n), ps, bits, signed=signed, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert got is out
    assert _guards_intact(obuf, SENT8), "store outside the rows"
    assert np.array_equal(out.cpu().numpy(), want), f"{ps} batch {batch} k {k} bits {bits} signed {signed} gap {gap}: rows"
    assert np.array_equal(ntt.to_numpy_u32(tw).reshape(w.shape), w), "input changed"
    return want


def _check_unpack(ntt, dev, ps, rows, k, bits, signed, with_max, stream=None):
    """poly_unpack of the host rows [batch, stride]; returns the device's words"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    batch = rows.shape[0]
    want_w, want_max = M.unpack_rows(rows, k, n, q, bits, signed)
    ibuf, inp = _byte_buf(dev, rows)
    wbuf, tw = _word_buf(dev, (batch, k, n))
    mbuf, tm = _word_buf(dev, (batch, k))
    got = ntt.poly_unpack(tw if k > 1 else tw.view(batch, n), inp, ps, bits, signed=signed, maxima=tm if with_max else None,
                          stream=stream)
    if stream is not None:
        stream.synchronize()
    assert got[1] is (tm if with_max else None)
    assert _guards_intact(wbuf, SENT32) and _guards_intact(mbuf, SENT32), "store outside the outputs"
    where = f"{ps} batch {batch} k {k} bits {bits} signed {signed}"
    w = ntt.to_numpy_u32(tw)
    assert np.array_equal(w, want_w), where + ": coefficients"
    if with_max:
        assert np.array_equal(ntt.to_numpy_u32(tm), want_max), where + ": maxima"
    else:
        assert bool((tm == SENT32).all()), "maxima written though not asked for"
    assert np.array_equal(inp.cpu().numpy(), rows) and _guards_intact(ibuf, SENT8), "input changed"
    return w


def _edge_positions(n):
    """first coefficient of the first and last group of every wave (so of the polynomial too)"""
    return sorted({p for wave in range(n // 1024) for p in (1024 * wave, 1024 * wave + 1020)})


def _signed_words(rng, batch, k, n, q, bits):
    """centred values over the whole field range, the four extremes in the first
    and last group of every wave; half of the words in [q, 2q)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    c = rng.integers(lo, hi + 1, (batch, k, n), dtype=np.int64)
    for i, p in enumerate(_edge_positions(n)):
        c[..., p:p + 4] = np.roll(np.array([lo, hi, -1, 0], dtype=np.int64), i)
    w = (c % q).astype(np.uint32)
    w += np.where(rng.integers(0, 2, w.shape) == 1, np.uint32(q), np.uint32(0))
    return w


def _unsigned_words(rng, batch, k, n, q, bits):
    top = min(q, 1 << bits)
    w = rng.integers(0, top, (batch, k, n), dtype=np.uint32)
    for i, p in enumerate(_edge_positions(n)):
        w[..., p:p + 4] = np.roll(np.array([0, top - 1, 1, top // 2], dtype=np.uint32), i)
    w += np.where(rng.integers(0, 2, w.shape) == 1, np.uint32(q), np.uint32(0))
    return w


@pytest.mark.parametrize("signed", (True, False), ids=("signed", "unsigned"))
@pytest.mark.parametrize("ps", SETS)
def test_exact(ntt, dev, ps, signed):
    """every width of WIDTHS the set allows, batch 1 and 3 (n = 8192: eight waves
    for batch 1), stride = packed length + 32: pack against the model, unpack
    of those rows with and without maxima, equal coefficients either way"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0x9AC + n + signed)
    for bits in _widths(q, signed):
        for batch in (1, 3):
            w = (_signed_words if signed else _unsigned_words)(rng, batch, 1, n, q, bits)
            rows = _check_pack(ntt, dev, ps, w, bits, signed, 32, rng)
            a = _check_unpack(ntt, dev, ps, rows, 1, bits, signed, True)
            b = _check_unpack(ntt, dev, ps, rows, 1, bits, signed, False)
            assert np.array_equal(a, b) and np.array_equal(a, w % np.uint32(q))


@pytest.mark.parametrize("ps", SETS)
def test_unsigned_full_width_from_random_bytes(ntt, dev, ps):
    """bits = qbits, unsigned, random bytes: fields on both sides of q in every polynomial"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    bits, batch, k = M.qbits(q), 3, 2
    rng = np.random.default_rng(0xB17E5 + n)
    rows = rng.integers(0, 256, (batch, k * n * bits // 8), dtype=np.uint8)
    f = M.unpack_fields(rows.reshape(batch, k, -1), n, bits)
    assert bool((f < q).any(axis=-1).all()) and bool((f >= q).any(axis=-1).all())
    _, mx = M.unpack_rows(rows, k, n, q, bits, False)
    assert bool((mx >= q).all())
    _check_unpack(ntt, dev, ps, rows, k, bits, False, True)
    _check_unpack(ntt, dev, ps, rows, k, bits, False, False)


@pytest.mark.parametrize("ps", ("p-I", "p-III"))
def test_truncation(ntt, dev, ps):
    """every value outside the field's range: the model's truncation is the expectation"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    bits = 20
    rng = np.random.default_rng(0x7C)
    c = rng.integers(1 << (bits - 1), (q - 1) // 2 + 1, (3, 1, n), dtype=np.int64)
    c = np.where(rng.integers(0, 2, c.shape) == 1, -c - 1, c)          # >= 2^(b-1) or < -2^(b-1)
    w = (c % q).astype(np.uint32)
    rows = _check_pack(ntt, dev, ps, w, bits, True, 0, rng)
    back, _ = M.unpack_rows(rows, 1, n, q, bits, True)
    assert not (back == w).any(), "a value was in range"
    w = rng.integers(1 << bits, q, (3, 1, n), dtype=np.uint32)
    _check_pack(ntt, dev, ps, w, bits, False, 0, rng)


@pytest.mark.parametrize("k", (1, 4, 5))
@pytest.mark.parametrize("ps", ("p-I", "p-III", "p-III-8192"))
def test_rows_and_gaps(ntt, dev, ps, k):
    """k polynomials per row, stride = packed length and + 32: poly_pack leaves
    the gap's pattern intact (_check_pack), poly_unpack of rows that differ in
    their gaps alone gives equal outputs"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0x6A9 + k + n)
    for signed, bits in ((True, 22), (False, M.qbits(q))):
        w = (_signed_words if signed else _unsigned_words)(rng, 3, k, n, q, bits)
        dense = _check_pack(ntt, dev, ps, w, bits, signed, 0, rng)
        a = _check_unpack(ntt, dev, ps, dense, k, bits, signed, True)
        gapped = _check_pack(ntt, dev, ps, w, bits, signed, 32, rng)
        other = gapped.copy()
        other[:, -32:] ^= 0xFF
        assert np.array_equal(gapped[:, :-32], dense)
        b = _check_unpack(ntt, dev, ps, gapped, k, bits, signed, True)
        c = _check_unpack(ntt, dev, ps, other, k, bits, signed, True)
        assert np.array_equal(a, b) and np.array_equal(b, c)


@pytest.mark.parametrize("ps,batch", (("ref", 7), ("p-I", 7), ("p-III", 3), ("p-III", 5), ("p-III-4096", 2), ("p-III-8192", 2)))
def test_more_than_one_workgroup(ntt, dev, ps, batch):
    """two workgroups (module docstring), the second one's tile partly filled where n allows"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(batch + n)
    bits = min(23, M.qbits(q) - 1)
    w = _signed_words(rng, batch, 1, n, q, bits)
    rows = _check_pack(ntt, dev, ps, w, bits, True, 32, rng)
    _check_unpack(ntt, dev, ps, rows, 1, bits, True, True)


def test_chunk_walk(ntt, dev):
    """16 389 polynomials of n = 1024: 4098 tiles, so with 8 workgroups per CU on
    256 CUs a workgroup walks two tiles and the last tile holds one polynomial
    (on a device with fewer CUs the walk is longer; the ends are the same).
    Round trips on the device; the first and last rows against the model."""
    ps, bits, batch = "p-I", 20, 4 * 4096 + 5
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    g = torch.Generator(device=dev).manual_seed(0xC4A)
    c = torch.randint(-(1 << (bits - 1)), 1 << (bits - 1), (batch, n), generator=g, dtype=torch.int32, device=dev)
    w = c.remainder(q)
    stride = n * bits // 8 + 32
    rows = torch.full((batch, stride), SENT8, dtype=torch.uint8, device=dev)
    ntt.poly_pack(rows, w, ps, bits)
    back = torch.full_like(w, SENT32)
    mx = torch.full((batch,), SENT32, dtype=torch.int32, device=dev)
    ntt.poly_unpack(back, rows, ps, bits, maxima=mx)
    assert torch.equal(back, w)
    assert torch.equal(mx, c.abs().max(dim=1).values.to(torch.int32))
    assert bool((rows[:, -32:] == SENT8).all())
    sel = torch.tensor([0, 1, 2, 3, 4, 8191, 8192, batch - 6, batch - 5, batch - 2, batch - 1], device=dev)
    want = M.pack_rows(ntt.to_numpy_u32(w[sel]).reshape(-1, 1, n), q, bits, True, stride, np.full((len(sel), 32), SENT8, np.uint8))
    assert np.array_equal(rows[sel].cpu().numpy(), want)


@pytest.mark.parametrize("ps", ("p-III", "p-III-4096", "p-III-8192"))
def test_planted_maximum(ntt, dev, ps):
    """all fields 1 but one, the polynomial's maximum, in its first or its last
    wave (and there in the first or last group): signed -2^(b-1), which reports
    2^(b-1), and 2^(b-1) - 1; unsigned the largest field"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    pos = (0, 3, 1020, 1023, n - 1024, n - 1021, n - 4, n - 1)
    for signed, bits in ((True, 22), (False, 30)):
        f = np.ones((2 * len(pos), 1, n), dtype=np.uint32)
        for i, p in enumerate(pos):
            f[2 * i, 0, p] = 1 << (bits - 1)                 # signed: -2^(b-1)
            f[2 * i + 1, 0, p] = (1 << (bits - 1)) - 1 if signed else (1 << bits) - 1
        rows = M.pack_fields(f, bits).reshape(len(f), -1)
        _, mx = M.unpack_rows(rows, 1, n, q, bits, signed)
        assert mx[0::2, 0].tolist() == [1 << (bits - 1)] * len(pos)
        _check_unpack(ntt, dev, ps, rows, 1, bits, signed, True)


@pytest.mark.parametrize("ps", SETS)
def test_bytes_round_trip_on_device(ntt, dev, ps):
    """poly_pack(poly_unpack(random bytes)) == bytes, signed, at the set's widest field"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    bits, batch, k = M.qbits(q) - 1, 5, 3
    packed = k * n * bits // 8
    g = torch.Generator(device=dev).manual_seed(0xB0B + n)
    rows = torch.randint(0, 256, (batch, packed + 32), generator=g, dtype=torch.uint8, device=dev)
    w = torch.full((batch, k, n), SENT32, dtype=torch.int32, device=dev)
    ntt.poly_unpack(w, rows, ps, bits)
    again = torch.full_like(rows, SENT8)
    ntt.poly_pack(again, w, ps, bits)
    assert torch.equal(again[:, :packed], rows[:, :packed])
    assert bool((again[:, packed:] == SENT8).all())


def test_non_default_stream(ntt, dev):
    ps = "p-III-8192"
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(5)
    w = _signed_words(rng, 3, 2, n, q, 22)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    rows = _check_pack(ntt, dev, ps, w, 22, True, 32, rng, stream=s)
    _check_unpack(ntt, dev, ps, rows, 2, 22, True, True, stream=s)


def test_wrapper_checks(ntt, dev):
    ps, n, bits = "p-III", 2048, 22
    packed = n * bits // 8
    w = torch.zeros((2, n), dtype=torch.int32, device=dev)
    rows = torch.zeros((2, packed + 32), dtype=torch.uint8, device=dev)
    mx = torch.zeros(2, dtype=torch.int32, device=dev)
    ntt.poly_pack(rows.view(torch.int8), w, ps, bits)        # int8 storage is accepted
    ntt.poly_unpack(w, rows, ps, bits, maxima=mx)
    for bad_bits in (7, 30, 31):
        with pytest.raises(ValueError):
            ntt.poly_pack(rows, w, ps, bad_bits)
    with pytest.raises(ValueError):
        ntt.poly_unpack(w, rows, ps, 31, signed=False)
    with pytest.raises(ValueError):
        ntt.poly_pack(rows[:, :packed - 16].contiguous(), w, ps, bits)     # stride too short
    with pytest.raises(ValueError):
        ntt.poly_pack(rows[:, :packed + 8].contiguous(), w, ps, bits)      # stride not a multiple of 16
    with pytest.raises(ValueError):
        ntt.poly_pack(rows[:, :packed + 16], w, ps, bits)                  # not contiguous
    with pytest.raises(ValueError):
        ntt.poly_pack(rows.view(-1), w, ps, bits)                          # not [batch, stride]
    with pytest.raises(ValueError):
        ntt.poly_pack(rows, w[:1], ps, bits)                               # batch mismatch
    with pytest.raises(ValueError):
        ntt.poly_pack(rows, w.view(-1), ps, bits)                          # flat w
    with pytest.raises(ValueError):
        ntt.poly_unpack(w, rows, ps, bits, maxima=mx[:1])
    with pytest.raises(ValueError):
        ntt.poly_unpack(w, rows.cpu(), ps, bits)
    with pytest.raises(ValueError):
        ntt.poly_pack(torch.zeros((2, 9 * packed), dtype=torch.uint8, device=dev),
                      torch.zeros((2, 9, n), dtype=torch.int32, device=dev), ps, bits)   # k = 9
    with pytest.raises(TypeError):
        ntt.poly_pack(rows.view(torch.int16), w, ps, bits)
    with pytest.raises(TypeError):
        ntt.poly_unpack(w.to(torch.int64), rows, ps, bits)
    with pytest.raises(TypeError):
        ntt.poly_unpack(w, rows, ps, bits, maxima=mx.to(torch.int16))
