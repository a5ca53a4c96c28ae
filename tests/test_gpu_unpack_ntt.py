"""poly_unpack_ntt on the GPU, bit-exact against the numpy model
(unpack_ntt_model.py: pack_model.unpack_rows, the oracle's poly_ntt, the
negation).

Every device buffer lies between guard words and every output word starts as
a sentinel; a row's gap bytes hold a random pattern the kernel must not look
at; the pstride - n words after each polynomial are still the sentinel
afterwards (for pstride = 2n: slot 0 of a [k][2][n] buffer keeps its pattern);
the inputs are checked unchanged.

Geometry the shapes are taken from (csrc/ntt_unpack_ntt.hpp, k_ntt_fwd's): a
workgroup is 8 waves; a wave unit is one n = 2048 polynomial or two n = 1024
ones, one per half-wave.  batch k = 1 is one wave (n = 1024: half a wave, the
other half loading the same polynomial and storing nothing).  batch 3, k 5 is
15 polynomials: at n = 1024 an odd count whose last unit is half invalid and
whose units straddle rows; at n = 2048 two workgroups, the second with 7 of
its 8 waves at work.  A workgroup walks a second pass only from 2 * 8 * CUs * 4
units on: test_chunk_walk.
"""
import numpy as np
import pytest
import torch

import pack_model as M
import unpack_ntt_model as U
from conftest import PARAM_SETS

pytestmark = pytest.mark.gpu

WIDTHS = (8, 9, 20, 22, 23, 24, 29, 30)
GUARD = 64           # guard bytes / words on each side: keeps every view 16-byte aligned
SENT8 = 0x5A
SENT32 = 0xA5A5A5A5
SENT32_I = int(np.uint32(SENT32).view(np.int32))
GAP = 48


def _widths(q, signed):
    legal = M.bits_range(q, signed)
    return [b for b in WIDTHS if b in legal]


def _byte_buf(dev, rows):
    buf = torch.full((rows.size + 2 * GUARD,), SENT8, dtype=torch.uint8, device=dev)
    view = buf[GUARD:GUARD + rows.size].view(rows.shape)
    view.copy_(torch.from_numpy(rows).to(dev))
    return buf, view


def _word_buf(dev, count):
    buf = torch.full((count + 2 * GUARD,), SENT32_I, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + count]


def _guards_intact(buf, sentinel):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all())


def _rows_of_fields(rng, f, bits, gap=GAP):
    """fields [batch, k, n] packed back to back, then a random gap"""
    batch = f.shape[0]
    packed = M.pack_fields(f, bits).reshape(batch, -1)
    rows = np.empty((batch, packed.shape[1] + gap), dtype=np.uint8)
    rows[:, :packed.shape[1]] = packed
    rows[:, packed.shape[1]:] = rng.integers(0, 256, (batch, gap), dtype=np.uint8)
    return rows


def _random_rows(rng, batch, k, n, bits, gap=GAP):
    """random bytes: every field value, unsigned ones on both sides of q at the set's full width"""
    return rng.integers(0, 256, (batch, k * n * bits // 8 + gap), dtype=np.uint8)


def _check(ntt, oracle, dev, ps, rows, k, bits, signed, neg, with_max, pstride, stream=None):
    """poly_unpack_ntt of the host rows [batch, stride] against the model; returns the device's [batch, k, n]"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    batch = rows.shape[0]
    npoly = batch * k
    want, want_max = U.unpack_ntt_rows(oracle, rows, ps, k, bits, signed, neg)
    ibuf, inp = _byte_buf(dev, rows)
    mbuf, tm = _word_buf(dev, npoly)
    if pstride == 2 * n:
        # slot 1 of [batch][k][2][n] rows, through the view from word n on; slot 0 holds a pattern that must survive
        obuf, whole = _word_buf(dev, npoly * 2 * n)
        pattern = (np.arange(npoly * n, dtype=np.uint32) * np.uint32(2654435761)).reshape(npoly, n)
        whole.view(npoly, 2, n)[:, 0, :] = ntt.from_numpy_u32(pattern, dev)
        out = whole[n:]
        expect = np.concatenate([pattern[0], U.place(want, pstride, 0)])
        expect.reshape(npoly, 2, n)[:, 0, :] = pattern
    else:
        # batch k pstride words: the gap behind the last polynomial is part of the tensor
        obuf, whole = _word_buf(dev, npoly * pstride)
        out = whole
        expect = U.place(want, pstride, SENT32, npoly * pstride)
    got = ntt.poly_unpack_ntt(out, inp, ps, bits, k, signed=signed, negate=neg, pstride=pstride,
                              maxima=tm if with_max else None, stream=stream)
    if stream is not None:
        stream.synchronize()
    where = f"{ps} batch {batch} k {k} bits {bits} signed {signed} neg {neg} max {with_max} pstride {pstride}"
    assert got[0] is out and got[1] is (tm if with_max else None)
    assert _guards_intact(obuf, SENT32_I) and _guards_intact(mbuf, SENT32_I), where + ": store outside the outputs"
    have = ntt.to_numpy_u32(whole)
    assert np.array_equal(have, expect), where + ": output words or the words between polynomials"
    if with_max:
        assert np.array_equal(ntt.to_numpy_u32(tm).reshape(batch, k), want_max), where + ": maxima"
    else:
        assert bool((tm == SENT32_I).all()), where + ": maxima written though not asked for"
    assert np.array_equal(inp.cpu().numpy(), rows) and _guards_intact(ibuf, SENT8), where + ": input changed"
    assert int(want.max()) < q
    return want


@pytest.mark.parametrize("signed", (True, False), ids=("signed", "unsigned"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_one_polynomial(ntt, oracle, dev, ps, signed):
    """batch k = 1: every width, both signs of the output, with and without maxima"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0x0117 + n + signed)
    for bits in _widths(q, signed):
        rows = _random_rows(rng, 1, 1, n, bits)
        for neg in (False, True):
            for with_max in (False, True):
                _check(ntt, oracle, dev, ps, rows, 1, bits, signed, neg, with_max, n)


@pytest.mark.parametrize("signed", (True, False), ids=("signed", "unsigned"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_rows_and_units(ntt, oracle, dev, ps, signed):
    """batch 3, k 5, a 48-byte gap: every width; the output's sign, the maxima
    and pstride in {n, 2n, n + 4} go round with the widths, and the set's
    widest field takes all three pstride under both signs"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0x3515 + n + signed)
    strides = (n, 2 * n, n + 4)
    widths = _widths(q, signed)
    for i, bits in enumerate(widths):
        rows = _random_rows(rng, 3, 5, n, bits)
        _check(ntt, oracle, dev, ps, rows, 5, bits, signed, bool(i & 1), bool(i & 2), strides[i % 3])
    rows = _random_rows(rng, 3, 5, n, widths[-1])
    for pstride in strides:
        for neg in (False, True):
            _check(ntt, oracle, dev, ps, rows, 5, widths[-1], signed, neg, True, pstride)


@pytest.mark.parametrize("ps,bits", (("ref", 24), ("p-I", 29), ("p-III", 30)))
def test_unsigned_fields_at_and_above_q(ntt, oracle, dev, ps, bits):
    """fields q, q + 1, 2^b - 1 in a few positions (a polynomial's first and last
    coefficient, a lane's last register, the half-wave boundary) among fields
    < q: f - q enters the transform and the maximum is >= q; a polynomial
    without such a field reports a maximum < q"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0xAB0 + n)
    f = rng.integers(0, q, (2, 3, n), dtype=np.uint32)
    for i, p in enumerate((0, 31, 32, 63, 64, n // 2, n - 64, n - 1)):
        f[0, i % 3, p] = (q, q + 1, (1 << bits) - 1)[i % 3]
    f[1, 2, n - 1] = q
    rows = _rows_of_fields(rng, f, bits)
    _, mx = M.unpack_rows(rows, 3, n, q, bits, False)
    assert (mx >= q).tolist() == [[True, True, True], [False, False, True]]
    for neg in (False, True):
        _check(ntt, oracle, dev, ps, rows, 3, bits, False, neg, True, 2 * n)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_signed_extremes(ntt, oracle, dev, ps):
    """-2^(b-1), which reports 2^(b-1), and 2^(b-1) - 1, planted among fields of
    +-1 at the ends of the polynomial and of a lane's registers"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0xE7 + n)
    for bits in (8, M.qbits(q) - 1):
        lo, hi, m = 1 << (bits - 1), (1 << (bits - 1)) - 1, (1 << bits) - 1
        pos = (0, 1, 63, n // 2 - 1, n - 64, n - 1)
        f = np.where(rng.integers(0, 2, (len(pos), 2, n)) == 1, 1, m).astype(np.uint32)
        for i, p in enumerate(pos):
            f[i, 0, p] = lo
            f[i, 1, p] = hi
        rows = _rows_of_fields(rng, f, bits)
        _, mx = M.unpack_rows(rows, 2, n, q, bits, True)
        assert mx.tolist() == [[lo, hi]] * len(pos)
        _check(ntt, oracle, dev, ps, rows, 2, bits, True, True, True, n)
        _check(ntt, oracle, dev, ps, rows, 2, bits, True, False, True, n + 4)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_zero_stays_zero(ntt, oracle, dev, ps):
    """all-zero fields with neg = 1: every output word is 0, never q"""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(1)
    for signed, bits in ((False, M.qbits(q)), (True, 20)):
        rows = _rows_of_fields(rng, np.zeros((2, 2, n), dtype=np.uint32), bits)
        want = _check(ntt, oracle, dev, ps, rows, 2, bits, signed, True, True, 2 * n)
        assert not want.any()


def test_non_default_stream(ntt, oracle, dev):
    ps = "p-III"
    n = ntt.param_info(ps)["n"]
    rng = np.random.default_rng(5)
    rows = _random_rows(rng, 3, 2, n, 30)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    _check(ntt, oracle, dev, ps, rows, 2, 30, False, True, True, 2 * n, stream=s)


@pytest.mark.parametrize("ps", ("p-I", "p-III"))
def test_chunk_walk(ntt, dev, ps):
    """The smallest count at which a workgroup walks two passes and the last
    workgroup's second pass holds one unit: batch_shape gives chunk 2 from
    2 * (8 waves * CUs * 4 workgroups per CU) units on, a workgroup then takes 16
    units, so 64 CUs + 8 + 1 units; at n = 1024 that is twice as many
    polynomials less one, so that the last unit's second half is invalid too.
    k = 1, unsigned, the set's full width, random bytes; against the device's own
    poly_unpack + poly_ntt + negation, which their own tests pin."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    bits = M.qbits(q)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    units = 2 * 8 * cus * 4 + 8 + 1
    npoly = units if n == 2048 else 2 * units - 1
    stride = n * bits // 8 + 16
    g = torch.Generator(device=dev).manual_seed(0xC4A + n)
    rows = torch.randint(0, 256, (npoly, stride), generator=g, dtype=torch.uint8, device=dev)
    before = rows.clone()
    t = torch.empty((npoly, n), dtype=torch.int32, device=dev)
    mx = torch.empty(npoly, dtype=torch.int32, device=dev)
    ntt.poly_unpack(t, rows, ps, bits, signed=False, maxima=mx)
    ntt.poly_ntt(t, ps)
    want = (q - t).remainder(q)
    obuf, out = _word_buf(dev, npoly * n)
    mbuf, tm = _word_buf(dev, npoly)
    ntt.poly_unpack_ntt(out, rows, ps, bits, 1, negate=True, maxima=tm)
    assert _guards_intact(obuf, SENT32_I) and _guards_intact(mbuf, SENT32_I)
    assert torch.equal(out.view(npoly, n), want)
    assert torch.equal(tm, mx)
    assert torch.equal(rows, before)


def test_wrapper_checks(ntt, dev):
    ps, n, bits, k = "p-III", 2048, 30, 2
    packed = k * n * bits // 8
    rows = torch.zeros((2, packed + 32), dtype=torch.uint8, device=dev)
    out = torch.zeros(2 * k * 2 * n, dtype=torch.int32, device=dev)
    mx = torch.zeros(2 * k, dtype=torch.int32, device=dev)
    ntt.poly_unpack_ntt(out, rows.view(torch.int8), ps, bits, k, pstride=2 * n, maxima=mx)   # batch k pstride elements
    ntt.poly_unpack_ntt(out[n:], rows, ps, bits, k, pstride=2 * n)                          # ending with the last polynomial
    ntt.poly_unpack_ntt(out[:2 * k * n].view(2, k, n), rows, ps, bits, k)                   # dense, any contiguous shape
    for bad in (dict(bits=7), dict(bits=31), dict(bits=30, signed=True), dict(k=0), dict(k=9), dict(pstride=n - 4),
                dict(pstride=n + 2), dict(pstride=n + 4)):
        kw = dict(dict(bits=bits, k=k, pstride=2 * n), **bad)
        with pytest.raises(ValueError):
            ntt.poly_unpack_ntt(out, rows, ps, kw.pop("bits"), kw.pop("k"), **kw)
    with pytest.raises(ValueError):
        ntt.poly_unpack_ntt(out[n + 4:], rows, ps, bits, k, pstride=2 * n)             # neither of the two sizes
    with pytest.raises(ValueError):
        ntt.poly_unpack_ntt(out, rows[:, :packed - 16].contiguous(), ps, bits, k, pstride=2 * n)   # stride too short
    with pytest.raises(ValueError):
        ntt.poly_unpack_ntt(out, rows[:, :packed + 16], ps, bits, k, pstride=2 * n)    # not contiguous
    with pytest.raises(ValueError):
        ntt.poly_unpack_ntt(out, rows.view(-1), ps, bits, k, pstride=2 * n)            # not [batch, stride]
    with pytest.raises(ValueError):
        ntt.poly_unpack_ntt(out, rows, ps, bits, k, pstride=2 * n, maxima=mx[:1])
    with pytest.raises(ValueError):
        ntt.poly_unpack_ntt(out, rows.cpu(), ps, bits, k, pstride=2 * n)
    with pytest.raises(TypeError):
        ntt.poly_unpack_ntt(out.to(torch.int64), rows, ps, bits, k, pstride=2 * n)
    with pytest.raises(TypeError):
        ntt.poly_unpack_ntt(out, rows.view(torch.int16), ps, bits, k, pstride=2 * n)
    with pytest.raises(ntt.NTTError):                                                   # NTT_ERR_PARAM: n > 2048
        ntt.poly_unpack_ntt(torch.zeros(4096, dtype=torch.int32, device=dev),
                            torch.zeros((1, 4096 * bits // 8), dtype=torch.uint8, device=dev), "p-III-4096", bits, 1)
