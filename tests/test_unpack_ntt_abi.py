"""poly_unpack_ntt without a GPU: its argument validation with fake pointers
(validation fails before any GPU work), every row of the header's check table
in order, a later defect beside an earlier one, the extents of the alias rule,
the header's declaration and the wrapper's signature."""
import pytest

SETS = ("ref", "p-I", "p-III")
QBITS = {"ref": 24, "p-I": 29, "p-III": 30}
FAKE = 0x100000      # never dereferenced
FAR = 0x1000000000   # 64 GiB apart: no two fake buffers overlap
BYTES, OUT, MAX = FAKE, FAKE + FAR, FAKE + 2 * FAR


def test_header_and_wrapper(ntt):
    import inspect
    with open(ntt.HEADER_PATH) as f:
        h = f.read()
    assert "int poly_unpack_ntt(uint32_t *d_out, size_t pstride, uint32_t *d_max /* [batch][k] or NULL */," in h
    assert "const uint8_t *d_in, size_t stride, size_t batch, int k, int bits, int sgn," in h
    assert "int neg, int param_set, void *stream);" in h
    for phrase in ("so 0 stays 0", "are never written", "never read", "fills slot 1 of [nkeys][k][2][n] verification rows",
                   "no branch, loop bound, global or LDS address depends on a field's", "((batch k - 1) pstride + n) words"):
        assert phrase in h, phrase
    sig = inspect.signature(ntt.poly_unpack_ntt)
    assert list(sig.parameters) == ["out", "inp", "param_set", "bits", "k", "signed", "negate", "pstride", "maxima", "stream"]
    for name, default in (("signed", False), ("negate", False), ("pstride", None), ("maxima", None), ("stream", None)):
        assert sig.parameters[name].default is default, name


def _call(ntt, ps, n):
    """stride / pstride None: the packed length / n"""
    L = ntt.lib()

    def call(out=OUT, pstride=None, mx=MAX, by=BYTES, stride=None, batch=3, k=1, bits=20, sgn=0, neg=1, ps=ps):
        return L.poly_unpack_ntt(out, n if pstride is None else pstride, mx, by,
                                 k * n * bits // 8 if stride is None else stride, batch, k, bits, sgn, neg, ps, None)
    return call


def test_symbol_is_exported(ntt):
    assert hasattr(ntt.lib(), "poly_unpack_ntt")


@pytest.mark.parametrize("ps", SETS)
def test_validation(ntt, ps):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E = ntt
    n = ntt.param_info(ps)["n"]
    qb = QBITS[ps]
    call = _call(ntt, ntt.PARAM_SETS[ps], n)
    # NTT_ERR_PARAM
    for bad_ps in (-1, 5, ntt.PARAM_SETS["p-III-4096"], ntt.PARAM_SETS["p-III-8192"]):
        assert call(ps=bad_ps, stride=1 << 20, pstride=8192) == E.NTT_ERR_PARAM
    for k in (-1, 0, 9):
        assert call(k=k, stride=1 << 20) == E.NTT_ERR_PARAM
    for sgn in (-1, 2):
        assert call(sgn=sgn) == E.NTT_ERR_PARAM
    for neg in (-1, 2):
        assert call(neg=neg) == E.NTT_ERR_PARAM
    # bits 7 / 8 / qbits - 1 / qbits / qbits + 1 per sgn; an accepted width gets as far as the NULL check
    for sgn, bits, ok in ((1, 7, False), (1, 8, True), (1, qb - 1, True), (1, qb, False), (1, qb + 1, False),
                          (0, 7, False), (0, 8, True), (0, qb - 1, True), (0, qb, True), (0, qb + 1, False),
                          (0, 0, False), (1, -1, False), (0, 32, False), (0, 33, False)):
        want = E.NTT_ERR_NULL if ok else E.NTT_ERR_PARAM
        assert call(by=None, sgn=sgn, bits=bits, stride=1 << 20) == want, (sgn, bits)
    for k, bits in ((1, 20), (5, qb - 1), (8, 9)):
        packed = k * n * bits // 8
        assert call(k=k, bits=bits, stride=packed - 16) == E.NTT_ERR_PARAM
        for off in (1, 4, 8, 12, 17):
            assert call(k=k, bits=bits, stride=packed + off) == E.NTT_ERR_PARAM, off
        for stride in (packed, packed + 16, packed + 48):
            assert call(out=None, k=k, bits=bits, stride=stride) == E.NTT_ERR_NULL
    for pstride in (0, n - 4, n + 1, n + 2, 2 * n + 3):
        assert call(pstride=pstride) == E.NTT_ERR_PARAM, pstride
    for pstride in (n, n + 4, 2 * n, 1 << 20):
        assert call(out=None, pstride=pstride) == E.NTT_ERR_NULL, pstride
    # batch == 0: NTT_OK after the parameters, nothing else is looked at
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, out=None, by=None, mx=None) == E.NTT_OK
    assert call(batch=0, out=BYTES + 1, by=BYTES + 1, mx=BYTES + 1) == E.NTT_OK
    for kw in (dict(bits=7), dict(k=0), dict(sgn=2), dict(neg=2), dict(stride=8), dict(pstride=n + 2), dict(ps=9),
               dict(ps=ntt.PARAM_SETS["p-III-4096"])):
        assert call(batch=0, **kw) == E.NTT_ERR_PARAM, kw
    # NTT_ERR_NULL
    assert call(out=None) == E.NTT_ERR_NULL
    assert call(by=None) == E.NTT_ERR_NULL
    assert call(out=None, by=None, mx=None) == E.NTT_ERR_NULL
    assert call(mx=None, by=None) == E.NTT_ERR_NULL          # NULL d_max is accepted: the next defect speaks
    # NTT_ERR_ALIGN
    for kw in (dict(by=BYTES + 8), dict(by=BYTES + 4), dict(by=BYTES + 1), dict(out=OUT + 8), dict(out=OUT + 4),
               dict(out=OUT + 1), dict(mx=MAX + 1), dict(mx=MAX + 2)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(mx=MAX + 4, batch=1 << 31) == E.NTT_ERR_SIZE   # 4-byte alignment is enough for d_max
    # NTT_ERR_SIZE: batch * k > 2^31 - 1
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(batch=(1 << 31) // 5 + 1, k=5) == E.NTT_ERR_SIZE
    assert call(batch=1 << 28, k=8) == E.NTT_ERR_SIZE
    assert call(batch=1 << 61, k=8) == E.NTT_ERR_SIZE
    assert call(mx=None, batch=1 << 31) == E.NTT_ERR_SIZE


@pytest.mark.parametrize("ps", SETS)
def test_alias_extents(ntt, ps):
    """d_out's extent is ((batch k - 1) pstride + n) words, the byte side's
    (batch - 1) stride + k n bits / 8 bytes, d_max's batch k words: one 16-byte
    (d_max: 4-byte) step inside at either end is an overlap.  (One step outside
    is no defect and would launch on the fake pointers: that side belongs to
    the GPU tests, which place buffers back to back.)"""
    E = ntt
    n = ntt.param_info(ps)["n"]
    call = _call(ntt, ntt.PARAM_SETS[ps], n)
    batch, k, bits = 3, 2, 20
    packed = k * n * bits // 8
    for stride in (packed, packed + 48):
        for pstride in (n, n + 4, 2 * n):
            bb, ob, mb = (batch - 1) * stride + packed, ((batch * k - 1) * pstride + n) * 4, batch * k * 4
            kw = dict(batch=batch, k=k, bits=bits, stride=stride, pstride=pstride)
            for by in (OUT + ob - 16, OUT - bb + 16, OUT, OUT + 4 * n):    # the last: inside the first polynomial's gap or beyond
                assert call(by=by, **kw) == E.NTT_ERR_ALIAS, (stride, pstride, hex(by))
            for mx in (OUT, OUT + ob - 4, OUT - mb + 4):
                assert call(mx=mx, **kw) == E.NTT_ERR_ALIAS, (pstride, hex(mx))
            for mx in (BYTES, BYTES + bb - 4, BYTES - mb + 4):
                assert call(mx=mx, **kw) == E.NTT_ERR_ALIAS, (stride, hex(mx))


def test_interleaved_outputs_are_not_operands(ntt):
    """Slot 1 of [nkeys][k][2][n] rows is written through d_out = rows + n with
    pstride = 2n: its extent lies inside the rows buffer, between slot 0's
    polynomials, and that buffer is no operand of the call.  The rule compares
    extents of operands only, so with the bytes and the maxima elsewhere the
    call passes every check: shown here with an empty batch (a full one would
    launch), and by the same placement failing only once an *operand* is moved
    into the extent."""
    E = ntt
    n = ntt.param_info("p-III")["n"]
    call = _call(ntt, ntt.PARAM_SETS["p-III"], n)
    rows = OUT                       # [3][5][2][n] words
    kw = dict(out=rows + 4 * n, pstride=2 * n, batch=3, k=5, bits=30)
    ob = ((15 - 1) * 2 * n + n) * 4
    # the bytes directly before and directly behind d_out's extent would be accepted: one step inside is not
    assert call(by=rows + 4 * n + ob - 16, **kw) == E.NTT_ERR_ALIAS
    assert call(mx=rows + 4 * n + ob - 4, **kw) == E.NTT_ERR_ALIAS
    # the maxima in a gap of d_out (slot 0 of the second polynomial): inside the extent, an overlap
    assert call(mx=rows + 4 * 2 * n, **kw) == E.NTT_ERR_ALIAS
    # slot 0 of the first polynomial, [rows, rows + n), ends where d_out begins: outside the extent.  With the
    # maxima there the only defect left is the one planted after it in the table's order
    assert call(mx=rows + 4 * n - 60, **dict(kw, batch=1 << 31)) == E.NTT_ERR_SIZE
    assert call(mx=rows + 4 * n - 60, **dict(kw, batch=0)) == E.NTT_OK


def test_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E = ntt
    n = ntt.param_info("p-III")["n"]
    call = _call(ntt, ntt.PARAM_SETS["p-III"], n)
    assert call(bits=7, by=None) == E.NTT_ERR_PARAM
    assert call(k=0, out=None, stride=1 << 20) == E.NTT_ERR_PARAM
    assert call(sgn=2, by=BYTES + 8) == E.NTT_ERR_PARAM
    assert call(neg=2, out=OUT + 4) == E.NTT_ERR_PARAM
    assert call(stride=n * 20 // 8 - 16, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(stride=n * 20 // 8 + 8, by=OUT) == E.NTT_ERR_PARAM
    assert call(pstride=n + 2, by=OUT) == E.NTT_ERR_PARAM
    assert call(pstride=n - 4, out=None) == E.NTT_ERR_PARAM
    assert call(ps=7, by=OUT) == E.NTT_ERR_PARAM
    assert call(ps=ntt.PARAM_SETS["p-III-8192"], out=None, stride=1 << 20, pstride=8192) == E.NTT_ERR_PARAM
    assert call(batch=0, out=OUT + 1, by=OUT + 1, mx=OUT + 1) == E.NTT_OK      # an empty batch before everything but PARAM
    assert call(by=None, out=OUT + 4) == E.NTT_ERR_NULL
    assert call(out=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(out=None, by=BYTES + 1) == E.NTT_ERR_NULL
    assert call(by=None, mx=MAX + 2) == E.NTT_ERR_NULL
    assert call(by=BYTES + 8, batch=1 << 31) == E.NTT_ERR_ALIGN    # alignment before the batch limit
    assert call(out=OUT + 8, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(mx=MAX + 2, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(by=OUT + 8) == E.NTT_ERR_ALIGN                     # ... and before the overlap
    assert call(mx=OUT + 2) == E.NTT_ERR_ALIGN
    assert call(by=OUT, batch=1 << 31) == E.NTT_ERR_SIZE           # the batch limit before the overlap
    assert call(mx=OUT, batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(by=OUT) == E.NTT_ERR_ALIAS
    assert call(mx=OUT) == E.NTT_ERR_ALIAS
    assert call(mx=BYTES) == E.NTT_ERR_ALIAS
