"""poly_pack / poly_unpack without a GPU: their argument validation with fake
pointers (validation fails before any GPU work), every NTT_ERR_* and each limit
on both sides, the documented order of checks, the header's declarations and
the wrappers' signatures."""
import pytest

SETS = ("ref", "p-I", "p-III", "p-III-4096", "p-III-8192")
QBITS = {"ref": 24, "p-I": 29, "p-III": 30, "p-III-4096": 30, "p-III-8192": 30}
FAKE = 0x100000      # never dereferenced
FAR = 0x1000000000   # 64 GiB apart: no two fake buffers overlap
BYTES, W, MAX = FAKE, FAKE + FAR, FAKE + 2 * FAR


def test_header_and_wrappers(ntt):
    import inspect
    with open(ntt.HEADER_PATH) as f:
        h = f.read()
    assert "int poly_pack(uint8_t *d_out, size_t stride, const uint32_t *d_w, size_t batch," in h
    assert "int k, int bits, int sgn, int param_set, void *stream);" in h
    assert "int poly_unpack(uint32_t *d_w, uint32_t *d_max /* [batch][k] or NULL */, const uint8_t *d_in," in h
    assert "size_t stride, size_t batch, int k, int bits, int sgn, int param_set, void *stream);" in h
    for phrase in ("Field i", "stream bits [i b, (i+1) b)", "poly_pack never writes them", "poly_unpack never reads them",
                   "poly_pack(poly_unpack(bytes)) == bytes", "NTT_ERR_SIZE   batch * k > 2^31 - 1"):
        assert phrase in h, phrase
    sig = inspect.signature(ntt.poly_pack)
    assert list(sig.parameters) == ["out", "w", "param_set", "bits", "signed", "stream"]
    assert sig.parameters["signed"].default is True and sig.parameters["stream"].default is None
    sig = inspect.signature(ntt.poly_unpack)
    assert list(sig.parameters) == ["w", "inp", "param_set", "bits", "signed", "maxima", "stream"]
    assert sig.parameters["signed"].default is True and sig.parameters["maxima"].default is None
    assert sig.parameters["stream"].default is None
    import pack_model
    for ps in SETS:
        assert pack_model.qbits(ntt.param_info(ps)["q"]) == QBITS[ps]
        assert pack_model.PRIMES[ps] == ntt.param_info(ps)["q"]


def _calls(ntt, ps, n):
    """pack and unpack with the same keyword arguments; stride None: the packed length"""
    L = ntt.lib()

    def stride_of(stride, k, bits):
        return k * n * bits // 8 if stride is None else stride

    def pack(by=BYTES, w=W, mx=MAX, stride=None, batch=3, k=1, bits=20, sgn=1, ps=ps):
        return L.poly_pack(by, stride_of(stride, k, bits), w, batch, k, bits, sgn, ps, None)

    def unpack(by=BYTES, w=W, mx=MAX, stride=None, batch=3, k=1, bits=20, sgn=1, ps=ps):
        return L.poly_unpack(w, mx, by, stride_of(stride, k, bits), batch, k, bits, sgn, ps, None)
    return pack, unpack


@pytest.mark.parametrize("ps", SETS)
def test_validation(ntt, ps):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E = ntt
    n = ntt.param_info(ps)["n"]
    qb = QBITS[ps]
    for call in _calls(ntt, ntt.PARAM_SETS[ps], n):
        for bad_ps in (-1, 5):
            assert call(ps=bad_ps) == E.NTT_ERR_PARAM
        for k in (-1, 0, 9):
            assert call(k=k, stride=1 << 20) == E.NTT_ERR_PARAM
        for sgn in (-1, 2):
            assert call(sgn=sgn) == E.NTT_ERR_PARAM
        # bits 7 / 8 / qbits - 1 / qbits / qbits + 1 per sgn; an accepted width gets as far as the NULL check
        for sgn, bits, ok in ((1, 7, False), (1, 8, True), (1, qb - 1, True), (1, qb, False), (1, qb + 1, False),
                              (0, 7, False), (0, 8, True), (0, qb - 1, True), (0, qb, True), (0, qb + 1, False),
                              (0, 0, False), (1, -1, False), (0, 32, False), (0, 33, False)):
            want = E.NTT_ERR_NULL if ok else E.NTT_ERR_PARAM
            assert call(by=None, sgn=sgn, bits=bits, stride=1 << 20) == want, (sgn, bits)
        # stride: one step short, and not a multiple of 16
        for k, bits in ((1, 20), (5, qb - 1), (8, 9)):
            packed = k * n * bits // 8
            assert packed % 128 == 0
            assert call(k=k, bits=bits, stride=packed - 16) == E.NTT_ERR_PARAM
            for off in (1, 4, 8, 12, 17):
                assert call(k=k, bits=bits, stride=packed + off) == E.NTT_ERR_PARAM, off
            for stride in (packed, packed + 16, packed + 32):
                assert call(w=None, k=k, bits=bits, stride=stride) == E.NTT_ERR_NULL
        assert call(k=8, w=None) == E.NTT_ERR_NULL
        assert call(by=None) == E.NTT_ERR_NULL
        assert call(w=None) == E.NTT_ERR_NULL
        for kw in (dict(by=BYTES + 8), dict(by=BYTES + 4), dict(by=BYTES + 1), dict(w=W + 8), dict(w=W + 4), dict(w=W + 1)):
            assert call(**kw) == E.NTT_ERR_ALIGN, kw
        # batch * k > 2^31 - 1
        assert call(batch=1 << 31) == E.NTT_ERR_SIZE
        assert call(batch=(1 << 31) // 5 + 1, k=5) == E.NTT_ERR_SIZE
        assert call(batch=1 << 28, k=8) == E.NTT_ERR_SIZE
        assert call(batch=1 << 61, k=8) == E.NTT_ERR_SIZE
        # the byte side against the coefficients: one 16-byte step inside at either end, and equal
        batch, bits = 3, 20
        packed = n * bits // 8
        for stride in (packed, packed + 32):
            bb, wb = (batch - 1) * stride + packed, batch * n * 4
            for by in (W + wb - 16, W - bb + 16, W):
                assert call(by=by, stride=stride) == E.NTT_ERR_ALIAS, (stride, hex(by))
        # (the byte side's extent ends with the last row's fields, not its gap: rows ending exactly where d_w begins
        # overlap nothing and would launch, so that side is left to the GPU tests)
        assert call(batch=0) == E.NTT_OK
        assert call(batch=0, by=None, w=None, mx=None) == E.NTT_OK
        assert call(batch=0, by=BYTES + 1, w=BYTES + 1, mx=BYTES + 1) == E.NTT_OK
        assert call(batch=0, bits=7) == E.NTT_ERR_PARAM
        assert call(batch=0, k=0) == E.NTT_ERR_PARAM
        assert call(batch=0, sgn=2) == E.NTT_ERR_PARAM
        assert call(batch=0, stride=8) == E.NTT_ERR_PARAM
        assert call(batch=0, ps=9) == E.NTT_ERR_PARAM
    # d_max: poly_unpack's alone
    pack, unpack = _calls(ntt, ntt.PARAM_SETS[ps], n)
    for mx in (MAX + 1, MAX + 2):
        assert unpack(mx=mx) == E.NTT_ERR_ALIGN
    assert unpack(mx=None, by=None) == E.NTT_ERR_NULL      # NULL d_max is accepted: the next defect speaks
    assert unpack(mx=None, batch=1 << 31) == E.NTT_ERR_SIZE
    assert unpack(mx=MAX + 4, batch=1 << 31) == E.NTT_ERR_SIZE   # 4-byte alignment is enough
    batch, k, bits = 3, 4, 20
    packed = k * n * bits // 8
    bb, wb, mb = (batch - 1) * packed + packed, batch * k * n * 4, batch * k * 4
    for mx in (W, W + wb - 4, W - mb + 4):                 # the maxima inside d_w's first / last word
        assert unpack(k=k, mx=mx) == E.NTT_ERR_ALIAS, hex(mx)
    for mx in (BYTES, BYTES + bb - 4, BYTES - mb + 4):     # ... and inside the input's
        assert unpack(k=k, mx=mx) == E.NTT_ERR_ALIAS, hex(mx)


def test_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E = ntt
    n = ntt.param_info("p-III")["n"]
    for call in _calls(ntt, ntt.PARAM_SETS["p-III"], n):
        assert call(bits=7, by=None) == E.NTT_ERR_PARAM
        assert call(k=0, w=None, stride=1 << 20) == E.NTT_ERR_PARAM
        assert call(sgn=2, by=BYTES + 8) == E.NTT_ERR_PARAM
        assert call(stride=n * 20 // 8 - 16, batch=1 << 31) == E.NTT_ERR_PARAM
        assert call(stride=n * 20 // 8 + 8, by=W) == E.NTT_ERR_PARAM
        assert call(ps=7, by=W) == E.NTT_ERR_PARAM
        assert call(by=None, w=W + 4) == E.NTT_ERR_NULL
        assert call(w=None, batch=1 << 31) == E.NTT_ERR_NULL
        assert call(w=None, by=BYTES + 1) == E.NTT_ERR_NULL
        assert call(by=BYTES + 8, batch=1 << 31) == E.NTT_ERR_ALIGN    # alignment before the batch limit
        assert call(by=W + 8) == E.NTT_ERR_ALIGN                       # ... and before the overlap
        assert call(by=W, batch=1 << 31) == E.NTT_ERR_SIZE             # the batch limit before the overlap
        assert call(by=W) == E.NTT_ERR_ALIAS
    _, unpack = _calls(ntt, ntt.PARAM_SETS["p-III"], n)
    assert unpack(mx=MAX + 2, by=None) == E.NTT_ERR_NULL
    assert unpack(mx=MAX + 2, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert unpack(mx=W + 2) == E.NTT_ERR_ALIGN
    assert unpack(mx=W, batch=1 << 31) == E.NTT_ERR_SIZE
    assert unpack(mx=W) == E.NTT_ERR_ALIAS
    assert unpack(mx=BYTES) == E.NTT_ERR_ALIAS
