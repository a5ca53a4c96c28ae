"""poly_gen_a without a GPU: its argument validation with fake pointers
(validation fails before any GPU work), every NTT_ERR_* and each limit, the
documented order of checks, the alias extent under pstride, the header's
declaration and the wrapper's signature."""
import pytest

SETS = ("p-I", "p-III", "p-III-4096", "p-III-8192")
FAKE = 0x100000      # never dereferenced
FAR = 0x1000000000   # 64 GiB apart: no two fake buffers overlap
A, SEED = FAKE, FAKE + FAR


def test_header_and_wrapper(ntt):
    import inspect
    with open(ntt.HEADER_PATH) as f:
        h = f.read()
    assert "int poly_gen_a(uint32_t *d_a, size_t pstride, const uint8_t *d_seed, size_t seedlen," in h
    assert "size_t batch, int k, int nblocks, int param_set, void *stream);" in h
    assert "#define NTT_GEN_A_BLOCKS_MAX 256" in h
    for phrase in ("buf = cshake128_simple(seed, outlen = 168 * nblocks, cstm = 0)", "if pos > 168 * nb - 4 * nbytes:",
                   "four times:  v = le32(buf + pos) & mask;  pos += nbytes", "if v < q and i < k * n:  a[i / n][i % n] = v;  i += 1",
                   "4 * floor(168 * nb / (4 * nbytes))", "words 40 and 41 unused", "representation and not scheme",
                   "refills_max(k, n) = min(65535, 4 * ceil(k n / 40))", "get 0", "would need three-byte draws",
                   "((batch k - 1) pstride + n) words", "never written"):
        assert phrase in h, phrase
    sig = inspect.signature(ntt.poly_gen_a)
    assert list(sig.parameters) == ["a", "seed", "param_set", "nblocks", "k", "pstride", "stream"]
    assert sig.parameters["pstride"].default is None and sig.parameters["stream"].default is None
    assert ntt.GEN_A_BLOCKS_MAX == 256
    import gen_a_model
    assert gen_a_model.BLOCKS_MAX == ntt.GEN_A_BLOCKS_MAX
    assert (343576577, 856145921) == (ntt.param_info("p-I")["q"], ntt.param_info("p-III")["q"])   # test_gen_a_model's Q1, Q3
    for ps in SETS:
        assert gen_a_model.nbytes(ntt.param_info(ps)["q"]) == 4
    assert gen_a_model.nbytes(ntt.param_info("ref")["q"]) == 3


def _call(ntt, ps, n):
    L = ntt.lib()

    def call(a=A, seed=SEED, pstride=None, seedlen=32, batch=3, k=4, nblocks=108, ps=ps):
        return L.poly_gen_a(a, n if pstride is None else pstride, seed, seedlen, batch, k, nblocks, ps, None)
    return call


@pytest.mark.parametrize("ps", SETS)
def test_validation(ntt, ps):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E = ntt
    n = ntt.param_info(ps)["n"]
    call = _call(ntt, ntt.PARAM_SETS[ps], n)
    for bad_ps in (-1, 5, ntt.PARAM_SETS["ref"]):
        assert call(ps=bad_ps) == E.NTT_ERR_PARAM
    for k in (-1, 0, 9):
        assert call(k=k) == E.NTT_ERR_PARAM
    for nblocks in (-1, 0, 257, 1 << 20):
        assert call(nblocks=nblocks) == E.NTT_ERR_PARAM
    for seedlen in (0, 4, 12, 33, 168, 176):
        assert call(seedlen=seedlen) == E.NTT_ERR_PARAM
    for pstride in (0, n - 4, n - 1, n + 1, n + 2, n + 3, 2 * n + 6):
        assert call(pstride=pstride) == E.NTT_ERR_PARAM, pstride
    # every accepted limit gets as far as the NULL check
    for kw in (dict(k=1), dict(k=8), dict(nblocks=1), dict(nblocks=256), dict(seedlen=8), dict(seedlen=160),
               dict(pstride=n), dict(pstride=n + 4), dict(pstride=2 * n), dict(pstride=1 << 40)):
        assert call(a=None, **kw) == E.NTT_ERR_NULL, kw
    assert call(a=None) == E.NTT_ERR_NULL
    assert call(seed=None) == E.NTT_ERR_NULL
    for kw in (dict(a=A + 8), dict(a=A + 4), dict(a=A + 1), dict(seed=SEED + 4), dict(seed=SEED + 1)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(seed=SEED + 8, a=None) == E.NTT_ERR_NULL     # 8-byte alignment is enough for the seeds
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(batch=1 << 40) == E.NTT_ERR_SIZE
    # the seeds one 8-byte step inside either end of d_a's extent, which ends with the last polynomial's n
    # words, not with its gap
    batch, k, seedlen = 3, 4, 32
    for pstride in (n, n + 4, 2 * n):
        ext = ((batch * k - 1) * pstride + n) * 4
        for seed in (A + ext - 8, A - batch * seedlen + 8, A, A + 4 * n):
            assert call(seed=seed, pstride=pstride) == E.NTT_ERR_ALIAS, (pstride, hex(seed))
    # (seeds that begin exactly where the extent ends -- inside the last gap's place -- overlap nothing and would
    # launch, so that side is left to the GPU tests)
    ext_dense = ((batch * k - 1) * n + n) * 4
    assert call(seed=A + ext_dense, pstride=2 * n) == E.NTT_ERR_ALIAS    # inside the strided extent ...
    assert call(seed=A + ext_dense + 8 * n, pstride=2 * n) == E.NTT_ERR_ALIAS
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, a=None, seed=None) == E.NTT_OK
    assert call(batch=0, a=A + 1, seed=A + 1) == E.NTT_OK
    assert call(batch=0, k=0) == E.NTT_ERR_PARAM
    assert call(batch=0, nblocks=0) == E.NTT_ERR_PARAM
    assert call(batch=0, seedlen=12) == E.NTT_ERR_PARAM
    assert call(batch=0, pstride=n + 2) == E.NTT_ERR_PARAM
    assert call(batch=0, ps=9) == E.NTT_ERR_PARAM


def test_ref_is_rejected(ntt):
    """a 24-bit prime would need three-byte draws"""
    n = ntt.param_info("ref")["n"]
    call = _call(ntt, ntt.PARAM_SETS["ref"], n)
    assert call() == ntt.NTT_ERR_PARAM
    assert call(batch=0) == ntt.NTT_ERR_PARAM
    assert call(a=None, seed=None) == ntt.NTT_ERR_PARAM


def test_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E = ntt
    n = ntt.param_info("p-III")["n"]
    call = _call(ntt, ntt.PARAM_SETS["p-III"], n)
    assert call(k=0, a=None) == E.NTT_ERR_PARAM
    assert call(nblocks=257, a=A + 4) == E.NTT_ERR_PARAM
    assert call(seedlen=12, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(pstride=n + 2, seed=A) == E.NTT_ERR_PARAM
    assert call(ps=7, seed=A) == E.NTT_ERR_PARAM
    assert call(a=None, seed=SEED + 4) == E.NTT_ERR_NULL
    assert call(seed=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(a=A + 8, batch=1 << 31) == E.NTT_ERR_ALIGN     # alignment before the batch limit
    assert call(a=A + 8, seed=A + 8) == E.NTT_ERR_ALIGN        # ... and before the overlap
    assert call(seed=A, batch=1 << 31) == E.NTT_ERR_SIZE       # the batch limit before the overlap
    assert call(seed=A) == E.NTT_ERR_ALIAS
