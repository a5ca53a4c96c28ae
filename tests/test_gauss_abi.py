"""poly_sample_gauss and poly_hsum without a GPU: the symbols, their argument
validation with fake pointers (validation fails before any GPU work), every
NTT_ERR_* and each limit on both sides, the documented order of checks, and
the constants in the header and in Python."""
import ctypes

import pytest

SETS = ("ref", "p-I", "p-III", "p-III-4096", "p-III-8192")
FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap
OUT, SEED, NONCE, CDT = FAKE, FAKE + FAR, FAKE + 2 * FAR, FAKE + 3 * FAR
SUM, W = FAKE + 4 * FAR, FAKE + 5 * FAR
S128, S256 = 0, 1


def test_symbols_are_there(ntt):
    L = ctypes.CDLL(ntt.LIB_PATH)
    for name in ("poly_sample_gauss", "poly_hsum"):
        assert hasattr(L, name), name


def test_python_constants(ntt):
    assert (ntt.GAUSS_CHUNK, ntt.GAUSS_ROWS_MAX, ntt.GAUSS_COLS_MAX) == (512, 128, 4)
    with open(ntt.HEADER_PATH) as f:
        h = f.read()
    for line in ("#define NTT_GAUSS_CHUNK 512", "#define NTT_GAUSS_ROWS_MAX 128", "#define NTT_GAUSS_COLS_MAX 4",
                 "int poly_sample_gauss(uint32_t *d_out, const uint8_t *d_seed, size_t seedlen,",
                 "int poly_hsum(uint64_t *d_sum, const uint32_t *d_w, size_t batch, int h,"):
        assert line in h, line
    import gauss_model
    assert (gauss_model.CHUNK, gauss_model.ROWS_MAX, gauss_model.COLS_MAX) == (512, 128, 4)
    assert all(ntt.param_info(ps)["n"] % ntt.GAUSS_CHUNK == 0 and ntt.param_info(ps)["n"] // ntt.GAUSS_CHUNK <= 16 for ps in SETS)


def _gauss(ntt, ps):
    L = ntt.lib()

    def call(out=OUT, seed=SEED, seedlen=32, d_nonce=NONCE, nonce=0, cdt=CDT, rows=77, cols=2, batch=3, algo=S256, ps=ps):
        return L.poly_sample_gauss(out, seed, seedlen, d_nonce, nonce, cdt, rows, cols, batch, algo, ps, None)
    return call


@pytest.mark.parametrize("ps", SETS)
def test_gauss_validation(ntt, ps):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E, call = ntt, _gauss(ntt, ntt.PARAM_SETS[ps])
    n = ntt.param_info(ps)["n"]
    for bad_ps in (-1, 5):
        assert call(ps=bad_ps) == E.NTT_ERR_PARAM
    for algo in (-1, 2):
        assert call(algo=algo) == E.NTT_ERR_PARAM
    for rows in (-1, 0, 129, 1 << 20):
        assert call(rows=rows) == E.NTT_ERR_PARAM
    for cols in (-1, 0, 5, 8):
        assert call(cols=cols) == E.NTT_ERR_PARAM
    for nonce in (256, 0xFFFFFFFF):
        assert call(nonce=nonce) == E.NTT_ERR_PARAM
    for seedlen in (0, 4, 12, 33):
        assert call(seedlen=seedlen) == E.NTT_ERR_PARAM
    # one absorb block: 160 bytes for SHAKE128, 128 for SHAKE256
    assert call(algo=S128, seedlen=168) == E.NTT_ERR_PARAM
    assert call(algo=S256, seedlen=136) == E.NTT_ERR_PARAM
    assert call(algo=S256, seedlen=160) == E.NTT_ERR_PARAM
    # the accepted side of each limit: the call gets as far as the next check
    for kw in (dict(rows=1), dict(rows=128), dict(cols=1), dict(cols=3), dict(cols=4), dict(nonce=255), dict(seedlen=8),
               dict(algo=S128, seedlen=160), dict(algo=S256, seedlen=128), dict(algo=S128), dict(d_nonce=None)):
        assert call(out=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(out=None), dict(seed=None), dict(cdt=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(out=OUT + 8), dict(out=OUT + 4), dict(out=OUT + 1), dict(seed=SEED + 4), dict(seed=SEED + 1),
               dict(cdt=CDT + 2), dict(cdt=CDT + 1), dict(d_nonce=NONCE + 2), dict(d_nonce=NONCE + 1)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    # a seed row, a table word and a nonce need no more than 8, 4 and 4 bytes; NULL d_nonce is accepted: the next check speaks
    for kw in (dict(seed=SEED + 8), dict(cdt=CDT + 4), dict(d_nonce=NONCE + 4), dict(d_nonce=None), dict(out=OUT + 16)):
        assert call(batch=1 << 31, **kw) == E.NTT_ERR_SIZE, kw
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    batch, seedlen, rows, cols = 3, 32, 77, 2
    ob, sb, nb, tb = batch * n * 4, batch * seedlen, batch * 4, rows * cols * 4
    for out in (SEED + sb - 16, SEED - ob + 16, SEED):     # one 16-byte step inside at either end, and equal
        assert call(out=out) == E.NTT_ERR_ALIAS, hex(out)
    assert nb < 16
    for out in (NONCE - ob + 16, NONCE):                   # the nonces inside out's last / first 16 bytes
        assert call(out=out) == E.NTT_ERR_ALIAS, hex(out)
    for out in (CDT + tb - 16 + (-tb % 16), CDT - ob + 16, CDT):   # the table's last words, its first, and equal
        assert call(out=out) == E.NTT_ERR_ALIAS, hex(out)
    assert call(out=CDT + 16, rows=5, cols=1) == E.NTT_ERR_ALIAS   # 20 bytes of table, the last word inside out
    # an output that touches none of them would launch, so only the empty batch is tried
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, out=None, seed=None, d_nonce=None, cdt=None) == E.NTT_OK
    assert call(batch=0, out=OUT + 1, seed=OUT + 1, d_nonce=OUT + 1, cdt=OUT + 1) == E.NTT_OK
    assert call(batch=0, rows=0) == E.NTT_ERR_PARAM
    assert call(batch=0, cols=5) == E.NTT_ERR_PARAM
    assert call(batch=0, nonce=256) == E.NTT_ERR_PARAM
    assert call(batch=0, algo=2) == E.NTT_ERR_PARAM
    assert call(batch=0, seedlen=4) == E.NTT_ERR_PARAM


def test_gauss_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E, call = ntt, _gauss(ntt, ntt.PARAM_SETS["p-III"])
    assert call(rows=0, out=None) == E.NTT_ERR_PARAM
    assert call(cols=5, cdt=None) == E.NTT_ERR_PARAM
    assert call(nonce=256, seed=None) == E.NTT_ERR_PARAM
    assert call(seedlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(algo=2, out=OUT + 8) == E.NTT_ERR_PARAM
    assert call(ps=7, out=SEED) == E.NTT_ERR_PARAM
    assert call(out=None, seed=SEED + 4) == E.NTT_ERR_NULL
    assert call(seed=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(cdt=None, d_nonce=NONCE + 2) == E.NTT_ERR_NULL
    assert call(out=OUT + 8, batch=1 << 31) == E.NTT_ERR_ALIGN        # alignment before the batch limit
    assert call(cdt=CDT + 2, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(d_nonce=NONCE + 2, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(out=SEED + 8) == E.NTT_ERR_ALIGN                      # ... and before the overlap
    assert call(out=SEED, batch=1 << 31) == E.NTT_ERR_SIZE            # the batch limit before the overlap
    assert call(out=SEED) == E.NTT_ERR_ALIAS
    assert call(out=NONCE) == E.NTT_ERR_ALIAS
    assert call(out=CDT) == E.NTT_ERR_ALIAS
    assert call(out=NONCE, d_nonce=None, batch=1 << 31) == E.NTT_ERR_SIZE


def _hsum(ntt, ps):
    L = ntt.lib()

    def call(d_sum=SUM, w=W, batch=3, h=25, ps=ps):
        return L.poly_hsum(d_sum, w, batch, h, ps, None)
    return call


@pytest.mark.parametrize("ps", SETS)
def test_hsum_validation(ntt, ps):
    E, call = ntt, _hsum(ntt, ntt.PARAM_SETS[ps])
    n = ntt.param_info(ps)["n"]
    for bad_ps in (-1, 5):
        assert call(ps=bad_ps) == E.NTT_ERR_PARAM
    for h in (-1, 0, n + 1, 1 << 20):
        assert call(h=h) == E.NTT_ERR_PARAM
    for h in (1, n):   # the accepted side: the next check speaks
        assert call(h=h, w=None) == E.NTT_ERR_NULL
    assert call(d_sum=None) == E.NTT_ERR_NULL
    assert call(w=None) == E.NTT_ERR_NULL
    for kw in (dict(w=W + 8), dict(w=W + 4), dict(w=W + 1), dict(d_sum=SUM + 4), dict(d_sum=SUM + 1)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    for kw in (dict(d_sum=SUM + 8), dict(w=W + 16), {}):
        assert call(batch=1 << 31, **kw) == E.NTT_ERR_SIZE, kw
    batch = 3
    wb, sb = batch * n * 4, batch * 8
    for d_sum in (W, W + wb - 8, W - sb + 8, W + 1024):
        assert call(d_sum=d_sum) == E.NTT_ERR_ALIAS, hex(d_sum)
    # sums ending where w begins, or beginning where it ends, would launch: only the empty batch is tried
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, d_sum=None, w=None) == E.NTT_OK
    assert call(batch=0, d_sum=SUM + 1, w=SUM + 1) == E.NTT_OK
    assert call(batch=0, h=0) == E.NTT_ERR_PARAM
    assert call(batch=0, ps=9) == E.NTT_ERR_PARAM


def test_hsum_first_defect_decides(ntt):
    E, call = ntt, _hsum(ntt, ntt.PARAM_SETS["p-I"])
    assert call(h=0, w=None) == E.NTT_ERR_PARAM
    assert call(h=1025, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(ps=5, d_sum=W) == E.NTT_ERR_PARAM
    assert call(w=None, d_sum=SUM + 4) == E.NTT_ERR_NULL
    assert call(d_sum=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(w=W + 8, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(d_sum=W + 4) == E.NTT_ERR_ALIGN
    assert call(d_sum=W, batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(d_sum=W) == E.NTT_ERR_ALIAS


def test_wrappers_are_there(ntt):
    """the Python entry points and their defaults (the GPU tests call them)"""
    import inspect
    sig = inspect.signature(ntt.poly_sample_gauss)
    assert list(sig.parameters) == ["out", "seed", "cdt", "param_set", "algo", "nonce", "nonces", "stream"]
    assert (sig.parameters["algo"].default, sig.parameters["nonce"].default) == ("shake256", 0)
    assert sig.parameters["nonces"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(ntt.poly_hsum)
    assert list(sig.parameters) == ["sums", "w", "param_set", "h", "stream"]
    assert sig.parameters["stream"].default is None
