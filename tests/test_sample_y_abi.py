"""poly_sample_y without a GPU: its argument validation with fake pointers
(validation fails before any GPU work), every NTT_ERR_* and each limit on both
sides, the documented order of checks, and the constants in the header and in
Python."""
import pytest

SETS = ("ref", "p-I", "p-III", "p-III-4096", "p-III-8192")
FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap
Y, SEED, NONCE = FAKE, FAKE + FAR, FAKE + 2 * FAR
S128, S256 = 0, 1


def test_python_constants(ntt):
    assert ntt.SAMPLE_Y_REFILLS_MAX == 255
    with open(ntt.HEADER_PATH) as f:
        h = f.read()
    assert "#define NTT_SAMPLE_Y_REFILLS_MAX 255" in h
    assert "int poly_sample_y(uint32_t *d_y, const uint8_t *d_seed, size_t seedlen," in h
    import sample_model
    assert sample_model.REFILLS_MAX == ntt.SAMPLE_Y_REFILLS_MAX


def _call(ntt, ps):
    L = ntt.lib()

    def call(y=Y, seed=SEED, seedlen=32, d_nonce=NONCE, nonce=0, batch=3, bits=22, algo=S256, ps=ps):
        return L.poly_sample_y(y, seed, seedlen, d_nonce, nonce, batch, bits, algo, ps, None)
    return call


@pytest.mark.parametrize("ps", SETS)
def test_validation(ntt, ps):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E, call = ntt, _call(ntt, ntt.PARAM_SETS[ps])
    n = ntt.param_info(ps)["n"]
    for bad_ps in (-1, 5):
        assert call(ps=bad_ps) == E.NTT_ERR_PARAM
    for algo in (-1, 2):
        assert call(algo=algo) == E.NTT_ERR_PARAM
    for bits in (-1, 0, 1, 25, 32):
        assert call(bits=bits) == E.NTT_ERR_PARAM
    for nonce in (256, 0xFFFFFFFF):
        assert call(nonce=nonce) == E.NTT_ERR_PARAM
    for seedlen in (0, 4, 12, 33):
        assert call(seedlen=seedlen) == E.NTT_ERR_PARAM
    # one absorb block: 160 bytes for SHAKE128, 128 for SHAKE256
    assert call(algo=S128, seedlen=168) == E.NTT_ERR_PARAM
    assert call(algo=S256, seedlen=136) == E.NTT_ERR_PARAM
    assert call(algo=S256, seedlen=160) == E.NTT_ERR_PARAM
    # the accepted side of each limit: the call gets as far as the next check
    for kw in (dict(bits=2), dict(bits=24), dict(nonce=255), dict(nonce=0), dict(seedlen=8), dict(algo=S128, seedlen=160),
               dict(algo=S256, seedlen=128), dict(algo=S128), dict(d_nonce=None)):
        assert call(y=None, **kw) == E.NTT_ERR_NULL, kw
    assert call(y=None) == E.NTT_ERR_NULL
    assert call(seed=None) == E.NTT_ERR_NULL
    for kw in (dict(y=Y + 8), dict(y=Y + 4), dict(y=Y + 1), dict(seed=SEED + 4), dict(seed=SEED + 1), dict(d_nonce=NONCE + 2),
               dict(d_nonce=NONCE + 1)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    # a seed row and a nonce need no more than 8 and 4 bytes; NULL d_nonce is accepted: the next check speaks
    for kw in (dict(seed=SEED + 8), dict(d_nonce=NONCE + 4), dict(d_nonce=None), dict(y=Y + 16)):
        assert call(batch=1 << 31, **kw) == E.NTT_ERR_SIZE, kw
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    batch, seedlen = 3, 32
    yb, sb, nb = batch * n * 4, batch * seedlen, batch * 4
    for y in (SEED + sb - 16, SEED - yb + 16, SEED):     # one 16-byte step inside at either end, and equal
        assert call(y=y) == E.NTT_ERR_ALIAS, hex(y)
    assert nb < 16
    for y in (NONCE - yb + 16, NONCE):                   # the nonces inside y's last / first 16 bytes
        assert call(y=y) == E.NTT_ERR_ALIAS, hex(y)
    assert call(y=NONCE - 5 * n * 4 + 16, batch=5) == E.NTT_ERR_ALIAS   # 20 bytes of nonces, 16 of them inside y
    # d_y ending where the seeds begin overlaps nothing: the call would launch, so only the empty batch is tried
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, y=None, seed=None, d_nonce=None) == E.NTT_OK
    assert call(batch=0, y=Y + 1, seed=Y + 1, d_nonce=Y + 1) == E.NTT_OK
    assert call(batch=0, bits=1) == E.NTT_ERR_PARAM
    assert call(batch=0, nonce=256) == E.NTT_ERR_PARAM
    assert call(batch=0, algo=2) == E.NTT_ERR_PARAM
    assert call(batch=0, seedlen=4) == E.NTT_ERR_PARAM


def test_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E, call = ntt, _call(ntt, ntt.PARAM_SETS["p-III"])
    assert call(bits=1, y=None) == E.NTT_ERR_PARAM
    assert call(nonce=256, seed=None) == E.NTT_ERR_PARAM
    assert call(seedlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(algo=2, y=Y + 8) == E.NTT_ERR_PARAM
    assert call(ps=7, y=SEED) == E.NTT_ERR_PARAM
    assert call(y=None, seed=SEED + 4) == E.NTT_ERR_NULL
    assert call(seed=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(seed=None, d_nonce=NONCE + 2) == E.NTT_ERR_NULL
    assert call(y=Y + 8, batch=1 << 31) == E.NTT_ERR_ALIGN         # alignment before the batch limit
    assert call(d_nonce=NONCE + 2, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(y=SEED + 8) == E.NTT_ERR_ALIGN                     # ... and before the overlap
    assert call(y=SEED, batch=1 << 31) == E.NTT_ERR_SIZE           # the batch limit before the overlap
    assert call(y=SEED) == E.NTT_ERR_ALIAS
    assert call(y=NONCE) == E.NTT_ERR_ALIAS
    assert call(y=NONCE, d_nonce=None, batch=1 << 31) == E.NTT_ERR_SIZE


def test_wrapper_is_there(ntt):
    """the Python entry point and its defaults (the GPU tests call it)"""
    import inspect
    sig = inspect.signature(ntt.poly_sample_y)
    assert list(sig.parameters) == ["y", "seed", "param_set", "bits", "algo", "nonce", "nonces", "stream"]
    assert (sig.parameters["algo"].default, sig.parameters["nonce"].default) == ("shake256", 0)
    assert sig.parameters["nonces"].default is None and sig.parameters["stream"].default is None
