"""ntt_xof / poly_challenge without a GPU: both entry points' argument
validation with fake pointers (validation fails before any GPU work), every
NTT_ERR_* and each limit on both sides, and the documented order of checks."""
import pytest

SETS = ("ref", "p-I", "p-III", "p-III-4096", "p-III-8192")
FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap
OUT, IN0, IN1 = FAKE, FAKE + FAR, FAKE + 2 * FAR
S128, S256 = 0, 1


def test_python_constants(ntt):
    assert ntt.XOF_ALGOS == {"shake128": S128, "shake256": S256}
    assert (ntt.XOF_OUT_MAX, ntt.CHALLENGE_H_MAX) == (512, 128)
    with open(ntt.HEADER_PATH) as f:
        h = f.read()
    for line in ("#define NTT_XOF_SHAKE128 0", "#define NTT_XOF_SHAKE256 1", "#define NTT_XOF_OUT_MAX 512",
                 "#define NTT_CHALLENGE_H_MAX 128", "#define NTT_CHALLENGE_BLOCKS_MAX 64"):
        assert line in h


def _xof(ntt):
    L = ntt.lib()

    def call(out=OUT, outlen=32, in0=IN0, len0=64, in1=IN1, len1=64, batch=3, algo=S256, cstm=-1):
        return L.ntt_xof(out, outlen, in0, len0, in1, len1, batch, algo, cstm, None)
    return call


def test_xof_validation(ntt):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E, call = ntt, _xof(ntt)
    for algo in (-1, 2):
        assert call(algo=algo) == E.NTT_ERR_PARAM
    for cstm in (-2, 65536):
        assert call(cstm=cstm) == E.NTT_ERR_PARAM
    for outlen in (0, 4, 12, 520, 516):
        assert call(outlen=outlen) == E.NTT_ERR_PARAM
    for bad in (1, 4, 63, 1 << 32):
        assert call(len0=bad) == E.NTT_ERR_PARAM
        assert call(len1=bad) == E.NTT_ERR_PARAM
    assert call(len0=1 << 31, len1=1 << 31) == E.NTT_ERR_PARAM          # the sum reaches 2^32
    # the accepted side of each limit: the call gets as far as the next check
    for kw in (dict(cstm=0), dict(cstm=65535), dict(cstm=-1), dict(algo=S128), dict(outlen=8), dict(outlen=512),
               dict(len0=(1 << 31), len1=(1 << 31) - 8), dict(len0=0), dict(len1=0), dict(len0=0, len1=0)):
        assert call(out=None, **kw) == E.NTT_ERR_NULL, kw
    assert call(in0=None) == E.NTT_ERR_NULL
    assert call(in1=None) == E.NTT_ERR_NULL
    # a zero-length segment's pointer is not looked at: NULL, misaligned or inside the output
    for in0 in (None, IN0 + 1, OUT):
        assert call(in0=in0, len0=0, out=OUT + 4) == E.NTT_ERR_ALIGN
        assert call(in1=in0, len1=0, out=OUT + 4) == E.NTT_ERR_ALIGN
    for kw in (dict(out=OUT + 4), dict(in0=IN0 + 4), dict(in1=IN1 + 4), dict(out=OUT + 1)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    batch, outlen, len0, len1 = 3, 32, 64, 128
    ob = batch * outlen
    for name, base, size in (("in0", IN0, batch * len0), ("in1", IN1, batch * len1)):
        for out in (base + size - 8, base - ob + 8, base):    # one word at either end, and equal
            kw = dict(out=out, outlen=outlen, len0=len0, len1=len1, batch=batch)
            assert call(**kw) == E.NTT_ERR_ALIAS, (name, hex(out))
    # empty batch: a no-op whatever the pointers, after the parameter checks
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, out=None, in0=None, in1=None) == E.NTT_OK
    assert call(batch=0, out=OUT + 1, in0=IN0 + 1, in1=OUT + 1) == E.NTT_OK
    assert call(batch=0, outlen=0) == E.NTT_ERR_PARAM
    assert call(batch=0, algo=2) == E.NTT_ERR_PARAM


def test_xof_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E, call = ntt, _xof(ntt)
    assert call(algo=2, out=None) == E.NTT_ERR_PARAM
    assert call(len0=4, in0=None) == E.NTT_ERR_PARAM
    assert call(outlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(out=None, in0=IN0 + 4) == E.NTT_ERR_NULL
    assert call(in1=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(in0=IN0 + 4, batch=1 << 31) == E.NTT_ERR_ALIGN        # alignment before the batch limit
    assert call(out=IN0 + 4, batch=3) == E.NTT_ERR_ALIGN              # ... and before the overlap
    assert call(out=IN0, batch=1 << 31) == E.NTT_ERR_SIZE             # the batch limit before the overlap
    assert call(out=IN0, batch=3) == E.NTT_ERR_ALIAS


POS, VAL, SEED = FAKE, FAKE + FAR, FAKE + 2 * FAR


def _chal(ntt, ps):
    L = ntt.lib()

    def call(pos=POS, val=VAL, seed=SEED, seedlen=32, batch=3, h=40, ps=ps):
        return L.poly_challenge(pos, val, seed, seedlen, batch, h, ps, None)
    return call


@pytest.mark.parametrize("ps", SETS)
def test_challenge_validation(ntt, ps):
    E, call = ntt, _chal(ntt, ntt.PARAM_SETS[ps])
    for bad_ps in (-1, 5):
        assert call(ps=bad_ps) == E.NTT_ERR_PARAM
    for h in (0, -1, 129):
        assert call(h=h) == E.NTT_ERR_PARAM
    for seedlen in (0, 4, 12, 168, 164):
        assert call(seedlen=seedlen) == E.NTT_ERR_PARAM
    for kw in (dict(h=1), dict(h=128), dict(seedlen=8), dict(seedlen=160)):
        assert call(pos=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(pos=None), dict(val=None), dict(seed=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(pos=POS + 4), dict(val=VAL + 4), dict(seed=SEED + 4), dict(seed=SEED + 1)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    batch, h, seedlen = 3, 40, 32
    lb, sb = batch * h * 4, batch * seedlen
    assert call(val=POS + lb - 8) == E.NTT_ERR_ALIAS
    assert call(val=POS - lb + 8) == E.NTT_ERR_ALIAS
    assert call(val=POS) == E.NTT_ERR_ALIAS
    for which in ("pos", "val"):
        for p in (SEED + sb - 8, SEED - lb + 8, SEED):
            assert call(**{which: p}) == E.NTT_ERR_ALIAS, (which, hex(p))
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, pos=None, val=None, seed=None) == E.NTT_OK
    assert call(batch=0, pos=POS + 1, val=POS + 1, seed=POS + 1) == E.NTT_OK
    assert call(batch=0, h=0) == E.NTT_ERR_PARAM


def test_challenge_first_defect_decides(ntt):
    E, call = ntt, _chal(ntt, ntt.PARAM_SETS["p-III"])
    assert call(h=0, pos=None) == E.NTT_ERR_PARAM
    assert call(seedlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(pos=None, val=VAL + 4) == E.NTT_ERR_NULL
    assert call(seed=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(val=VAL + 4, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(val=POS + 4) == E.NTT_ERR_ALIGN
    assert call(val=POS, batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(val=POS) == E.NTT_ERR_ALIAS
