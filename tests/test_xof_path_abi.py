"""ntt_xof_path / ntt_xof_ragged_path / ntt_xof_small_batch_max without a GPU:
fake pointers (validation fails before any GPU work).  A bad path is refused
before anything else; for every legal path the validation sequences of
tests/test_xof_abi.py and tests/test_xof_ragged_abi.py give the same codes in
the same order as the unpathed entry points; the header's constants are the
binding's."""
import ctypes

import pytest
import torch

FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap
OUT, IN0, IN1 = FAKE, FAKE + FAR, FAKE + 2 * FAR
MSG, OFF = IN0, IN1
S128, S256 = 0, 1
PATHS = (0, 1, 2)


def _xof(ntt, path):
    L = ntt.lib()

    def call(out=OUT, outlen=32, in0=IN0, len0=64, in1=IN1, len1=64, batch=3, algo=S256, cstm=-1, path=path):
        return L.ntt_xof_path(out, outlen, in0, len0, in1, len1, batch, algo, cstm, path, None)
    return call


def _ragged(ntt, path):
    L = ntt.lib()

    def call(out=OUT, outlen=32, msg=MSG, msg_bytes=64, off=OFF, batch=3, algo=S256, cstm=-1, path=path):
        return L.ntt_xof_ragged_path(out, outlen, msg, msg_bytes, off, batch, algo, cstm, path, None)
    return call


def test_constants_symbols_and_header(ntt):
    assert ntt.XOF_PATHS == {"auto": 0, "lane": 1, "wave": 2}
    assert (ntt.XOF_PATH_AUTO, ntt.XOF_PATH_LANE, ntt.XOF_PATH_WAVE) == (0, 1, 2)
    with open(ntt.HEADER_PATH) as f:
        text = f.read()
    for line in ("#define NTT_XOF_PATH_AUTO 0", "#define NTT_XOF_PATH_LANE 1", "#define NTT_XOF_PATH_WAVE 2"):
        assert line in text
    h = " ".join(text.split())
    for proto in ("int ntt_xof_path(uint8_t *d_out, size_t outlen, const uint8_t *d_in0, size_t len0, const uint8_t *d_in1, "
                  "size_t len1, size_t batch, int algo, int cstm, int path, void *stream);",
                  "int ntt_xof_ragged_path(uint8_t *d_out, size_t outlen, const uint8_t *d_msg, size_t msg_bytes, "
                  "const uint64_t *d_off, size_t batch, int algo, int cstm, int path, void *stream);",
                  "int ntt_xof_small_batch_max(int algo, int ragged, size_t *max_batch);"):
        assert proto in h
    for name in ("ntt_xof_path", "ntt_xof_ragged_path", "ntt_xof_small_batch_max"):
        assert ctypes.cast(getattr(ntt.lib(), name), ctypes.c_void_p).value


@pytest.mark.parametrize("path", (-1, 3))
def test_bad_path_is_refused_first(ntt, path):
    """before the parameters, the empty batch and every pointer check"""
    E, x, r = ntt, _xof(ntt, path), _ragged(ntt, path)
    for call in (x, r):
        assert call() == E.NTT_ERR_PARAM
        assert call(batch=0) == E.NTT_ERR_PARAM
        assert call(batch=0, out=None) == E.NTT_ERR_PARAM
        assert call(out=None) == E.NTT_ERR_PARAM
        assert call(out=OUT + 4) == E.NTT_ERR_PARAM
        assert call(batch=1 << 31) == E.NTT_ERR_PARAM
        assert call(out=IN0) == E.NTT_ERR_PARAM
    assert x(in0=None, in1=None) == E.NTT_ERR_PARAM
    assert r(msg=None, off=None) == E.NTT_ERR_PARAM


@pytest.mark.parametrize("path", PATHS)
def test_xof_validation(ntt, path):
    """tests/test_xof_abi.py::test_xof_validation, through ntt_xof_path: every call
    here must fail validation or be an empty batch"""
    E, call = ntt, _xof(ntt, path)
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
    for kw in (dict(cstm=0), dict(cstm=65535), dict(cstm=-1), dict(algo=S128), dict(outlen=8), dict(outlen=512),
               dict(len0=(1 << 31), len1=(1 << 31) - 8), dict(len0=0), dict(len1=0), dict(len0=0, len1=0)):
        assert call(out=None, **kw) == E.NTT_ERR_NULL, kw
    assert call(in0=None) == E.NTT_ERR_NULL
    assert call(in1=None) == E.NTT_ERR_NULL
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
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, out=None, in0=None, in1=None) == E.NTT_OK
    assert call(batch=0, out=OUT + 1, in0=IN0 + 1, in1=OUT + 1) == E.NTT_OK
    assert call(batch=0, outlen=0) == E.NTT_ERR_PARAM
    assert call(batch=0, algo=2) == E.NTT_ERR_PARAM


@pytest.mark.parametrize("path", PATHS)
def test_xof_first_defect_decides(ntt, path):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI, on every path"""
    E, call = ntt, _xof(ntt, path)
    assert call(algo=2, out=None) == E.NTT_ERR_PARAM
    assert call(len0=4, in0=None) == E.NTT_ERR_PARAM
    assert call(outlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(out=None, in0=IN0 + 4) == E.NTT_ERR_NULL
    assert call(in1=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(in0=IN0 + 4, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(out=IN0 + 4, batch=3) == E.NTT_ERR_ALIGN
    assert call(out=IN0, batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(out=IN0, batch=3) == E.NTT_ERR_ALIAS


@pytest.mark.parametrize("path", PATHS)
def test_ragged_validation(ntt, path):
    """tests/test_xof_ragged_abi.py::test_validation, through ntt_xof_ragged_path"""
    E, call = ntt, _ragged(ntt, path)
    for algo in (-1, 2):
        assert call(algo=algo) == E.NTT_ERR_PARAM
    for cstm in (-2, 65536):
        assert call(cstm=cstm) == E.NTT_ERR_PARAM
    for outlen in (0, 4, 12, 520, 516):
        assert call(outlen=outlen) == E.NTT_ERR_PARAM
    for bad in (1, 4, 7, 9, 63, (1 << 32) + 4):
        assert call(msg_bytes=bad) == E.NTT_ERR_PARAM
    for kw in (dict(cstm=0), dict(cstm=65535), dict(cstm=-1), dict(algo=S128), dict(outlen=8), dict(outlen=512),
               dict(msg_bytes=0), dict(msg_bytes=8), dict(msg_bytes=1 << 32), dict(msg_bytes=1 << 40)):
        assert call(out=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(out=None), dict(off=None), dict(msg=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    for msg in (None, MSG + 1, OUT):
        assert call(msg=msg, msg_bytes=0, out=OUT + 4) == E.NTT_ERR_ALIGN
        assert call(msg=msg, msg_bytes=0, batch=1 << 31) == E.NTT_ERR_SIZE
        assert call(msg=msg, msg_bytes=0, out=OFF) == E.NTT_ERR_ALIAS
    for kw in (dict(out=OUT + 4), dict(msg=MSG + 4), dict(off=OFF + 4), dict(out=OUT + 1), dict(off=OFF + 1), dict(msg=MSG + 7)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(batch=(1 << 31) - 1, out=None) == E.NTT_ERR_NULL
    batch, outlen, msg_bytes = 3, 32, 128
    ob = batch * outlen
    for name, base, size in (("msg", MSG, msg_bytes), ("off", OFF, 8 * (batch + 1))):
        for out in (base + size - 8, base - ob + 8, base):
            kw = dict(out=out, outlen=outlen, msg_bytes=msg_bytes, batch=batch)
            assert call(**kw) == E.NTT_ERR_ALIAS, (name, hex(out))
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, out=None, msg=None, off=None) == E.NTT_OK
    assert call(batch=0, out=OUT + 1, msg=MSG + 1, off=OUT + 1) == E.NTT_OK
    assert call(batch=0, outlen=0) == E.NTT_ERR_PARAM
    assert call(batch=0, outlen=12) == E.NTT_ERR_PARAM
    assert call(batch=0, algo=2) == E.NTT_ERR_PARAM
    assert call(batch=0, msg_bytes=4) == E.NTT_ERR_PARAM


@pytest.mark.parametrize("path", PATHS)
def test_ragged_first_defect_decides(ntt, path):
    E, call = ntt, _ragged(ntt, path)
    assert call(algo=2, out=None) == E.NTT_ERR_PARAM
    assert call(msg_bytes=4, msg=None) == E.NTT_ERR_PARAM
    assert call(outlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(out=None, msg=MSG + 4) == E.NTT_ERR_NULL
    assert call(off=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(msg=None, out=OUT + 4) == E.NTT_ERR_NULL
    assert call(msg=MSG + 4, batch=1 << 31) == E.NTT_ERR_ALIGN
    assert call(out=MSG + 4, batch=3) == E.NTT_ERR_ALIGN
    assert call(out=MSG, batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(out=MSG, batch=3) == E.NTT_ERR_ALIAS
    assert call(out=OFF, batch=3) == E.NTT_ERR_ALIAS
    assert call(msg=OFF, batch=0x7FFFFFFF, out=None) == E.NTT_ERR_NULL
    assert call(msg=OFF, off=OFF, out=OFF) == E.NTT_ERR_ALIAS           # the inputs may overlap each other
    assert call(msg=OFF, off=OFF, out=None) == E.NTT_ERR_NULL


def test_small_batch_max(ntt):
    L, E = ntt.lib(), ntt
    v = ctypes.c_size_t(12345)
    for algo, ragged in ((-1, 0), (2, 0), (S128, -1), (S256, 2)):
        assert L.ntt_xof_small_batch_max(algo, ragged, ctypes.byref(v)) == E.NTT_ERR_PARAM
        assert L.ntt_xof_small_batch_max(algo, ragged, None) == E.NTT_ERR_PARAM    # the parameters come first
    assert v.value == 12345
    for algo in (S128, S256):
        for ragged in (0, 1):
            assert L.ntt_xof_small_batch_max(algo, ragged, None) == E.NTT_ERR_NULL
            assert L.ntt_xof_small_batch_max(algo, ragged, ctypes.byref(v)) == E.NTT_OK
            assert 0 <= v.value <= 0x7FFFFFFF
            name = {S128: "shake128", S256: "shake256"}[algo]
            assert ntt.xof_small_batch_max(name, ragged=bool(ragged)) == v.value
    with pytest.raises(ValueError):
        ntt.xof_small_batch_max("sha3")


def test_wrappers_reject_a_bad_path_before_the_call(ntt):
    out = torch.zeros((3, 32), dtype=torch.uint8)
    msg = torch.zeros(64, dtype=torch.uint8)
    off = torch.zeros(4, dtype=torch.int64)
    for path in ("", "Wave", 2, None):
        with pytest.raises(ValueError, match="path"):
            ntt.xof(out, msg.view(1, 64).expand(3, 64).contiguous(), path=path)
        with pytest.raises(ValueError, match="path"):
            ntt.xof_ragged(out, msg, off, path=path)
    for path in ("auto", "lane", "wave"):   # well-formed CPU tensors are refused as such (no CPU fallback)
        with pytest.raises(ValueError, match="device tensors"):
            ntt.xof_ragged(out, msg, off, path=path)
