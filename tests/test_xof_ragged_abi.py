"""ntt_xof_ragged without a GPU: the entry point's argument validation with
fake pointers (validation fails before any GPU work), every NTT_ERR_* and each
limit on both sides, the documented order of checks, the exported symbol, the
Python wrapper's own checks (dtypes and shapes come before the devices, so CPU
tensors reach them) and ragged_pack."""
import ctypes

import numpy as np
import pytest
import torch

FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap
OUT, MSG, OFF = FAKE, FAKE + FAR, FAKE + 2 * FAR
S128, S256 = 0, 1


def _call(ntt):
    L = ntt.lib()

    def call(out=OUT, outlen=32, msg=MSG, msg_bytes=64, off=OFF, batch=3, algo=S256, cstm=-1):
        return L.ntt_xof_ragged(out, outlen, msg, msg_bytes, off, batch, algo, cstm, None)
    return call


def test_symbol_and_header(ntt):
    assert ntt.lib().ntt_xof_ragged.argtypes is not None
    assert ctypes.cast(ntt.lib().ntt_xof_ragged, ctypes.c_void_p).value
    with open(ntt.HEADER_PATH) as f:
        h = " ".join(f.read().split())
    assert ("int ntt_xof_ragged(uint8_t *d_out, size_t outlen, const uint8_t *d_msg, size_t msg_bytes, "
            "const uint64_t *d_off, size_t batch, int algo, int cstm, void *stream);") in h


def test_validation(ntt):
    """every call here must fail validation or be an empty batch: a valid one
    would launch on fake pointers"""
    E, call = ntt, _call(ntt)
    for algo in (-1, 2):
        assert call(algo=algo) == E.NTT_ERR_PARAM
    for cstm in (-2, 65536):
        assert call(cstm=cstm) == E.NTT_ERR_PARAM
    for outlen in (0, 4, 12, 520, 516):
        assert call(outlen=outlen) == E.NTT_ERR_PARAM
    for bad in (1, 4, 7, 9, 63, (1 << 32) + 4):
        assert call(msg_bytes=bad) == E.NTT_ERR_PARAM
    # the accepted side of each limit: the call gets as far as the next check
    for kw in (dict(cstm=0), dict(cstm=65535), dict(cstm=-1), dict(algo=S128), dict(outlen=8), dict(outlen=512),
               dict(msg_bytes=0), dict(msg_bytes=8), dict(msg_bytes=1 << 32), dict(msg_bytes=1 << 40)):
        assert call(out=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(out=None), dict(off=None), dict(msg=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    # an empty buffer's pointer is not looked at: NULL, misaligned or inside the output get as far as the next check
    for msg in (None, MSG + 1, OUT):
        assert call(msg=msg, msg_bytes=0, out=OUT + 4) == E.NTT_ERR_ALIGN
        assert call(msg=msg, msg_bytes=0, batch=1 << 31) == E.NTT_ERR_SIZE
        assert call(msg=msg, msg_bytes=0, out=OFF) == E.NTT_ERR_ALIAS
    for kw in (dict(out=OUT + 4), dict(msg=MSG + 4), dict(off=OFF + 4), dict(out=OUT + 1), dict(off=OFF + 1), dict(msg=MSG + 7)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(batch=(1 << 31) - 1, out=None) == E.NTT_ERR_NULL       # the largest batch passes the size check's side
    batch, outlen, msg_bytes = 3, 32, 128
    ob = batch * outlen
    for name, base, size in (("msg", MSG, msg_bytes), ("off", OFF, 8 * (batch + 1))):
        for out in (base + size - 8, base - ob + 8, base):    # one word at either end, and equal
            kw = dict(out=out, outlen=outlen, msg_bytes=msg_bytes, batch=batch)
            assert call(**kw) == E.NTT_ERR_ALIAS, (name, hex(out))
    # empty batch: a no-op whatever the pointers, after the parameter checks
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, out=None, msg=None, off=None) == E.NTT_OK
    assert call(batch=0, out=OUT + 1, msg=MSG + 1, off=OUT + 1) == E.NTT_OK
    assert call(batch=0, outlen=0) == E.NTT_ERR_PARAM
    assert call(batch=0, outlen=12) == E.NTT_ERR_PARAM
    assert call(batch=0, algo=2) == E.NTT_ERR_PARAM
    assert call(batch=0, msg_bytes=4) == E.NTT_ERR_PARAM


def test_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E, call = ntt, _call(ntt)
    assert call(algo=2, out=None) == E.NTT_ERR_PARAM
    assert call(msg_bytes=4, msg=None) == E.NTT_ERR_PARAM
    assert call(outlen=4, batch=1 << 31) == E.NTT_ERR_PARAM
    assert call(out=None, msg=MSG + 4) == E.NTT_ERR_NULL
    assert call(off=None, batch=1 << 31) == E.NTT_ERR_NULL
    assert call(msg=None, out=OUT + 4) == E.NTT_ERR_NULL
    assert call(msg=MSG + 4, batch=1 << 31) == E.NTT_ERR_ALIGN         # alignment before the batch limit
    assert call(out=MSG + 4, batch=3) == E.NTT_ERR_ALIGN               # ... and before the overlap
    assert call(out=MSG, batch=1 << 31) == E.NTT_ERR_SIZE              # the batch limit before the overlap
    assert call(out=MSG, batch=3) == E.NTT_ERR_ALIAS
    assert call(out=OFF, batch=3) == E.NTT_ERR_ALIAS
    assert call(msg=OFF, batch=0x7FFFFFFF, out=None) == E.NTT_ERR_NULL


def test_inputs_may_overlap_each_other(ntt):
    """msg == off passes every check but the output's: only d_out is held apart"""
    E, call = ntt, _call(ntt)
    assert call(msg=OFF, off=OFF, out=OFF) == E.NTT_ERR_ALIAS
    assert call(msg=OFF, off=OFF, out=None) == E.NTT_ERR_NULL


def test_wrapper_rejects_before_the_call(ntt):
    """dtype and shape errors are found on CPU tensors; well-formed CPU tensors are refused as such (no CPU fallback)"""
    out = torch.zeros((3, 32), dtype=torch.uint8)
    msg = torch.zeros(64, dtype=torch.uint8)
    off = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="pad"):
        ntt.xof_ragged(out, msg[:60].clone(), off)                   # not a multiple of 8: the error names the padding rule
    with pytest.raises(ValueError, match="multiple of 8"):
        ntt.xof_ragged(out, msg[:1].clone(), off)
    with pytest.raises(ValueError):
        ntt.xof_ragged(out, msg.view(8, 8), off)                     # not 1-D
    with pytest.raises(ValueError):
        ntt.xof_ragged(out, msg, off[:3].clone())                    # batch offsets, not batch + 1
    with pytest.raises(ValueError):
        ntt.xof_ragged(out, msg, torch.zeros((4, 1), dtype=torch.int64))
    with pytest.raises(ValueError):
        ntt.xof_ragged(out.view(-1), msg, off)
    with pytest.raises(ValueError):
        ntt.xof_ragged(out[:, :12].clone(), msg, off)
    with pytest.raises(ValueError):
        ntt.xof_ragged(torch.zeros((3, 520), dtype=torch.uint8), msg, off)
    with pytest.raises(ValueError):
        ntt.xof_ragged(torch.zeros((3, 64), dtype=torch.uint8)[:, :32], msg, off)   # not contiguous
    with pytest.raises(ValueError):
        ntt.xof_ragged(out, torch.zeros(128, dtype=torch.uint8)[::2], off)
    with pytest.raises(ValueError):
        ntt.xof_ragged(out, msg, torch.zeros(8, dtype=torch.int64)[::2])
    with pytest.raises(TypeError):
        ntt.xof_ragged(out, msg.to(torch.int32), off)
    with pytest.raises(TypeError):
        ntt.xof_ragged(out.to(torch.int16), msg, off)
    with pytest.raises(TypeError):
        ntt.xof_ragged(out, msg, off.to(torch.int32))
    with pytest.raises(ValueError):
        ntt.xof_ragged(out, msg, off, algo="sha3")
    for cstm in (-1, 65536):
        with pytest.raises(ValueError):
            ntt.xof_ragged(out, msg, off, cstm=cstm)
    with pytest.raises(ValueError, match="device tensors"):
        ntt.xof_ragged(out, msg, off)
    with pytest.raises(ValueError, match="device tensors"):
        ntt.xof_ragged(out.to(torch.int8), msg.to(torch.int8), off, algo="shake128", cstm=65535)


def test_ragged_pack(ntt):
    messages = [b"abc", b"", bytes(range(13)), b"", b"\xff" * 8]
    msg, off = ntt.ragged_pack(messages, "cpu")
    assert msg.dtype == torch.uint8 and msg.dim() == 1 and msg.is_contiguous() and msg.numel() == 24
    assert off.dtype == torch.int64 and off.is_contiguous() and off.tolist() == [0, 3, 3, 16, 16, 24]
    assert msg.numpy().tobytes() == b"".join(messages)
    msg, off = ntt.ragged_pack([b"", b"x" * 9], "cpu")
    assert off.tolist() == [0, 0, 9] and msg.numpy().tobytes() == b"x" * 9 + bytes(7)   # zero-padded to a multiple of 8
    for empty in ([], [b""], [b"", b""]):
        msg, off = ntt.ragged_pack(empty, "cpu")
        assert msg.numel() == 0 and msg.dtype == torch.uint8 and off.tolist() == [0] * (len(empty) + 1)
    assert np.array_equal(ntt.ragged_pack([b"12345678"], "cpu")[0].numpy(), np.frombuffer(b"12345678", dtype=np.uint8))
