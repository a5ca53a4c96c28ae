"""ntt_xof on the GPU, exact: SHAKE against hashlib, cshake*_simple against
the plain-Python model (short messages: it costs about 1 ms a permutation).
Both algorithms, message lengths round the rate, every kind of split between
the two segments, output lengths round the rate, batches round the wave and
the workgroup, qTESLA's two H shapes.  The output lies between guard words
over garbage (every byte must be written, none outside) and the inputs must
come back unchanged."""
import hashlib

import numpy as np
import pytest
import torch

import keccak_model as K

pytestmark = pytest.mark.gpu

ALGOS = ("shake128", "shake256")
HASHLIB = {"shake128": hashlib.shake_128, "shake256": hashlib.shake_256}
GUARD = 64   # bytes either side of the output


def totals(rate):
    return (0, 8, rate - 8, rate, rate + 8, 2 * rate + 16)


def splits(total, rate):
    """(all, 0), (0, all) and a boundary inside a rate block (not on a block's edge)"""
    inside = min(max(total // 2 // 8 * 8, 8), max(total - 8, 0))
    if inside % rate == 0 and inside + 8 < total:
        inside += 8
    return sorted({(total, 0), (0, total), (inside, total - inside)})


def reference(algo, msg, outlen, cstm):
    return HASHLIB[algo](msg).digest(outlen) if cstm is None else K.cshake_simple(algo, msg, outlen, cstm)


def run_case(ntt, dev, algo, batch, len0, len1, outlen, cstm=None, seed=0, stream=None, one_segment=False):
    rng = np.random.default_rng([seed, batch, len0, len1, outlen])
    a0 = rng.integers(0, 256, (batch, len0), dtype=np.uint8)
    a1 = rng.integers(0, 256, (batch, len1), dtype=np.uint8)
    t0, t1 = torch.from_numpy(a0).to(dev), torch.from_numpy(a1).to(dev)
    buf = torch.full((batch * outlen + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[GUARD:-GUARD].view(batch, outlen)
    out.fill_(0xDB)
    if stream is not None:
        torch.cuda.synchronize(dev)
    ntt.xof(out, t0, None if one_segment else t1, algo=algo, cstm=cstm, stream=stream)
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    tag = f"{algo} batch {batch} len {len0}+{len1} out {outlen} cstm {cstm}"
    for b in range(batch):
        want = reference(algo, a0[b].tobytes() + a1[b].tobytes(), outlen, cstm)
        assert got[b].tobytes() == want, f"{tag}: message {b}"
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all()), f"{tag}: store outside the output"
    assert np.array_equal(t0.cpu().numpy(), a0) and np.array_equal(t1.cpu().numpy(), a1), f"{tag}: input changed"


@pytest.mark.parametrize("algo", ALGOS)
def test_shake_lengths_and_splits(ntt, dev, algo):
    rate = K.RATE[algo]
    for total in totals(rate):
        for len0, len1 in splits(total, rate):
            run_case(ntt, dev, algo, 65, len0, len1, 32)
    run_case(ntt, dev, algo, 3, rate + 8, 0, 32, one_segment=True)   # in1 = None


@pytest.mark.parametrize("algo", ALGOS)
def test_shake_output_lengths(ntt, dev, algo):
    rate = K.RATE[algo]
    for outlen in (8, 32, rate, rate + 8, 512):
        run_case(ntt, dev, algo, 63, rate - 16, 24, outlen)


@pytest.mark.parametrize("batch", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("algo", ALGOS)
def test_shake_batches(ntt, dev, algo, batch):
    rate = K.RATE[algo]
    run_case(ntt, dev, algo, batch, rate + 40, rate - 24, 32)
    run_case(ntt, dev, algo, batch, 8, 0, rate + 8)


@pytest.mark.parametrize("cstm", (0, 1, 0x1234, 65535))
@pytest.mark.parametrize("algo", ALGOS)
def test_cshake_simple(ntt, dev, algo, cstm):
    rate = K.RATE[algo]
    for total in totals(rate):
        len0, len1 = splits(total, rate)[1 if total else 0]
        run_case(ntt, dev, algo, 3, len0, len1, 32 if total != rate else rate + 8, cstm=cstm)
    run_case(ntt, dev, algo, 65, 8, 8, 32, cstm=cstm)


@pytest.mark.parametrize("algo,hi_bytes", (("shake128", 1024), ("shake256", 10240)))
def test_qtesla_shapes(ntt, dev, algo, hi_bytes):
    """hi bytes || a 64-byte digest: neither a multiple of the rate nor of any power-of-two chunk"""
    run_case(ntt, dev, algo, 65, hi_bytes, 64, 32)
    run_case(ntt, dev, algo, 257, hi_bytes, 64, 32)
    run_case(ntt, dev, algo, 2, hi_bytes, 64, 32, cstm=0x1234)


def test_non_default_stream(ntt, dev):
    s = torch.cuda.Stream(device=dev)
    run_case(ntt, dev, "shake256", 65, 136 + 40, 64, 32, stream=s)
    run_case(ntt, dev, "shake128", 65, 168 + 40, 64, 32, cstm=7, stream=s)


def test_wrapper_rejects_before_the_call(ntt, dev):
    out = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    msg = torch.zeros((3, 64), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ntt.xof(out, msg[:2].contiguous())                      # batch mismatch
    with pytest.raises(ValueError):
        ntt.xof(out, msg[:, :60].contiguous())                  # not a multiple of 8
    with pytest.raises(ValueError):
        ntt.xof(out[:, :12].contiguous(), msg)
    with pytest.raises(TypeError):
        ntt.xof(out, msg.to(torch.int32))
    with pytest.raises(ValueError):
        ntt.xof(out, msg, algo="sha3")
    with pytest.raises(ValueError):
        ntt.xof(out, msg, cstm=65536)
    with pytest.raises(ValueError):
        ntt.xof(out.view(-1), msg)
    with pytest.raises(ValueError):
        ntt.xof(msg[:, :32], msg)                               # not contiguous
    with pytest.raises(ntt.NTTError) as e:
        ntt.xof(msg.view(-1)[:96].view(3, 32), msg)             # the output inside an input: the library's check
    assert e.value.code == ntt.NTT_ERR_ALIAS
