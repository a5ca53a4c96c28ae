"""The wave-cooperative SHAKE kernels (two messages per wave, path="wave") on
the GPU, exact: SHAKE against hashlib, cshake*_simple against the plain-Python
model (short messages only: about 1 ms a permutation).  Every case runs
path="wave" into an output between guard bytes over garbage, compares it with
the reference and with path="lane", and checks that the inputs come back
unchanged.  The shapes are the smallest at which the kernels take another
path: an idle second half (odd batches), more than one wave and workgroup,
the domain byte and the 0x80 in the same lane, the segment boundary inside a
block, a second squeeze block, the two halves of a wave differing in length
both ways, every start alignment, the clamps, the buffer's last byte."""
import hashlib

import numpy as np
import pytest
import torch

import keccak_model as K

pytestmark = pytest.mark.gpu

ALGOS = ("shake128", "shake256")
HASHLIB = {"shake128": hashlib.shake_128, "shake256": hashlib.shake_256}
GUARD = 64   # bytes either side of the output


def reference(algo, m, outlen, cstm=None):
    return HASHLIB[algo](m).digest(outlen) if cstm is None else K.cshake_simple(algo, m, outlen, cstm)


def guarded(dev, batch, outlen):
    buf = torch.full((batch * outlen + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[GUARD:GUARD + batch * outlen].view(batch, outlen)
    out.fill_(0xDB)
    return buf, out


def guards_intact(buf, batch, outlen):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + batch * outlen:] == 0xA5).all())


def run_xof(ntt, dev, algo, batch, len0, len1, outlen, cstm=None, stream=None, path="wave"):
    rng = np.random.default_rng([31, batch, len0, len1, outlen])
    a0 = rng.integers(0, 256, (batch, len0), dtype=np.uint8)
    a1 = rng.integers(0, 256, (batch, len1), dtype=np.uint8)
    t0, t1 = torch.from_numpy(a0).to(dev), torch.from_numpy(a1).to(dev)
    buf, out = guarded(dev, batch, outlen)
    if stream is not None:
        torch.cuda.synchronize(dev)
    assert ntt.xof(out, t0, t1, algo=algo, cstm=cstm, stream=stream, path=path) is out
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    tag = f"{algo} batch {batch} len {len0}+{len1} out {outlen} cstm {cstm} path {path}"
    for b in range(batch):
        assert got[b].tobytes() == reference(algo, a0[b].tobytes() + a1[b].tobytes(), outlen, cstm), f"{tag}: message {b}"
    assert guards_intact(buf, batch, outlen), f"{tag}: store outside the output"
    assert np.array_equal(t0.cpu().numpy(), a0) and np.array_equal(t1.cpu().numpy(), a1), f"{tag}: input changed"
    if path == "wave":
        lane = torch.empty_like(out)
        ntt.xof(lane, t0, t1, algo=algo, cstm=cstm, path="lane")
        assert torch.equal(lane, out), f"{tag}: differs from path lane"


@pytest.mark.parametrize("batch", (1, 2, 3, 5, 8, 129, 131))
@pytest.mark.parametrize("algo", ALGOS)
def test_batches(ntt, dev, algo, batch):
    """odd batches leave the last wave's second half without a message; 129 and 131 are more than one workgroup at
    either workgroup size, with an odd tail"""
    rate = K.RATE[algo]
    run_xof(ntt, dev, algo, batch, 24, rate - 16, 32)


@pytest.mark.parametrize("algo", ALGOS)
def test_lengths_in_words(ntt, dev, algo):
    R = K.RATE[algo] // 8
    for words in (0, 1, R - 1, R, R + 1, 2 * R, 3 * R + 5):   # R - 1: the domain byte and 0x80 meet in one lane
        run_xof(ntt, dev, algo, 3, 8 * words, 0, 32)


@pytest.mark.parametrize("algo", ALGOS)
def test_segment_boundary(ntt, dev, algo):
    R = K.RATE[algo] // 8
    total = 2 * R + 3
    for w0 in (0, total, 3, R + 2):   # len0 = 0, len1 = 0, and the boundary inside the first and the second block
        run_xof(ntt, dev, algo, 3, 8 * w0, 8 * (total - w0), 32)
    run_xof(ntt, dev, algo, 2, 0, 0, 32)


@pytest.mark.parametrize("algo", ALGOS)
def test_output_lengths(ntt, dev, algo):
    rate = K.RATE[algo]
    for outlen in (8, 32, rate, rate + 8, 512):
        run_xof(ntt, dev, algo, 3, rate - 16, 24, outlen)


@pytest.mark.parametrize("cstm", (None, 0, 0x1234, 65535))
@pytest.mark.parametrize("algo", ALGOS)
def test_cstm(ntt, dev, algo, cstm):
    rate = K.RATE[algo]
    run_xof(ntt, dev, algo, 3, 16, rate, 32, cstm=cstm)
    run_xof(ntt, dev, algo, 1, rate - 8, 0, rate + 8, cstm=cstm)


@pytest.mark.parametrize("algo,hi_bytes", (("shake128", 4096), ("shake256", 10240)))
def test_qtesla_h_shapes(ntt, dev, algo, hi_bytes):
    run_xof(ntt, dev, algo, 3, hi_bytes, 64, 32)


def test_side_stream(ntt, dev):
    s = torch.cuda.Stream(device=dev)
    run_xof(ntt, dev, "shake256", 5, 136 + 40, 64, 32, stream=s)


def messages_of(lengths, seed):
    rng = np.random.default_rng([seed, len(lengths)])
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


def run_ragged(ntt, dev, algo, msg, off, outlen, cstm=None, stream=None, path="wave"):
    """one launch into an output between guards; the digests as a list of bytes, compared with path lane"""
    batch = off.numel() - 1
    msg0, off0 = msg.clone(), off.clone()
    buf, out = guarded(dev, batch, outlen)
    if stream is not None:
        torch.cuda.synchronize(dev)
    assert ntt.xof_ragged(out, msg, off, algo=algo, cstm=cstm, stream=stream, path=path) is out
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    assert guards_intact(buf, batch, outlen), "store outside the output"
    assert torch.equal(msg, msg0) and torch.equal(off, off0), "input changed"
    if path == "wave":
        lane = torch.empty_like(out)
        ntt.xof_ragged(lane, msg, off, algo=algo, cstm=cstm, path="lane")
        assert torch.equal(lane, out), "differs from path lane"
    return [got[b].tobytes() for b in range(batch)]


def check_ragged(ntt, dev, algo, messages, outlen=32, cstm=None, stream=None, path="wave"):
    msg, off = ntt.ragged_pack(messages, dev)
    got = run_ragged(ntt, dev, algo, msg, off, outlen, cstm, stream, path)
    for b, m in enumerate(messages):
        assert got[b] == reference(algo, m, outlen, cstm), f"{algo} cstm {cstm} out {outlen}: message {b} of {len(m)} bytes"
    return off.cpu().numpy()


@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_every_length(ntt, dev, algo, reverse):
    """0 .. 2 rate + 1 in one batch: the halves of a wave differ by one byte, the longer one first or second, and round
    every block edge one of them needs a permutation more than the other"""
    rate = K.RATE[algo]
    lengths = list(range(2 * rate + 2))
    check_ragged(ntt, dev, algo, messages_of(lengths[::-1] if reverse else lengths, 41))


@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_halves_far_apart(ntt, dev, algo):
    """one half finished blocks before the other, both ways, and an odd batch's idle half beside a long message"""
    rate = K.RATE[algo]
    check_ragged(ntt, dev, algo, messages_of([3 * rate + 5, 0, 1, 3 * rate + 5, 0, 2 * rate, rate - 1, 7, 3 * rate], 42))


@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_every_alignment(ntt, dev, algo):
    """the same bytes at begin = a (mod 8) for every a, behind filler messages"""
    rate = K.RATE[algo]
    data = messages_of([rate + 1], 43)[0]
    filler = messages_of([16], 44)[0]
    messages, placed, pos = [], [], 0
    for a in range(8):
        for L in (0, 1, 8 - a, rate - 1, rate, rate + 1):
            f = (a - pos) % 8 + 8 * (len(placed) % 2)
            messages += [filler[:f], data[:L]]
            pos += f
            placed.append((len(messages) - 1, a, L))
            pos += L
    off = check_ragged(ntt, dev, algo, messages)
    assert all(off[b] % 8 == a and off[b + 1] - off[b] == L for b, a, L in placed)
    assert sorted({a for _, a, _ in placed}) == list(range(8))


@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_output_lengths_cstm_and_stream(ntt, dev, algo):
    rate = K.RATE[algo]
    messages = messages_of([rate - 1, 5, rate + 9], 45)
    for outlen in (8, rate, rate + 8, 512):
        check_ragged(ntt, dev, algo, messages, outlen)
    for cstm in (0, 0x1234, 65535):
        check_ragged(ntt, dev, algo, messages, 32, cstm=cstm)
    check_ragged(ntt, dev, algo, messages, 32, stream=torch.cuda.Stream(device=dev))


@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_clamping_is_the_definition(ntt, dev, algo):
    """tests/test_gpu_xof_ragged.py's clamping case: a decreasing pair, a pair past the end and one straddling it, every
    offset inside a 2 M byte allocation"""
    M = 512
    whole = torch.from_numpy(np.random.default_rng(46).integers(0, 256, 2 * M, dtype=np.uint8)).to(dev)
    msg = whole[:M]
    assert msg.is_contiguous() and msg.data_ptr() == whole.data_ptr()
    offsets = [0, 40, 24, 100, M + 16, M + 8, 2 * M - 8]
    off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    host = whole.cpu().numpy().tobytes()[:M]
    spans = []
    for b in range(len(offsets) - 1):
        begin = min(offsets[b], M)
        spans.append((begin, min(max(offsets[b + 1], begin), M)))
    assert spans == [(0, 40), (40, 40), (24, 100), (100, M), (M, M), (M, M)]
    got = run_ragged(ntt, dev, algo, msg, off, 32)
    for b, (begin, end) in enumerate(spans):
        assert got[b] == reference(algo, host[begin:end], 32), f"{algo}: message {b} = [{begin}, {end})"


@pytest.mark.parametrize("algo", ALGOS)
def test_ragged_empty_buffer_and_last_byte(ntt, dev, algo):
    rate = K.RATE[algo]
    msg = torch.empty(0, dtype=torch.uint8, device=dev)
    off = torch.zeros(4, dtype=torch.int64, device=dev)
    assert run_ragged(ntt, dev, algo, msg, off, 32) == [reference(algo, b"", 32)] * 3
    assert run_ragged(ntt, dev, algo, msg, off, 32, cstm=5) == [reference(algo, b"", 32, 5)] * 3
    # the last message ends on the buffer's last byte: no pad bytes behind it, at a start that is not aligned
    lengths = [3, rate + 5]
    assert sum(lengths) % 8 == 0
    messages = messages_of(lengths, 47)
    msg, off = ntt.ragged_pack(messages, dev)
    assert msg.numel() == sum(lengths) and int(off[-1]) == msg.numel()
    check_ragged(ntt, dev, algo, messages)
    check_ragged(ntt, dev, algo, messages_of([5, 0, 2 * rate + 3 - 8], 48))   # ... with an idle second half beside it


@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("algo", ALGOS)
def test_auto_on_both_sides_of_the_switch(ntt, dev, algo, ragged):
    rate = K.RATE[algo]
    m = ntt.xof_small_batch_max(algo, ragged=ragged)
    for batch in ([min(m, 64)] if m > 0 else []) + [m + 1]:
        if ragged:
            lengths = np.random.default_rng([49, batch]).integers(0, rate + 9, batch).tolist()
            check_ragged(ntt, dev, algo, messages_of(lengths, 49), path="auto")
        else:
            run_xof(ntt, dev, algo, batch, 8, rate, 32, path="auto")


@pytest.mark.parametrize("ragged", (False, True))
def test_batch_past_2_27(ntt, dev, ragged):
    """2^27 + 3 empty messages, 8 bytes out (1 GiB of output): more than 2^26 waves and 2^32 threads, so a wave index
    made from a 32-bit thread index wraps and a single row of workgroups is cut short by the launch; either leaves
    digests unwritten.  Every digest is SHAKE256("")'s first 8 bytes; the last wave has an idle half."""
    batch, outlen = (1 << 27) + 3, 8
    buf, out = guarded(dev, batch, outlen)
    if ragged:
        msg = torch.empty(0, dtype=torch.uint8, device=dev)
        off = torch.zeros(batch + 1, dtype=torch.int64, device=dev)
        ntt.xof_ragged(out, msg, off, algo="shake256", path="wave")
    else:
        empty = torch.empty((batch, 0), dtype=torch.uint8, device=dev)
        ntt.xof(out, empty, None, algo="shake256", path="wave")
    want = int.from_bytes(hashlib.shake_256(b"").digest(outlen), "little", signed=True)
    words = out.view(torch.int64).view(-1)
    wrong = (words != want).nonzero()
    assert wrong.numel() == 0, f"{wrong.numel()} digests differ, the first at message {int(wrong[0])}"
    assert guards_intact(buf, batch, outlen), "store outside the output"
