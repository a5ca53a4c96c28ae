"""ntt_xof_ragged on the GPU, exact: SHAKE against hashlib, cshake*_simple
against the plain-Python model (messages of at most 2 rate + 1 bytes: it costs
about 1 ms a permutation).  Message lengths round every edge of a word and of
the rate, mixed in one wave; every start alignment; neighbours and pad bytes
that must not leak into a digest; output lengths round the rate between guard
words; batches round the wave and the workgroup; equality with ntt_xof where
both are defined; the clamping of the offsets; an empty buffer."""
import hashlib

import numpy as np
import pytest
import torch

import keccak_model as K

pytestmark = pytest.mark.gpu

ALGOS = ("shake128", "shake256")
HASHLIB = {"shake128": hashlib.shake_128, "shake256": hashlib.shake_256}
GUARD = 64   # bytes either side of the output


def edge_lengths(rate):
    return [0, 1, 7, 8, 9, 63, rate - 9, rate - 8, rate - 1, rate, rate + 1, rate + 7, rate + 8, 2 * rate - 1, 2 * rate,
            2 * rate + 1, 3 * rate + 5]


def reference(algo, m, outlen, cstm=None):
    return HASHLIB[algo](m).digest(outlen) if cstm is None else K.cshake_simple(algo, m, outlen, cstm)


def messages_of(lengths, seed):
    rng = np.random.default_rng([seed, len(lengths)])
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


def run(ntt, dev, algo, msg, off, outlen, cstm=None, stream=None):
    """one launch into an output between guards over garbage; returns the digests as a list of bytes"""
    batch = off.numel() - 1
    buf = torch.full((batch * outlen + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[GUARD:GUARD + batch * outlen].view(batch, outlen)
    out.fill_(0xDB)
    if stream is not None:
        torch.cuda.synchronize(dev)
    assert ntt.xof_ragged(out, msg, off, algo=algo, cstm=cstm, stream=stream) is out
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + batch * outlen:] == 0xA5).all()), "store outside the output"
    return [got[b].tobytes() for b in range(batch)]


def check(ntt, dev, algo, messages, outlen, cstm=None, stream=None):
    """pack, hash, compare every digest; the inputs must come back unchanged"""
    msg, off = ntt.ragged_pack(messages, dev)
    msg0, off0 = msg.clone(), off.clone()
    got = run(ntt, dev, algo, msg, off, outlen, cstm, stream)
    for b, m in enumerate(messages):
        assert got[b] == reference(algo, m, outlen, cstm), f"{algo} cstm {cstm} out {outlen}: message {b} of {len(m)} bytes"
    assert torch.equal(msg, msg0) and torch.equal(off, off0), "input changed"
    return off0.cpu().numpy()


def mixed_order(rate):
    """the edge lengths, then shuffled copies of them up to 65 messages, in the first order whose starts cover every
    value of begin & 7 (a condition on the input alone)"""
    base = edge_lengths(rate)
    for seed in range(64):
        rng = np.random.default_rng([rate, seed])
        order = list(base)
        while len(order) < 65:
            order += [base[i] for i in rng.permutation(len(base))]
        order = order[:65]
        starts = np.concatenate([[0], np.cumsum(order)[:-1]])
        if set(int(s) & 7 for s in starts) == set(range(8)):
            return order
    raise AssertionError("no order covers every start alignment")


@pytest.mark.parametrize("algo", ALGOS)
def test_lengths_round_every_edge(ntt, dev, algo):
    """one full wave of mixed lengths plus one lane of the next"""
    rate = K.RATE[algo]
    order = mixed_order(rate)
    assert len(order) == 65 and set(order) == set(edge_lengths(rate))
    off = check(ntt, dev, algo, messages_of(order, 1), 32)
    assert set(int(o) & 7 for o in off[:-1]) == set(range(8))


@pytest.mark.parametrize("algo", ALGOS)
def test_every_alignment(ntt, dev, algo):
    """the same L bytes at begin = a (mod 8) for every a, behind filler messages"""
    rate = K.RATE[algo]
    data = messages_of([rate + 1], 2)[0]
    filler = messages_of([16], 3)[0]
    messages, placed, pos = [], [], 0
    for a in range(8):
        for L in (0, 1, 8 - a, rate - 1, rate, rate + 1):
            f = (a - pos) % 8 + 8 * (len(placed) % 2)   # fillers of 0 .. 15 bytes, empty ones among them
            messages += [filler[:f], data[:L]]
            pos += f
            assert pos % 8 == a
            placed.append((len(messages) - 1, a, L))
            pos += L
    off = check(ntt, dev, algo, messages, 32)
    assert all(off[b] % 8 == a and off[b + 1] - off[b] == L for b, a, L in placed)
    assert sorted({a for _, a, _ in placed}) == list(range(8))


@pytest.mark.parametrize("algo", ALGOS)
def test_neighbours_and_padding_do_not_leak(ntt, dev, algo):
    rate = K.RATE[algo]
    lengths = [5, 0, rate - 1, 1, rate + 3, 8, 2 * rate + 1, 7, 3]   # 2 mod 8 bytes of padding at the end
    messages = messages_of(lengths, 4)
    msg, off = ntt.ragged_pack(messages, dev)
    assert msg.numel() > sum(lengths)
    first = run(ntt, dev, algo, msg, off, 32)
    offs = off.cpu().numpy()
    other = torch.from_numpy(np.random.default_rng(5).integers(0, 256, msg.numel(), dtype=np.uint8)).to(dev)
    inside = torch.arange(msg.numel(), device=dev)
    for b in range(len(messages)):
        mine = (inside >= int(offs[b])) & (inside < int(offs[b + 1]))
        changed = torch.where(mine, msg, other ^ (other == msg).to(torch.uint8))   # every other byte differs, pad bytes included
        assert bool((changed != msg)[~mine].all()) and torch.equal(changed[mine], msg[mine])
        before, off_before = changed.clone(), off.clone()
        again = run(ntt, dev, algo, changed, off, 32)
        assert again[b] == first[b] == reference(algo, messages[b], 32), f"{algo}: message {b} depends on bytes that are not its own"
        assert torch.equal(changed, before) and torch.equal(off, off_before), "input changed"


@pytest.mark.parametrize("algo", ALGOS)
def test_output_lengths(ntt, dev, algo):
    rate = K.RATE[algo]
    order = mixed_order(rate)[:63]
    for outlen in (8, 32, rate, rate + 8, 512):
        check(ntt, dev, algo, messages_of(order, 6), outlen)


@pytest.mark.parametrize("batch", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("algo", ALGOS)
def test_batches(ntt, dev, algo, batch):
    rate = K.RATE[algo]
    rng = np.random.default_rng([7, batch])
    lengths = rng.integers(0, 2 * rate + 9, batch).tolist()
    lengths[-1] = rate + 3   # the last lane absorbs a whole block and an odd tail
    check(ntt, dev, algo, messages_of(lengths, 7), 32)


def test_non_default_stream(ntt, dev):
    s = torch.cuda.Stream(device=dev)
    check(ntt, dev, "shake256", messages_of(mixed_order(136), 8), 32, stream=s)
    check(ntt, dev, "shake128", messages_of(edge_lengths(168)[:12], 8), 32, cstm=7, stream=s)


@pytest.mark.parametrize("cstm", (0, 0x0103, 65535))
@pytest.mark.parametrize("algo", ALGOS)
def test_cshake_simple(ntt, dev, algo, cstm):
    rate = K.RATE[algo]
    lengths = [n for n in edge_lengths(rate) if n <= 2 * rate + 1]
    lengths = [lengths[i] for i in (0, 1, 2, 4, 6, 7, 8, 9, 10, 12, 13, 15)]   # 0 1 7 9 r-9 r-8 r-1 r r+1 r+8 2r-1 2r+1
    assert len(lengths) == 12 and max(lengths) == 2 * rate + 1
    check(ntt, dev, algo, messages_of(lengths, 9), 32, cstm=cstm)


@pytest.mark.parametrize("cstm", (None, 0x1234))
@pytest.mark.parametrize("algo", ALGOS)
def test_equal_to_xof_where_both_are_defined(ntt, dev, algo, cstm):
    rate = K.RATE[algo]
    batch, n = 65, rate + 8
    msg = torch.from_numpy(np.random.default_rng(10).integers(0, 256, batch * n, dtype=np.uint8)).to(dev)
    off = (torch.arange(batch + 1, dtype=torch.int64) * n).to(dev)
    want = torch.empty((batch, 32), dtype=torch.uint8, device=dev)
    ntt.xof(want, msg.view(batch, -1), algo=algo, cstm=cstm)
    got = torch.empty_like(want)
    ntt.xof_ragged(got, msg, off, algo=algo, cstm=cstm)
    assert torch.equal(got, want)
    assert got[64].cpu().numpy().tobytes() == reference(algo, msg[64 * n:].cpu().numpy().tobytes(), 32, cstm)


@pytest.mark.parametrize("algo", ALGOS)
def test_clamping_is_the_definition(ntt, dev, algo):
    """a decreasing pair, a pair past the end and a pair straddling it, all inside a 2 M byte allocation whose second
    half holds other bytes: a kernel that failed to clamp gives a wrong digest and nothing worse"""
    M = 512
    whole = torch.from_numpy(np.random.default_rng(11).integers(0, 256, 2 * M, dtype=np.uint8)).to(dev)
    msg = whole[:M]
    assert msg.is_contiguous() and msg.data_ptr() == whole.data_ptr()
    offsets = [0, 40, 24, 100, M + 16, M + 8, 2 * M - 8]
    off = torch.tensor(offsets, dtype=torch.int64, device=dev)
    host = whole.cpu().numpy().tobytes()[:M]
    spans = []
    for b in range(len(offsets) - 1):
        begin = min(offsets[b], M)
        end = min(max(offsets[b + 1], begin), M)
        spans.append((begin, end))
    assert spans == [(0, 40), (40, 40), (24, 100), (100, M), (M, M), (M, M)]
    got = run(ntt, dev, algo, msg, off, 32)
    for b, (begin, end) in enumerate(spans):
        assert got[b] == reference(algo, host[begin:end], 32), f"{algo}: message {b} = [{begin}, {end})"


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_buffer(ntt, dev, algo):
    msg = torch.empty(0, dtype=torch.uint8, device=dev)
    off = torch.zeros(4, dtype=torch.int64, device=dev)
    assert run(ntt, dev, algo, msg, off, 32) == [reference(algo, b"", 32)] * 3
    assert run(ntt, dev, algo, msg, off, 32, cstm=5) == [reference(algo, b"", 32, 5)] * 3
