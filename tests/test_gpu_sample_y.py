"""poly_sample_y on the GPU, bit-exact against sample_model.sample_y for the
fixed seeds: qTESLA's shapes and the crossed ones (the stream ends at another
phase of the rate), n = 4096 / 8192, bits = 2 (every block rejects, every seed
refills several times), bits = 14 at batch 70 (tile blocks, rejecting blocks
and unequal per-lane offsets within one wave, a 6-lane tail wave), batches
round the wave, nonces as scalar, tensor and both, seed lengths up to the
absorb block, a non-default stream.  The output starts as 0xFFFFFFFF between
guard words: every word is rewritten, the guards and the seeds are not."""
import functools

import numpy as np
import pytest
import torch

import keccak_model as K
import sample_model as M

pytestmark = pytest.mark.gpu

GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
NSEEDS = 257

# one squeeze per (hash, seed, length, customisation) for the whole module: bits only masks it
K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


@functools.lru_cache(maxsize=None)
def model(n, q, bits, algo, nonce, idx, seedlen=32):
    """(y as uint32 [n], stats) of fixed seed idx"""
    st = {}
    y = M.sample_y(K.seeds(idx + 1, seedlen)[idx], n, q, bits, algo, nonce, st)
    return np.array(y, dtype=np.uint32), st


def want(info, bits, algo, nonces, seedlen=32):
    return np.stack([model(info["n"], info["q"], bits, algo, nc, b, seedlen)[0] for b, nc in enumerate(nonces)])


def run(ntt, dev, ps, batch, bits, algo, nonce=0, nonces=None, seedlen=32, stream=None):
    """y as uint32 [batch, n]; checks the guards and the seeds"""
    n = ntt.param_info(ps)["n"]
    sd = np.frombuffer(b"".join(K.seeds(batch, seedlen)), dtype=np.uint8).reshape(batch, seedlen)
    ts = torch.from_numpy(sd.copy()).to(dev)
    buf = torch.full((batch * n + 32,), GUARD, dtype=torch.int32, device=dev)
    y = buf[16:-16].view(batch, n)
    y.fill_(-1)
    tn = None if nonces is None else torch.tensor(nonces, dtype=torch.int32, device=dev)
    assert ntt.poly_sample_y(y, ts, ps, bits, algo=algo, nonce=nonce, nonces=tn, stream=stream) is y
    if stream is not None:
        stream.synchronize()
    assert bool((buf[:16] == GUARD).all()) and bool((buf[-16:] == GUARD).all()), "store outside y"
    assert np.array_equal(ts.cpu().numpy(), sd), "seeds changed"
    if tn is not None:
        assert tn.cpu().tolist() == list(nonces), "nonces changed"
    return ntt.to_numpy_u32(y).reshape(batch, n)


def check(ntt, dev, ps, batch, bits, algo, **kw):
    info = ntt.param_info(ps)
    got = run(ntt, dev, ps, batch, bits, algo, **kw)
    nonces = [((kw.get("nonces") or [0] * batch)[b] + kw.get("nonce", 0)) & 0xFF for b in range(batch)]
    w = want(info, bits, algo, nonces, kw.get("seedlen", 32))
    bad = np.argwhere(got != w)
    assert bad.size == 0, f"{ps} {algo} bits {bits} batch {batch}: first mismatch at (row, coefficient) {bad[0].tolist()}"
    assert int(got.max()) < info["q"]   # in particular no word kept its 0xFFFFFFFF


@pytest.mark.parametrize("ps,algo,bits", (("p-I", "shake128", 20), ("p-III", "shake256", 22), ("ref", "shake128", 22),
                                          ("p-I", "shake256", 20), ("p-III", "shake128", 22)))
def test_qtesla_and_crossed_shapes(ntt, dev, ps, algo, bits):
    """3 n bytes end 48 bytes into block 19 (1024, rate 168), 96 bytes into block 37 (2048, 168), mid-period at
    rate 136 for 1024 (block 23 = phase 1) and 8 draws into a period for 2048 (block 46 = phase 0)"""
    check(ntt, dev, ps, 65, bits, algo)


@pytest.mark.parametrize("ps", ("p-III-4096", "p-III-8192"))
@pytest.mark.parametrize("algo", ("shake128", "shake256"))
def test_large_n(ntt, dev, ps, algo):
    check(ntt, dev, ps, 3, 22, algo)


@pytest.mark.parametrize("ps,algo,batch", (("p-I", "shake128", 65), ("p-III", "shake256", 65)))
def test_bits_2_every_block_rejects(ntt, dev, ps, algo, batch):
    info = ntt.param_info(ps)
    stats = [model(info["n"], info["q"], 2, algo, 0, b)[1] for b in range(batch)]
    assert all(st["refills"] >= 2 and st["rejected"] > info["n"] // 8 for st in stats)
    check(ntt, dev, ps, batch, 2, algo)


@pytest.mark.parametrize("ps,algo,hit", (("p-I", "shake128", (19, 29, 44, 69)), ("p-III", "shake256", (8, 14, 27, 35, 54, 64, 65))))
def test_bits_14_both_paths_in_one_wave(ntt, dev, ps, algo, hit):
    info = ntt.param_info(ps)
    batch = 70
    stats = [model(info["n"], info["q"], 14, algo, 0, b)[1] for b in range(batch)]
    rejecting = [b for b, st in enumerate(stats) if st["rejected"]]
    assert rejecting == list(hit) and all(stats[b] == {"rejected": 1, "refills": 1} for b in hit)
    assert any(b < 64 for b in rejecting) and any(b >= 64 for b in rejecting)   # both waves
    check(ntt, dev, ps, batch, 14, algo)


@pytest.mark.parametrize("batch", (1, 63, 64, 65, 257))
def test_batches(ntt, dev, batch):
    check(ntt, dev, "p-I", batch, 20, "shake128")


def test_nonces(ntt, dev):
    ps, algo, bits = "p-I", "shake128", 20
    for nonce in (0, 1, 255):
        check(ntt, dev, ps, 5, bits, algo, nonce=nonce)
    tensor = [0, 1, 255, 3, 7]
    check(ntt, dev, ps, 5, bits, algo, nonces=tensor)       # row by row the scalar calls' model
    check(ntt, dev, ps, 5, bits, algo, nonces=tensor, nonce=2)   # 255 + 2 wraps to 1
    check(ntt, dev, ps, 5, bits, algo, nonces=[255] * 5, nonce=255)
    a = run(ntt, dev, ps, 5, bits, algo, nonces=tensor)
    for b, nonce in enumerate(tensor):
        assert np.array_equal(run(ntt, dev, ps, 5, bits, algo, nonce=nonce)[b], a[b]), (b, nonce)
    # p-III at rate 136, a different nonce in every lane of a wave and a tail
    check(ntt, dev, "p-III", 66, 14, "shake256", nonces=[(5 * b) % 4 for b in range(66)])


@pytest.mark.parametrize("algo,seedlen", (("shake128", 8), ("shake128", 160), ("shake256", 8), ("shake256", 128), ("shake256", 64)))
def test_seed_lengths(ntt, dev, algo, seedlen):
    """one lane of seed, qTESLA-III's 64 bytes, and the longest: all but the last lane of the absorb block"""
    check(ntt, dev, "p-I", 3, 20, algo, seedlen=seedlen)
    check(ntt, dev, "p-I", 3, 2, algo, seedlen=seedlen)     # the refills absorb the seed again


def test_non_default_stream(ntt, dev):
    torch.cuda.synchronize(dev)
    check(ntt, dev, "p-III", 65, 22, "shake256", stream=torch.cuda.Stream(device=dev))


def test_wrapper_rejects_before_the_call(ntt, dev):
    y = torch.zeros((3, 2048), dtype=torch.int32, device=dev)
    seed = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    nonces = torch.zeros(3, dtype=torch.int32, device=dev)
    for bits in (1, 25):
        with pytest.raises(ValueError):
            ntt.poly_sample_y(y, seed, "p-III", bits)
    for nonce in (-1, 256):
        with pytest.raises(ValueError):
            ntt.poly_sample_y(y, seed, "p-III", 22, nonce=nonce)
    with pytest.raises(ValueError):
        ntt.poly_sample_y(y, seed, "p-III", 22, algo="sha3")
    with pytest.raises(ValueError):
        ntt.poly_sample_y(y, seed[:2].contiguous(), "p-III", 22)
    with pytest.raises(ValueError):
        ntt.poly_sample_y(y, seed[:, :12].contiguous(), "p-III", 22)
    with pytest.raises(ValueError):
        ntt.poly_sample_y(y, torch.zeros((3, 136), dtype=torch.uint8, device=dev), "p-III", 22, algo="shake256")
    with pytest.raises(ValueError):
        ntt.poly_sample_y(y, seed, "p-III", 22, nonces=nonces[:2].contiguous())
    with pytest.raises(TypeError):
        ntt.poly_sample_y(y, seed, "p-III", 22, nonces=nonces.to(torch.uint8))
    with pytest.raises(TypeError):
        ntt.poly_sample_y(y.to(torch.uint8), seed, "p-III", 22)
    with pytest.raises(KeyError):
        ntt.poly_sample_y(y, seed, "p-IX", 22)
