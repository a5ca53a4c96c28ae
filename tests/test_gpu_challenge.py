"""poly_challenge on the GPU, exact against the model's enc: all five
parameter sets, batches round the wave, h from one entry to three squeeze
blocks (h = 57: a second block for every seed; h = 128: a third),
guard words round both outputs over garbage, the seeds unchanged, and the
lists fed to poly_scatter giving the model's dense c."""
import functools

import numpy as np
import pytest
import torch

from conftest import LARGE_SETS, PARAM_SETS

import keccak_model as K

pytestmark = pytest.mark.gpu

GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
GARBAGE = int(np.uint32(0xDEADBEEF).view(np.int32))
HS = (1, 25, 40, 57, 128)
NSEEDS = 257

# enc squeezes the same blocks for every parameter set (n and q only enter the draws):
# the blocks of a seed are computed once for the whole module, enc itself runs as written
K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


@functools.lru_cache(maxsize=None)
def model(n, q, seedlen=32):
    """enc of the fixed seeds at the largest h; a smaller h is its prefix (test_xof_model)"""
    out, stats = [], []
    for s in K.seeds(NSEEDS, seedlen):
        st = {}
        out.append(K.enc(s, n, q, max(HS), st))
        stats.append(st)
    return out, stats


def run(ntt, dev, ps, seeds, h, stream=None):
    """(pos, val) as uint32 [batch, h]; checks the guards and the seeds"""
    batch = len(seeds)
    sd = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(batch, -1)
    ts = torch.from_numpy(sd.copy()).to(dev)
    bufs = [torch.full((batch * h + 32,), GUARD, dtype=torch.int32, device=dev) for _ in range(2)]
    pos, val = (b[16:-16].view(batch, h) for b in bufs)
    pos.fill_(GARBAGE)
    val.fill_(GARBAGE)
    ntt.poly_challenge(pos, val, ts, ps, stream=stream)
    if stream is not None:
        stream.synchronize()
    for b in bufs:
        assert bool((b[:16] == GUARD).all()) and bool((b[-16:] == GUARD).all()), "store outside an output buffer"
    assert np.array_equal(ts.cpu().numpy(), sd), "seeds changed"
    return pos, val


@pytest.mark.parametrize("batch", (1, 65, 257))
@pytest.mark.parametrize("ps", PARAM_SETS + LARGE_SETS)
def test_challenge_exact(ntt, dev, ps, batch):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    want, stats = model(n, q)
    seeds = K.seeds(NSEEDS)[:batch]
    # what the cases are for, on the model: a rejected collision within the first 40 draws of
    # some seed of the larger batches, and second / third blocks at h = 57 / 128
    assert all(st["blocks"] >= 3 for st in stats[:batch])
    if batch >= 65 and n <= 2048:
        assert any(len(set(_raw_positions(s, n, 40))) < 40 for s in seeds)
    for h in HS:
        pos, val = run(ntt, dev, ps, seeds, h)
        gp, gv = ntt.to_numpy_u32(pos), ntt.to_numpy_u32(val)
        wp = np.array([want[b][0][:h] for b in range(batch)], dtype=np.uint32)
        wv = np.array([want[b][1][:h] for b in range(batch)], dtype=np.uint32)
        assert np.array_equal(gp, wp), f"{ps} batch {batch} h {h}: positions"
        assert np.array_equal(gv, wv), f"{ps} batch {batch} h {h}: values"
        # the lists are poly_scatter's input as they are
        c = torch.full((batch, n), GARBAGE, dtype=torch.int32, device=dev)
        ntt.poly_scatter(c, pos, val, ps)
        dense = np.zeros((batch, n), dtype=np.uint32)
        for b in range(batch):
            dense[b, wp[b]] = wv[b]
        assert np.array_equal(ntt.to_numpy_u32(c), dense), f"{ps} batch {batch} h {h}: dense c"


def _raw_positions(seed, n, draws):
    r = K.cshake_simple("shake128", seed, 168, 0)
    return [((r[3 * j] << 8) | r[3 * j + 1]) & (n - 1) for j in range(draws)]


@pytest.mark.parametrize("seedlen", (8, 64, 160))
def test_challenge_seed_lengths(ntt, dev, seedlen):
    """one lane of seed, qTESLA-III's 64 bytes, and the longest: 20 of the block's 21 lanes"""
    ps, batch, h = "p-I", 3, 57
    info = ntt.param_info(ps)
    seeds = K.seeds(batch, seedlen)
    pos, val = run(ntt, dev, ps, seeds, h)
    for b in range(batch):
        wp, wv = K.enc(seeds[b], info["n"], info["q"], h)
        assert ntt.to_numpy_u32(pos)[b].tolist() == wp and ntt.to_numpy_u32(val)[b].tolist() == wv, (seedlen, b)


def test_challenge_non_default_stream(ntt, dev):
    ps, batch, h = "p-III", 65, 40
    info = ntt.param_info(ps)
    want, _ = model(info["n"], info["q"])
    torch.cuda.synchronize(dev)
    pos, val = run(ntt, dev, ps, K.seeds(NSEEDS)[:batch], h, stream=torch.cuda.Stream(device=dev))
    assert ntt.to_numpy_u32(pos).tolist() == [want[b][0][:h] for b in range(batch)]
    assert ntt.to_numpy_u32(val).tolist() == [want[b][1][:h] for b in range(batch)]


def test_wrapper_rejects_before_the_call(ntt, dev):
    pos = torch.zeros((3, 40), dtype=torch.int32, device=dev)
    val = torch.zeros_like(pos)
    seed = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        ntt.poly_challenge(pos, val[:, :39].contiguous(), seed, "p-III")
    with pytest.raises(ValueError):
        ntt.poly_challenge(pos.view(-1), val.view(-1), seed, "p-III")
    with pytest.raises(ValueError):
        ntt.poly_challenge(pos, val, seed[:2].contiguous(), "p-III")
    with pytest.raises(ValueError):
        ntt.poly_challenge(pos, val, seed[:, :12].contiguous(), "p-III")
    with pytest.raises(TypeError):
        ntt.poly_challenge(pos, val, seed.to(torch.int32), "p-III")
    with pytest.raises(TypeError):
        ntt.poly_challenge(pos.to(torch.uint8), val, seed, "p-III")
    big = torch.zeros((3, 129), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ntt.poly_challenge(big, torch.zeros_like(big), seed, "p-III")
    with pytest.raises(KeyError):
        ntt.poly_challenge(pos, val, seed, "p-IX")
