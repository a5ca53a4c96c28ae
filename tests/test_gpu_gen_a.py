"""poly_gen_a on the GPU, bit-exact against gen_a_model.gen_a for the fixed
seeds: refill-dominated keys whose lanes finish in different refills, an odd
first call, a first call that must stop at k n, 0 / 1 / 2 refills within one
wave, qTESLA's own shapes, n = 4096 / 8192 (the customisation crossing 255),
k = 8, strided outputs, seed lengths up to the absorb block, a non-default
stream.  The output starts as a sentinel between guard words: every word of a
polynomial is rewritten, the gaps, the guards and the seeds are not."""
import functools

import numpy as np
import pytest
import torch

import gen_a_model as M
import keccak_model as K

pytestmark = pytest.mark.gpu

GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
SENTINEL = 0xFFFFFFFF

# one squeeze per (hash, seed, length, customisation) for the whole module
K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


@functools.lru_cache(maxsize=None)
def model(n, q, k, nblocks, idx, seedlen=32):
    """(a as uint32 [k, n], refills) of fixed seed idx"""
    st = {}
    a = M.gen_a(K.seeds(idx + 1, seedlen)[idx], k, n, q, nblocks, st)
    return np.array(a, dtype=np.uint32), st["refills"]


def run(ntt, dev, ps, k, nblocks, idxs, pstride=None, seedlen=32, stream=None):
    """the strided output as uint32 [batch, k, pstride]; checks the guards and the seeds.  Lane b gets seed idxs[b]."""
    n = ntt.param_info(ps)["n"]
    batch, pstride = len(idxs), n if pstride is None else pstride
    all_seeds = K.seeds(max(idxs) + 1, seedlen)
    sd = np.frombuffer(b"".join(all_seeds[i] for i in idxs), dtype=np.uint8).reshape(batch, seedlen)
    ts = torch.from_numpy(sd.copy()).to(dev)
    buf = torch.full((batch * k * pstride + 32,), GUARD, dtype=torch.int32, device=dev)
    a = buf[16:-16]
    a.fill_(-1)
    kw = {} if pstride == n else {"pstride": pstride}
    assert ntt.poly_gen_a(a, ts, ps, nblocks, k, stream=stream, **kw) is a
    if stream is not None:
        stream.synchronize()
    assert bool((buf[:16] == GUARD).all()) and bool((buf[-16:] == GUARD).all()), "store outside a"
    assert np.array_equal(ts.cpu().numpy(), sd), "seeds changed"
    return ntt.to_numpy_u32(a).reshape(batch, k, pstride)


def check(ntt, dev, ps, k, nblocks, idxs, **kw):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    idxs = list(idxs)
    got = run(ntt, dev, ps, k, nblocks, idxs, **kw)
    want = np.stack([model(n, q, k, nblocks, i, kw.get("seedlen", 32))[0] for i in idxs])
    bad = np.argwhere(got[:, :, :n] != want)
    assert bad.size == 0, f"{ps} k {k} nblocks {nblocks}: first mismatch at (key, polynomial, coefficient) {bad[0].tolist()}"
    assert int(got[:, :, :n].max()) < q                      # in particular no word kept its sentinel
    assert bool((got[:, :, n:] == SENTINEL).all()), "a gap between polynomials was written"
    return [model(n, q, k, nblocks, i, kw.get("seedlen", 32))[1] for i in idxs]


def test_refill_dominated(ntt, dev):
    """nblocks 1: one full wave and a 3-lane tail, lanes finishing in different refills"""
    refills = check(ntt, dev, "p-I", 1, 1, range(67))
    assert min(refills) == 37 and max(refills) == 41


@pytest.mark.parametrize("batch", (1, 63, 64, 65))
def test_batches(ntt, dev, batch):
    check(ntt, dev, "p-I", 1, 1, range(batch))


def test_odd_first_call(ntt, dev):
    """35 blocks: the last two words of the first call are not drawn; a polynomial boundary in mid-stream"""
    refills = check(ntt, dev, "p-I", 2, 35, range(5))
    assert 41 <= min(refills) and max(refills) <= 45


def test_first_call_stops_at_kn(ntt, dev):
    refills = check(ntt, dev, "p-III", 1, 70, range(16))
    assert refills == [0] * 16


def test_0_1_2_refills_in_one_wave(ntt, dev):
    refills = check(ntt, dev, "p-III", 1, 61, range(16))
    assert set(refills) == {0, 1, 2}


@pytest.mark.parametrize("ps,k,nblocks", (("p-I", 4, 108), ("p-III", 5, 180)))
def test_qtesla_shapes(ntt, dev, ps, k, nblocks):
    refills = check(ntt, dev, ps, k, nblocks, range(3))
    assert refills == {"p-I": [48, 48, 48], "p-III": [134, 133, 132]}[ps]


def test_customisation_crosses_255(ntt, dev):
    refills = check(ntt, dev, "p-III-8192", 1, 2, range(2))
    assert sorted(refills) == [255, 256]


def test_n_4096(ntt, dev):
    check(ntt, dev, "p-III-4096", 1, 1, range(2))


def test_k_8(ntt, dev):
    refills = check(ntt, dev, "p-I", 8, 1, range(2))
    assert 321 in refills and max(refills) < M.refills_max(8, 1024) == 820


@pytest.mark.parametrize("ps,k,nblocks", (("p-I", 2, 35), ("p-III", 1, 61)))
def test_strides(ntt, dev, ps, k, nblocks):
    n = ntt.param_info(ps)["n"]
    for pstride in (2 * n, n + 4):
        check(ntt, dev, ps, k, nblocks, range(5), pstride=pstride)


@pytest.mark.parametrize("seedlen", (8, 160))
def test_seed_lengths(ntt, dev, seedlen):
    """one lane of seed, and the longest: all but the last lane of the absorb block; the refills absorb it again"""
    check(ntt, dev, "p-I", 1, 1, range(3), seedlen=seedlen)


def test_non_default_stream(ntt, dev):
    torch.cuda.synchronize(dev)
    check(ntt, dev, "p-I", 1, 1, range(65), stream=torch.cuda.Stream(device=dev))


def test_batch_independence(ntt, dev):
    """the same seed at lanes 0 and 66 (another wave, its tail) gives the same row"""
    idxs = [5] + list(range(1, 66)) + [5]
    got = run(ntt, dev, "p-I", 1, 1, idxs)
    assert np.array_equal(got[0], got[66])
    check(ntt, dev, "p-I", 1, 1, idxs)


def test_wrapper_rejects_before_the_call(ntt, dev):
    n = 1024
    a = torch.zeros(3 * 4 * n, dtype=torch.int32, device=dev)
    seed = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    for nblocks in (0, 257):
        with pytest.raises(ValueError):
            ntt.poly_gen_a(a, seed, "p-I", nblocks, 4)
    for k in (0, 9, 3):          # 3: a.numel() is not batch * k * pstride
        with pytest.raises(ValueError):
            ntt.poly_gen_a(a, seed, "p-I", 108, k)
    for pstride in (n - 4, n + 2, 2 * n):   # 2 n: a is too small
        with pytest.raises(ValueError):
            ntt.poly_gen_a(a, seed, "p-I", 108, 4, pstride=pstride)
    with pytest.raises(ValueError):
        ntt.poly_gen_a(a, seed[:, :12].contiguous(), "p-I", 108, 4)
    with pytest.raises(ValueError):
        ntt.poly_gen_a(a, seed[:2].contiguous(), "p-I", 108, 4)
    with pytest.raises(ValueError):
        ntt.poly_gen_a(a, seed.view(-1), "p-I", 108, 4)
    with pytest.raises(TypeError):
        ntt.poly_gen_a(a.to(torch.uint8), seed, "p-I", 108, 4)
    with pytest.raises(TypeError):
        ntt.poly_gen_a(a, seed.to(torch.int32), "p-I", 108, 4)
    with pytest.raises(KeyError):
        ntt.poly_gen_a(a, seed, "p-IX", 108, 4)
    with pytest.raises(ntt.NTTError):
        ntt.poly_gen_a(a, seed, "ref", 108, 4)   # n = 1024 as p-I, a 24-bit prime: the library's NTT_ERR_PARAM
