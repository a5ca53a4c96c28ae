"""poly_sample_gauss on the GPU, bit-exact against gauss_model.sample_gauss for
the fixed seeds: qTESLA's pairings of hash and table width and the crossed
ones (samples straddle blocks at another period), one and three limbs at both
rates, n = 4096 / 8192, batches round the wave counted in chunks, nonces as
scalar, tensor and both, seed lengths up to the absorb block, a non-default
stream, and tables made to sit on the comparator's edges.  The output starts
as 0xFFFFFFFF between guard words: every word is rewritten, the guards, the
seeds, the nonces and the table are not."""
import functools

import numpy as np
import pytest
import torch

import gauss_model as G
import keccak_model as K

pytestmark = pytest.mark.gpu

GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
SIGMA = 8.5
TABLES = {1: 30, 2: 77, 3: 90, 4: 110}   # rows of the sigma = 8.5 table at each width (the last that is still increasing, or fewer)

# one squeeze per (hash, seed, length, customisation) for the whole module
K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


def table_for(cols):
    return tuple(tuple(row) for row in G.cdt_table(SIGMA, TABLES[cols], cols))


@functools.lru_cache(maxsize=None)
def model(n, q, table, algo, nonce, idx, seedlen=32):
    """the polynomial of fixed seed idx as uint32 [n]; table is a tuple of row tuples"""
    seed = K.seeds(idx + 1, seedlen)[idx]
    return np.array(G.sample_gauss(seed, n, q, [list(r) for r in table], len(table[0]), algo, nonce), dtype=np.uint32)


def run(ntt, dev, ps, batch, table, algo, nonce=0, nonces=None, seedlen=32, stream=None):
    """out as uint32 [batch, n]; checks the guards, the seeds, the nonces and the table"""
    n = ntt.param_info(ps)["n"]
    sd = np.frombuffer(b"".join(K.seeds(batch, seedlen)), dtype=np.uint8).reshape(batch, seedlen)
    ts = torch.from_numpy(sd.copy()).to(dev)
    tab = np.array(table, dtype=np.uint32)
    tt = ntt.from_numpy_u32(tab, dev)
    buf = torch.full((batch * n + 32,), GUARD, dtype=torch.int32, device=dev)
    out = buf[16:-16].view(batch, n)
    out.fill_(-1)
    tn = None if nonces is None else torch.tensor(nonces, dtype=torch.int32, device=dev)
    assert ntt.poly_sample_gauss(out, ts, tt, ps, algo=algo, nonce=nonce, nonces=tn, stream=stream) is out
    if stream is not None:
        stream.synchronize()
    assert bool((buf[:16] == GUARD).all()) and bool((buf[-16:] == GUARD).all()), "store outside out"
    assert np.array_equal(ts.cpu().numpy(), sd), "seeds changed"
    assert np.array_equal(ntt.to_numpy_u32(tt), tab), "table changed"
    if tn is not None:
        assert tn.cpu().tolist() == list(nonces), "nonces changed"
    return ntt.to_numpy_u32(out).reshape(batch, n)


def check(ntt, dev, ps, batch, table, algo, **kw):
    info = ntt.param_info(ps)
    got = run(ntt, dev, ps, batch, table, algo, **kw)
    nonces = [((kw.get("nonces") or [0] * batch)[b] + kw.get("nonce", 0)) & 0xFF for b in range(batch)]
    masked = tuple(tuple(int(w) & G.LIMB for w in row) for row in table)
    want = np.stack([model(info["n"], info["q"], masked, algo, nc, b, kw.get("seedlen", 32)) for b, nc in enumerate(nonces)])
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{ps} {algo} cols {len(table[0])} batch {batch}: first mismatch at (row, coefficient) {bad[0].tolist()}"
    assert int(got.max()) < info["q"]   # in particular no word kept its 0xFFFFFFFF, and -0 is not q
    return got


@pytest.mark.parametrize("ps,algo,cols", (("p-I", "shake128", 2), ("p-III", "shake256", 4), ("p-I", "shake256", 4),
                                          ("p-III", "shake128", 2)))
def test_qtesla_and_crossed_shapes(ntt, dev, ps, algo, cols):
    """21 samples a block (rate 168, two limbs), 8 + 9 over two blocks (rate 136, four), and the crossed
    17 a block and 10 + 11 over two; 512 samples end inside a block in all four"""
    got = check(ntt, dev, ps, 5, table_for(cols), algo)
    q = ntt.param_info(ps)["q"]
    c = np.where(got > q // 2, got.astype(np.int64) - q, got.astype(np.int64))
    assert (c > 0).any() and (c < 0).any() and (c == 0).any() and np.abs(c).max() > 20


@pytest.mark.parametrize("algo", ("shake128", "shake256"))
@pytest.mark.parametrize("cols", (1, 3))
def test_one_and_three_limbs(ntt, dev, algo, cols):
    """42 / 34 samples a block; 14 a block and 11 + 11 + 12 over three blocks"""
    check(ntt, dev, "p-I", 3, table_for(cols), algo)


@pytest.mark.parametrize("ps", ("p-III-4096", "p-III-8192"))
def test_large_n(ntt, dev, ps):
    """8 and 16 chunks a polynomial"""
    check(ntt, dev, ps, 3, table_for(4), "shake256")


@pytest.mark.parametrize("ps,algo,cols,batch", (("p-I", "shake128", 2, 1), ("p-I", "shake128", 2, 31), ("p-I", "shake128", 2, 32),
                                                ("p-I", "shake128", 2, 33), ("p-III", "shake256", 4, 17)))
def test_batches_round_the_wave(ntt, dev, ps, algo, cols, batch):
    """p-I is two chunks a polynomial: 2, 62, 64 and 66 lanes; p-III four: 68 lanes, a 4-lane tail wave"""
    check(ntt, dev, ps, batch, table_for(cols), algo)


def test_nonces(ntt, dev):
    ps, algo, table = "p-I", "shake128", table_for(2)
    for nonce in (1, 255):
        check(ntt, dev, ps, 3, table, algo, nonce=nonce)
    tensor = [0, 1, 255, 3, 7]
    a = check(ntt, dev, ps, 5, table, algo, nonces=tensor)      # row by row the scalar calls' model
    check(ntt, dev, ps, 5, table, algo, nonces=tensor, nonce=2)   # 255 + 2 wraps to 1
    check(ntt, dev, ps, 5, table, algo, nonces=[255] * 5, nonce=255)
    for b, nonce in enumerate(tensor):
        assert np.array_equal(run(ntt, dev, ps, 5, table, algo, nonce=nonce)[b], a[b]), (b, nonce)
    # the two chunks of a polynomial: the same nonce, different customisation
    assert not np.array_equal(a[0, :512], a[0, 512:])
    # p-III at rate 136: a different nonce in every polynomial of the wave, and a tail wave
    check(ntt, dev, "p-III", 17, table_for(4), "shake256", nonces=[(5 * b) % 7 for b in range(17)])


@pytest.mark.parametrize("algo,seedlen", (("shake128", 8), ("shake128", 64), ("shake128", 160), ("shake256", 128)))
def test_seed_lengths(ntt, dev, algo, seedlen):
    """one lane of seed, qTESLA-III's 64 bytes, and the longest: all but the last lane of the absorb block"""
    check(ntt, dev, "p-I", 3, table_for(2), algo, seedlen=seedlen)


def test_non_default_stream(ntt, dev):
    torch.cuda.synchronize(dev)
    check(ntt, dev, "p-III", 5, table_for(4), "shake256", stream=torch.cuda.Stream(device=dev))


def test_one_row(ntt, dev):
    got = check(ntt, dev, "p-I", 3, (table_for(2)[0],), "shake128")   # T_0: about one sample in 21 stays below it
    q = ntt.param_info("p-I")["q"]
    assert set(np.unique(got).tolist()) == {0, 1, q - 1}


def test_all_zero_table(ntt, dev):
    """every sample reaches every row: +-rows, by the sign bit alone"""
    rows, q = 9, ntt.param_info("p-I")["q"]
    got = check(ntt, dev, "p-I", 3, ((0, 0),) * rows, "shake128")
    assert set(np.unique(got).tolist()) == {rows, q - rows}


def test_all_ones_table(ntt, dev):
    """no sample reaches a row: 0 whatever the sign bit, never q"""
    got = check(ntt, dev, "p-I", 3, ((G.LIMB, G.LIMB),) * 5, "shake128")
    assert not got.any()


@pytest.mark.parametrize("algo,cols", (("shake128", 2), ("shake256", 4)))
def test_rows_at_the_samples(ntt, dev, algo, cols):
    """rows equal to chosen samples' R, R - 1 and R + 1 (equality, and rows that differ from a sample in
    the last limb alone), R with 2^(31 k) added or taken away for every limb k (a difference in limb k
    alone), and R with the limbs below k cleared or all set (a borrow through every lower limb)"""
    info = ntt.param_info("p-I")
    n, top = info["n"], 1 << (31 * cols)
    rows = []
    for idx, picks in ((0, (0, 1, 511, 512, 1023)), (2, (20, 21, 700))):   # both chunks, block edges, two polynomials
        words = G.sample_words(K.seeds(idx + 1)[idx], n, cols, algo, 0)
        for i in picks:
            R = G.sample_value(words[i], cols)
            rows += [R, R - 1, R + 1]
            for k in range(1, cols):
                rows += [R + (1 << (31 * k)), R - (1 << (31 * k)), (R >> (31 * k)) << (31 * k), R | ((1 << (31 * k)) - 1)]
    rows = [T for T in dict.fromkeys(rows) if 0 <= T < top][:G.ROWS_MAX]
    assert len(rows) >= 24 * cols
    table = tuple(tuple(G.limbs(T, cols)) for T in rows)
    got = check(ntt, dev, "p-I", 3, table, algo)
    # the picked samples are decided by equality: the model's count there includes the row R itself
    words = G.sample_words(K.seeds(1)[0], n, cols, algo, 0)
    R0 = G.sample_value(words[0], cols)
    m = sum(R0 >= T for T in rows)
    assert sum(R0 > T for T in rows) == m - 1 and got[0, 0] in (m, info["q"] - m)


def test_bit_31_of_a_table_word_is_ignored(ntt, dev):
    table = table_for(2)
    marked = tuple(tuple(w | (0x80000000 if (j + k) % 3 else 0) for k, w in enumerate(row)) for j, row in enumerate(table))
    a = check(ntt, dev, "p-I", 3, marked, "shake128")
    assert np.array_equal(a, run(ntt, dev, "p-I", 3, table, "shake128"))
    table4 = table_for(4)
    marked4 = tuple(tuple(w | 0x80000000 for w in row) for row in table4)
    check(ntt, dev, "p-I", 3, marked4, "shake256")


def test_wrapper_rejects_before_the_call(ntt, dev):
    out = torch.zeros((3, 2048), dtype=torch.int32, device=dev)
    seed = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
    cdt = torch.zeros((110, 4), dtype=torch.int32, device=dev)
    nonces = torch.zeros(3, dtype=torch.int32, device=dev)
    for nonce in (-1, 256):
        with pytest.raises(ValueError):
            ntt.poly_sample_gauss(out, seed, cdt, "p-III", nonce=nonce)
    with pytest.raises(ValueError):
        ntt.poly_sample_gauss(out, seed, cdt, "p-III", algo="sha3")
    for bad in (torch.zeros((129, 4), dtype=torch.int32, device=dev), torch.zeros((110, 5), dtype=torch.int32, device=dev),
                torch.zeros((0, 4), dtype=torch.int32, device=dev), torch.zeros(440, dtype=torch.int32, device=dev),
                torch.zeros((110, 8), dtype=torch.int32, device=dev)[:, :4]):
        with pytest.raises(ValueError):
            ntt.poly_sample_gauss(out, seed, bad, "p-III")
    with pytest.raises(TypeError):
        ntt.poly_sample_gauss(out, seed, cdt.to(torch.int64), "p-III")
    with pytest.raises(ValueError):
        ntt.poly_sample_gauss(out, seed, cdt.cpu(), "p-III")
    with pytest.raises(ValueError):
        ntt.poly_sample_gauss(out, seed[:2].contiguous(), cdt, "p-III")
    with pytest.raises(ValueError):
        ntt.poly_sample_gauss(out, seed[:, :12].contiguous(), cdt, "p-III")
    with pytest.raises(ValueError):
        ntt.poly_sample_gauss(out, torch.zeros((3, 136), dtype=torch.uint8, device=dev), cdt, "p-III", algo="shake256")
    with pytest.raises(ValueError):
        ntt.poly_sample_gauss(out, seed, cdt, "p-III", nonces=nonces[:2].contiguous())
    with pytest.raises(TypeError):
        ntt.poly_sample_gauss(out, seed, cdt, "p-III", nonces=nonces.to(torch.uint8))
    with pytest.raises(TypeError):
        ntt.poly_sample_gauss(out.to(torch.uint8), seed, cdt, "p-III")
    with pytest.raises(KeyError):
        ntt.poly_sample_gauss(out, seed, cdt, "p-IX")
