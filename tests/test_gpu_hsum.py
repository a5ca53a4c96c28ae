"""poly_hsum on the GPU against the sum of the h largest |c| by numpy's sort
(gauss_model.hsum is the same by a threshold; both are compared on one case):
all five sets, batches 1, 3 and 65, h from 1 to n, and inputs built round the
tie term -- exactly h - 1, h and h + 1 copies of the maximum, a block of equal
values straddling the h-th place -- besides random canonical and lazy input,
zeros, all-equal, +-(q-1)/2 and real sampler output.  The sums lie between
guard words and the input must come back unchanged."""
import numpy as np
import pytest
import torch

import gauss_model as G
import keccak_model as K

pytestmark = pytest.mark.gpu

SETS = ("ref", "p-I", "p-III", "p-III-4096", "p-III-8192")
SET_H = {"ref": 25, "p-I": 25, "p-III": 40, "p-III-4096": 40, "p-III-8192": 40}
GUARD = -0x5A5A5A5A5A5A5A5B


def hs(ps_h, n):
    return sorted({1, 2, ps_h, n - 1, n})


def want(w, q, h):
    """[batch] sums of the h largest |c| of w [batch, n] (uint32, entries < 2q)"""
    x = w.astype(np.int64) % q
    a = np.sort(np.minimum(x, q - x), axis=1)
    return a[:, a.shape[1] - h:].sum(axis=1)


def run(ntt, dev, ps, w, h, stream=None):
    """the sums as int64 [batch]; checks the guards and the input"""
    batch = w.shape[0]
    tw = ntt.from_numpy_u32(w, dev)
    buf = torch.full((batch + 4,), GUARD, dtype=torch.int64, device=dev)
    sums = buf[2:-2]
    sums.fill_(-1)
    assert ntt.poly_hsum(sums, tw, ps, h, stream=stream) is sums
    if stream is not None:
        stream.synchronize()
    assert buf[:2].tolist() == [GUARD] * 2 and buf[-2:].tolist() == [GUARD] * 2, "store outside the sums"
    assert np.array_equal(ntt.to_numpy_u32(tw).reshape(w.shape), w), "input changed"
    return sums.cpu().numpy()


def check(ntt, dev, ps, w, h_list=None):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    w = np.ascontiguousarray(w, dtype=np.uint32).reshape(-1, n)
    for h in h_list or hs(SET_H[ps], n):
        got = run(ntt, dev, ps, w, h)
        exp = want(w, q, h)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{ps} h {h}: polynomial {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"


def from_centred(c, q):
    return (np.asarray(c, dtype=np.int64) % q).astype(np.uint32)


@pytest.mark.parametrize("ps", SETS)
@pytest.mark.parametrize("batch", (1, 3, 65))
def test_random_canonical_and_lazy(ntt, dev, ps, batch):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(batch * 8 + ntt.PARAM_SETS[ps])
    check(ntt, dev, ps, rng.integers(0, q, (batch, n)))
    lazy = rng.integers(q, 2 * q, (batch, n))
    lazy[:, ::3] -= q   # both ranges within one polynomial
    check(ntt, dev, ps, lazy, [SET_H[ps], n])


@pytest.mark.parametrize("ps", SETS)
def test_zero_equal_and_extremes(ntt, dev, ps):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    half = (q - 1) // 2
    w = np.zeros((6, n), dtype=np.uint32)
    w[1, :] = 7                       # all equal: h * 7
    w[2, :] = q - 7                   # ... and as negatives
    w[3, :] = half                    # +(q-1)/2 everywhere: h (q-1)/2 needs more than 32 bits
    w[4, ::2], w[4, 1::2] = half, half + 1          # +-(q-1)/2 alternating
    w[5, :] = q                       # lazy zero
    w[5, 5], w[5, n - 1] = q + half + 1, half       # two extremes among zeros
    check(ntt, dev, ps, w)
    assert int(want(w, q, n)[3]) == n * half > 1 << 32
    got = run(ntt, dev, ps, w, n)
    assert got.tolist() == [0, 7 * n, 7 * n, n * half, n * half, 2 * half]


@pytest.mark.parametrize("ps", SETS)
def test_copies_of_the_maximum(ntt, dev, ps):
    """exactly h - 1, h and h + 1 copies of the maximum over a small-valued rest (which itself ties)"""
    info = ntt.param_info(ps)
    n, q, h = info["n"], info["q"], SET_H[ps]
    rng = np.random.default_rng(n + h)
    rows = []
    for copies in (h - 1, h, h + 1):
        for top in (50, (q - 1) // 2):
            c = rng.integers(-9, 10, n)
            c[rng.permutation(n)[:copies]] = top * rng.choice((-1, 1), copies)
            rows.append(from_centred(c, q))
    w = np.stack(rows)
    check(ntt, dev, ps, w, [h - 1, h, h + 1, n])
    exp = want(w, q, h)
    assert exp[0] == (h - 1) * 50 + 9 and exp[2] == h * 50 and exp[4] == h * 50   # the rest's maximum fills one place


@pytest.mark.parametrize("ps", SETS)
def test_tie_block_across_the_hth_place(ntt, dev, ps):
    """distinct values above a block of equal ones that begins before the h-th place and ends after it:
    the block counts exactly h - #{above} times"""
    info = ntt.param_info(ps)
    n, q, h = info["n"], info["q"], SET_H[ps]
    rng = np.random.default_rng(n - h)
    rows, exps = [], []
    for above, block, t in ((h - 1, 2, 1000), (h - 3, 7, 1000), (1, n - 1, 3), (h // 2, h, 1 << 20), (0, h + 1, 12345),
                            (h - 1, 64, (q - 1) // 2 - h)):
        c = np.zeros(n, dtype=np.int64)
        vals = np.concatenate([t + 1 + np.arange(above), np.full(block, t), rng.integers(0, min(t, 900), n - above - block)])
        c[rng.permutation(n)] = vals * rng.choice((-1, 1), n)
        rows.append(from_centred(c, q))
        exps.append(int((t + 1 + np.arange(above)).sum()) + (h - above) * t)
    w = np.stack(rows)
    assert want(w, q, h).tolist() == exps
    check(ntt, dev, ps, w, [h - 1, h, h + 1])
    # the model of the header's sentence, by a threshold, on the same rows
    assert [G.hsum(row, q, h) for row in rows] == exps


@pytest.mark.parametrize("ps,algo,cols,rows", (("p-I", "shake128", 2, 77), ("p-III", "shake256", 4, 110)))
def test_sampler_output(ntt, dev, ps, algo, cols, rows):
    """what key generation feeds it: poly_sample_gauss's polynomials, sigma = 8.5 (ties everywhere)"""
    info = ntt.param_info(ps)
    n, q, batch = info["n"], info["q"], 6
    seeds = torch.from_numpy(np.frombuffer(b"".join(K.seeds(batch)), dtype=np.uint8).reshape(batch, 32).copy()).to(dev)
    cdt = ntt.from_numpy_u32(np.array(G.cdt_table(8.5, rows, cols), dtype=np.uint32), dev)
    out = torch.empty((batch, n), dtype=torch.int32, device=dev)
    ntt.poly_sample_gauss(out, seeds, cdt, ps, algo=algo)
    w = ntt.to_numpy_u32(out).reshape(batch, n)
    check(ntt, dev, ps, w)
    s = want(w, q, SET_H[ps])
    assert (s > 10 * SET_H[ps]).all() and (s < 40 * SET_H[ps]).all()   # h values near 2.5 to 3.5 sigma


def test_non_default_stream(ntt, dev):
    info = ntt.param_info("p-III")
    w = np.random.default_rng(5).integers(0, 2 * info["q"], (9, info["n"])).astype(np.uint32)
    torch.cuda.synchronize(dev)
    got = run(ntt, dev, "p-III", w, 40, stream=torch.cuda.Stream(device=dev))
    assert np.array_equal(got, want(w, info["q"], 40))


def test_wrapper_rejects_before_the_call(ntt, dev):
    w = torch.zeros((3, 2048), dtype=torch.int32, device=dev)
    sums = torch.zeros(3, dtype=torch.int64, device=dev)
    for h in (0, -1, 2049):
        with pytest.raises(ValueError):
            ntt.poly_hsum(sums, w, "p-III", h)
    with pytest.raises(ValueError):
        ntt.poly_hsum(sums[:2].contiguous(), w, "p-III", 40)
    with pytest.raises(ValueError):
        ntt.poly_hsum(torch.zeros(6, dtype=torch.int64, device=dev)[::2], w, "p-III", 40)
    with pytest.raises(ValueError):
        ntt.poly_hsum(sums.cpu(), w, "p-III", 40)
    with pytest.raises(TypeError):
        ntt.poly_hsum(sums.to(torch.int32), w, "p-III", 40)
    with pytest.raises(TypeError):
        ntt.poly_hsum(sums, w.to(torch.int64), "p-III", 40)
    with pytest.raises(KeyError):
        ntt.poly_hsum(sums, w, "p-IX", 40)
