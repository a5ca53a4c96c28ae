"""poly_round on the GPU, exact against the numpy model (round_model.py).

Every hi buffer lies between n guard bytes and every norms buffer between
guard words, all prefilled with garbage; an output that is not asked for keeps
its garbage, and the input is unchanged.  Random inputs give nearly the same
two maxima for every polynomial, so the reductions are checked with planted
maxima: one coefficient per polynomial, at every position at which the lane,
the wave or the half of the polynomial changes.
"""
import numpy as np
import pytest
import torch

import round_model as M
from conftest import LARGE_SETS, PARAM_SETS

pytestmark = pytest.mark.gpu

SETS = PARAM_SETS + LARGE_SETS
BATCHES = (1, 3, 257)
GARBAGE8 = 0x5A
GARBAGE32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
NGUARD = 8   # guard words on each side of norms (keeps it 8-byte aligned)
VARIANTS = ("hi+norms", "hi", "norms")


def _hi_buf(dev, nbytes, n):
    buf = torch.full((nbytes + 2 * n,), GARBAGE8, dtype=torch.uint8, device=dev)
    return buf, buf[n:n + nbytes]


def _norms_buf(dev, npoly):
    buf = torch.full((2 * npoly + 2 * NGUARD,), GARBAGE32, dtype=torch.int32, device=dev)
    return buf, buf[NGUARD:NGUARD + 2 * npoly]


def _check_round(ntt, dev, ps, w, d, variant, stream=None):
    """One poly_round call on the host polynomials w [B, n]; every assertion
    of the module's docstring."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    B = w.shape[0]
    tw = ntt.from_numpy_u32(w, dev)
    hbuf, hi = _hi_buf(dev, B * n, n)
    nbuf, norms = _norms_buf(dev, B)
    ntt.poly_round(tw, ps, d, hi=hi if "hi" in variant else None, norms=norms if "norms" in variant else None,
                   stream=stream)
    if stream is not None:
        stream.synchronize()
    want_hi, want_norms = M.poly_round(w, q, d)
    assert bool((hbuf[:n] == GARBAGE8).all()) and bool((hbuf[-n:] == GARBAGE8).all()), "store outside hi"
    assert bool((nbuf[:NGUARD] == GARBAGE32).all()) and bool((nbuf[-NGUARD:] == GARBAGE32).all()), "store outside norms"
    if "hi" in variant:
        got = hi.cpu().numpy().view(np.int8).reshape(B, n)
        assert np.array_equal(got, want_hi), f"{ps} batch {B} d {d} {variant}: hi"
    else:
        assert bool((hi == GARBAGE8).all()), "hi written though not asked for"
    if "norms" in variant:
        got = ntt.to_numpy_u32(norms).reshape(B, 2)
        assert np.array_equal(got, want_norms), f"{ps} batch {B} d {d} {variant}: norms"
    else:
        assert bool((norms == GARBAGE32).all()), "norms written though not asked for"
    assert np.array_equal(ntt.to_numpy_u32(tw).reshape(w.shape), w), "input changed"
    return want_norms


def _random_with_edges(rng, B, n, q, d):
    w = rng.integers(0, 2 * q, (B, n), dtype=np.uint32)
    edges = M.edge_values(q, d)
    for b in range(B):   # every edge value in every polynomial, at positions of its own
        w[b, rng.permutation(n)[:len(edges)]] = edges
    return w


@pytest.mark.parametrize("dsel", (0, 1, 2), ids=("min_d", "own_d", "d30"))
@pytest.mark.parametrize("ps", SETS)
def test_exact(ntt, dev, ps, dsel):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    d = (M.min_d(q), M.OWN_D[ps], 30)[dsel]
    rng = np.random.default_rng(0x20D + n + d)
    for B in BATCHES:
        w = _random_with_edges(rng, B, n, q, d)
        for variant in VARIANTS:
            _check_round(ntt, dev, ps, w, d, variant)


def _positions(n):
    return (0, 1, 31, 32, 63, 64, 255, 256, n // 2 - 1, n // 2, n - 1)


@pytest.mark.parametrize("ps", SETS)
def test_planted_maximum(ntt, dev, ps):
    """All-ones polynomials with one coefficient +m or q - m (c = -m),
    m = (q-1)/2, one polynomial per (position, sign): max |c| is m exactly,
    wherever it lies."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    d, m = M.OWN_D[ps], (q - 1) // 2
    pos = _positions(n)
    w = np.ones((2 * len(pos), n), dtype=np.uint32)
    for i, p in enumerate(pos):
        w[2 * i, p], w[2 * i + 1, p] = m, q - m
    want = _check_round(ntt, dev, ps, w, d, "hi+norms")
    assert np.all(want[:, 0] == m)
    _check_round(ntt, dev, ps, w, d, "norms")


@pytest.mark.parametrize("ps", SETS)
def test_two_maxima_apart(ntt, dev, ps):
    """The two maxima at different positions: the largest multiple of 2^d up
    to (q-1)/2 (large |c|, lo = 0) and, elsewhere, 2^(d-1) (lo at its positive
    bound), or in the twin q - (2^(d-1) - 1) (lo = -(2^(d-1) - 1)); all-ones
    elsewhere."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    d = M.OWN_D[ps]
    big, half = (((q - 1) // 2) >> d) << d, 1 << (d - 1)
    assert 0 < half < big <= (q - 1) // 2
    pos = _positions(n)
    w = np.ones((2 * len(pos), n), dtype=np.uint32)
    for i, p in enumerate(pos):
        p2 = pos[(i + 4) % len(pos)]
        w[2 * i, p], w[2 * i, p2] = big, half
        w[2 * i + 1, p], w[2 * i + 1, p2] = big, q - (half - 1)
    want = _check_round(ntt, dev, ps, w, d, "hi+norms")
    assert np.array_equal(want[0::2], np.tile(np.array([big, half], dtype=np.uint32), (len(pos), 1)))
    assert np.array_equal(want[1::2], np.tile(np.array([big, half - 1], dtype=np.uint32), (len(pos), 1)))
    _check_round(ntt, dev, ps, w, d, "norms")


def test_non_default_stream(ntt, dev):
    ps = "p-III-8192"
    info = ntt.param_info(ps)
    w = _random_with_edges(np.random.default_rng(5), 3, info["n"], info["q"], M.OWN_D[ps])
    torch.cuda.synchronize(dev)
    _check_round(ntt, dev, ps, w, M.OWN_D[ps], "hi+norms", stream=torch.cuda.Stream(device=dev))


def test_wrapper_checks(ntt, dev):
    ps, n = "p-III", 2048
    w = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    hi = torch.zeros(2 * n, dtype=torch.int8, device=dev)
    norms = torch.zeros(4, dtype=torch.int32, device=dev)
    ntt.poly_round(w, ps, 24, hi=hi, norms=norms)   # int8 storage is accepted
    with pytest.raises(ValueError):
        ntt.poly_round(w, ps, 24)
    with pytest.raises(ValueError):
        ntt.poly_round(w, ps, 24, hi=hi[:-1])
    with pytest.raises(ValueError):
        ntt.poly_round(w, ps, 24, norms=norms[:2])
    with pytest.raises(ValueError):
        ntt.poly_round(w, ps, 24, hi=hi.cpu())
    with pytest.raises(ValueError):
        ntt.poly_round(w, ps, 24, norms=norms.view(2, 2).t())
    with pytest.raises(ValueError):
        ntt.poly_round(w, ps, 0, norms=norms)
    with pytest.raises(TypeError):
        ntt.poly_round(w, ps, 24, hi=torch.zeros(2 * n, dtype=torch.int16, device=dev))
    with pytest.raises(ntt.NTTError):
        ntt.poly_round(w, ps, 21, hi=hi)   # hi would not fit a byte
