"""poly_mul_ntt_kl_round on the GPU: bit-identical to poly_mul_ntt_kl into a
temporary followed by the rounding.

    want = round_model.poly_round(poly_mul_ntt_kl(ys, ahat, add), q, d)

on the same device operands; poly_mul_ntt_kl is bit-exact against the CPU
oracle in its own tests and is not the code under test here.  The small
batches are test_gpu_mul_ntt_kl.py's (they straddle a workgroup's tail and the
n = 1024 half-wave tail); one batch per set lies just above the launch shape's
split threshold.  Every output lies between guards and is prefilled with
garbage; an output not asked for keeps it.
"""
import numpy as np
import pytest
import torch

import round_model as M
from conftest import PARAM_SETS

pytestmark = pytest.mark.gpu

KS = (1, 5, 8)
K_POOL = max(KS)
GARBAGE8 = 0x5A
GARBAGE32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
NGUARD = 8
_POOL = {}


def _upw(n):
    return 2 if n == 1024 else 1   # polynomials per wave unit (Lane::UPW)


def _small_batches(ntt, ps):
    n = ntt.param_info(ps)["n"]
    full = ntt.mul_kl_shape(ps, 2)["waves"] * _upw(n)
    return sorted({1, 2, 3, 7, full - 1, full, full + 1})


def _pool(ntt, dev, ps):
    """Device operands shared by the small cases of one set: y [2, B, n],
    ahat [K_POOL, 2, n] and add [B, K_POOL, n], entries < 2q (some >= q)."""
    if ps not in _POOL:
        info = ntt.param_info(ps)
        n, q = info["n"], info["q"]
        B = max(_small_batches(ntt, ps))
        rng = np.random.default_rng(0x20D5 + n + q % 1000)
        y, ahat, add = (rng.integers(0, 2 * q, shape, dtype=np.uint32)
                        for shape in ((2, B, n), (K_POOL, 2, n), (B, K_POOL, n)))
        _POOL[ps] = dict(n=n, q=q, y=ntt.from_numpy_u32(y, dev), ahat=ntt.from_numpy_u32(ahat, dev),
                         add=ntt.from_numpy_u32(add, dev))
    return _POOL[ps]


def _operands(p, batch, k, l):
    """Contiguous device operands of one case, cut from the pool."""
    n = p["n"]
    ys = [p["y"].view(2, -1, n)[j, :batch].contiguous().view(-1) for j in range(l)]
    ahat = p["ahat"].view(K_POOL, 2, n)[:k, :l].contiguous().view(-1)
    add = p["add"].view(-1, K_POOL, n)[:batch, :k].contiguous().view(-1)
    return ys, ahat, add


def _check(ntt, dev, ps, ys, ahat, add, batch, k, d, variant="hi+norms", stream=None):
    """One fused call against poly_mul_ntt_kl + the model; returns the wanted norms."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    npoly = batch * k
    full = torch.empty(npoly * n, dtype=torch.int32, device=dev)
    ntt.poly_mul_ntt_kl(full, ys, ahat, ps, add=add)
    w = ntt.to_numpy_u32(full).reshape(npoly, n)
    want_hi, want_norms = M.poly_round(w, q, d)
    before = [t.clone() for t in (*ys, ahat)] + ([] if add is None else [add.clone()])
    hbuf = torch.full((npoly * n + 2 * n,), GARBAGE8, dtype=torch.uint8, device=dev)
    nbuf = torch.full((2 * npoly + 2 * NGUARD,), GARBAGE32, dtype=torch.int32, device=dev)
    hi, norms = hbuf[n:n + npoly * n], nbuf[NGUARD:NGUARD + 2 * npoly]
    torch.cuda.synchronize(dev)
    ntt.poly_mul_ntt_kl_round(ys, ahat, ps, d, hi=hi if "hi" in variant else None,
                              norms=norms if "norms" in variant else None, add=add, stream=stream)
    if stream is not None:
        stream.synchronize()
    where = f"{ps} batch {batch} k {k} l {len(ys)} d {d} {variant}"
    assert bool((hbuf[:n] == GARBAGE8).all()) and bool((hbuf[-n:] == GARBAGE8).all()), f"{where}: store outside hi"
    assert bool((nbuf[:NGUARD] == GARBAGE32).all()) and bool((nbuf[-NGUARD:] == GARBAGE32).all()), \
        f"{where}: store outside norms"
    if "hi" in variant:
        assert np.array_equal(hi.cpu().numpy().view(np.int8).reshape(npoly, n), want_hi), f"{where}: hi"
    else:
        assert bool((hi == GARBAGE8).all()), f"{where}: hi written though not asked for"
    if "norms" in variant:
        assert np.array_equal(ntt.to_numpy_u32(norms).reshape(npoly, 2), want_norms), f"{where}: norms"
    else:
        assert bool((norms == GARBAGE32).all()), f"{where}: norms written though not asked for"
    for t, b in zip((*ys, ahat) if add is None else (*ys, ahat, add), before):
        assert torch.equal(t, b), f"{where}: input changed"
    return want_norms


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("l", (1, 2))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_exact_small_batches(ntt, dev, ps, k, l, with_add):
    p = _pool(ntt, dev, ps)
    for batch in _small_batches(ntt, ps):
        ys, ahat, add = _operands(p, batch, k, l)
        for d in (M.OWN_D[ps], M.min_d(p["q"])):
            _check(ntt, dev, ps, ys, ahat, add if with_add else None, batch, k, d)


@pytest.mark.parametrize("variant", ("hi", "norms"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_one_output(ntt, dev, ps, variant):
    p = _pool(ntt, dev, ps)
    for batch, k, l in ((7, 5, 2), (3, 5, 1)):
        ys, ahat, add = _operands(p, batch, k, l)
        _check(ntt, dev, ps, ys, ahat, add, batch, k, M.OWN_D[ps], variant)
    # norms alone: a d too small for hi bytes is served
    if variant == "norms":
        ys, ahat, add = _operands(p, 3, 5, 2)
        d = M.min_d(p["q"]) - 1
        full = torch.empty(3 * 5 * p["n"], dtype=torch.int32, device=dev)
        ntt.poly_mul_ntt_kl(full, ys, ahat, ps, add=add)
        c, lo, _ = M.split(ntt.to_numpy_u32(full).reshape(15, -1), p["q"], d)
        norms = torch.empty(30, dtype=torch.int32, device=dev)
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, d, norms=norms, add=add)
        want = np.stack([np.abs(c).max(axis=1), np.abs(lo).max(axis=1)], axis=1).astype(np.uint32)
        assert np.array_equal(ntt.to_numpy_u32(norms).reshape(15, 2), want)


@pytest.mark.parametrize("ps,k,above", (("ref", 4, 1025), ("p-I", 4, 1025), ("p-III", 5, 363)))
def test_just_above_the_split_threshold(ntt, dev, ps, k, above):
    """One work unit per b instead of the rows spread over k workgroups."""
    assert ntt.mul_kl_shape(ps, 2)["split_max"] + 1 == above
    n = ntt.param_info(ps)["n"]
    ys = [torch.empty(above * n, dtype=torch.int32, device=dev) for _ in range(2)]
    ahat = torch.empty(k * 2 * n, dtype=torch.int32, device=dev)
    add = torch.empty(above * k * n, dtype=torch.int32, device=dev)
    for i, t in enumerate((*ys, ahat, add)):
        ntt.fill_uniform(t, ps, 0xAB07E + i)
    _check(ntt, dev, ps, ys, ahat, add, above, k, M.OWN_D[ps])


def _positions(n):
    return (0, 1, 31, 32, 63, 64, 255, 256, n // 2 - 1, n // 2, n - 1)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_planted_maxima_through_the_addend(ntt, dev, ps):
    """ys = 0, so w = add: all-ones polynomials with one planted coefficient
    per (position, sign), then the two maxima at different positions."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    d, m = M.OWN_D[ps], (q - 1) // 2
    big, half = (m >> d) << d, 1 << (d - 1)
    pos = _positions(n)
    B, k = len(pos), 2
    ys = [torch.zeros(B * n, dtype=torch.int32, device=dev) for _ in range(2)]
    ahat = _pool(ntt, dev, ps)["ahat"].view(K_POOL, 2, n)[:k].contiguous().view(-1)
    w = np.ones((B, k, n), dtype=np.uint32)
    for b, p in enumerate(pos):
        w[b, 0, p], w[b, 1, p] = m, q - m
    want = _check(ntt, dev, ps, ys, ahat, ntt.from_numpy_u32(w, dev), B, k, d)
    assert np.all(want[:, 0] == m)
    w = np.ones((B, k, n), dtype=np.uint32)
    for b, p in enumerate(pos):
        p2 = pos[(b + 4) % len(pos)]
        w[b, 0, p], w[b, 0, p2] = big, half
        w[b, 1, p], w[b, 1, p2] = big, q - (half - 1)
    want = _check(ntt, dev, ps, ys, ahat, ntt.from_numpy_u32(w, dev), B, k, d).reshape(B, k, 2)
    assert np.all(want[:, :, 0] == big) and np.all(want[:, 0, 1] == half) and np.all(want[:, 1, 1] == half - 1)
    # the signer's form, one y: the norms alone
    _check(ntt, dev, ps, ys[:1], ahat.view(k, 2, n)[:, 0].contiguous().view(-1), ntt.from_numpy_u32(w, dev), B, k, d, "norms")


def test_non_default_stream(ntt, dev):
    ps = "p-III"
    p = _pool(ntt, dev, ps)
    ys, ahat, add = _operands(p, 7, 5, 2)
    _check(ntt, dev, ps, ys, ahat, add, 7, 5, M.OWN_D[ps], stream=torch.cuda.Stream(device=dev))


def test_wrapper_checks(ntt, dev):
    ps = "p-III"
    p = _pool(ntt, dev, ps)
    n = p["n"]
    ys, ahat, add = _operands(p, 3, 5, 2)
    hi = torch.empty(15 * n, dtype=torch.uint8, device=dev)
    norms = torch.empty(30, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, 24)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, 24, hi=hi[:-16])
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, 24, norms=norms[:-2])
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, 24, norms=norms, add=add[:-n])
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round([ys[0], ys[1][:-n]], ahat, ps, 24, norms=norms)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, 24, hi=hi.cpu())
    with pytest.raises(ntt.NTTError):   # an output over an input
        ntt.poly_mul_ntt_kl_round(ys, ahat, ps, 24, norms=add[:30], add=add)
