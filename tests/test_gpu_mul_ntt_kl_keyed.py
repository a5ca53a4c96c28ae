"""poly_mul_ntt_kl_keyed / poly_mul_ntt_kl_round_keyed on the GPU, bit-exact.

The yardstick is the unkeyed product, which is bit-exact against the CPU
oracle in its own tests and is not the code under test here: for each key j
the messages whose (clamped) index is j are gathered, the unkeyed
poly_mul_ntt_k (l = 1) / poly_mul_ntt_kl (l = 2) is run on key j's block and
the gathered addend, and the result is scattered back into want_w.  Then

    poly_mul_ntt_kl_keyed        == want_w
    poly_mul_ntt_kl_round_keyed  == round_model.poly_round(want_w, q, d)

The small batches are test_gpu_mul_ntt_kl_round.py's (odd batches at n = 1024,
a workgroup's tail; the launch is in the split shape there); one batch per set
lies just above the split threshold.  Outputs lie between garbage-filled
guards, an output not asked for keeps its garbage, d_key has garbage before and
after its batch words, and every input is unchanged afterwards.
"""
import numpy as np
import pytest
import torch

import round_model as M
from conftest import PARAM_SETS

pytestmark = pytest.mark.gpu

KS = (1, 5, 8)
K_POOL = max(KS)
NKEYS = 3
GARBAGE8 = 0x5A
GARBAGE32 = int(np.uint32(0xA5A5A5A5).view(np.int32))   # as a key index: far beyond any nkeys
NGUARD = 8
_POOL = {}


def _upw(n):
    return 2 if n == 1024 else 1   # polynomials per wave unit (Lane::UPW)


def _small_batches(ntt, ps):
    n = ntt.param_info(ps)["n"]
    full = ntt.mul_kl_shape(ps, 2)["waves"] * _upw(n)
    return sorted({1, 2, 3, 7, full - 1, full, full + 1})


def _pool(ntt, dev, ps):
    """Device operands shared by the small cases of one set: y [2, B, n], ahat
    [B, K_POOL, 2, n] (B keys: enough for keys = None with nkeys = batch) and
    add [B, K_POOL, n], entries < 2q (some >= q)."""
    if ps not in _POOL:
        info = ntt.param_info(ps)
        n, q = info["n"], info["q"]
        B = max(_small_batches(ntt, ps))
        rng = np.random.default_rng(0x4E7ED + n + q % 1000)
        y, ahat, add = (rng.integers(0, 2 * q, shape, dtype=np.uint32)
                        for shape in ((2, B, n), (B, K_POOL, 2, n), (B, K_POOL, n)))
        _POOL[ps] = dict(n=n, q=q, y=ntt.from_numpy_u32(y, dev), ahat=ntt.from_numpy_u32(ahat, dev),
                         add=ntt.from_numpy_u32(add, dev))
    return _POOL[ps]


def _operands(p, batch, k, l, nkeys):
    """Contiguous device operands of one case, cut from the pool."""
    ys = [p["y"][j, :batch].contiguous().view(-1) for j in range(l)]
    ahat = p["ahat"][:nkeys, :k, :l].contiguous()
    add = p["add"][:batch, :k].contiguous().view(-1)
    return ys, ahat, add


def _keys(pattern, batch, nkeys):
    """The raw indices of a named pattern (uint32 values, or None for d_key = NULL)."""
    b = np.arange(batch, dtype=np.uint64)
    if pattern == "mixed":       # the two halves of every n = 1024 unit differ
        return ((5 * b + 1) % 3).astype(np.uint32)
    if pattern == "all2":
        return np.full(batch, 2, dtype=np.uint32)
    if pattern == "zeros":
        return np.zeros(batch, dtype=np.uint32)
    if pattern == "beyond":      # nkeys, nkeys + 7, 0xFFFFFFFF and valid ones in turn
        return np.array([(nkeys, 0, nkeys + 7, 1, 0xFFFFFFFF, nkeys - 1)[i % 6] for i in range(batch)], dtype=np.uint32)
    if pattern == "cycle":
        return (b % nkeys).astype(np.uint32)
    assert pattern == "none"
    return None


def _want_w(ntt, dev, ps, ys, ahat, add, raw, batch):
    """want_w [batch, k, n] (uint32, numpy) from the unkeyed products, key by key."""
    nkeys, k, l, n = ahat.shape
    eff = np.minimum(np.arange(batch, dtype=np.uint64) if raw is None else raw.astype(np.uint64), nkeys - 1)
    want = torch.empty((batch, k, n), dtype=torch.int32, device=dev)
    for j in sorted(set(eff.tolist())):
        idx = torch.from_numpy(np.flatnonzero(eff == j)).to(dev)
        yj = [y.view(batch, n)[idx].contiguous() for y in ys]
        aj = None if add is None else add.view(batch, k, n)[idx].contiguous()
        out = torch.empty((len(idx), k, n), dtype=torch.int32, device=dev)
        if l == 1:
            ntt.poly_mul_ntt_k(out, yj[0], ahat[j, :, 0].contiguous(), ps, add=aj)
        else:
            ntt.poly_mul_ntt_kl(out, yj, ahat[j].contiguous(), ps, add=aj)
        want[idx] = out
    return ntt.to_numpy_u32(want)


def _check(ntt, dev, ps, ys, ahat, add, raw, batch, ds, variants=("hi+norms",), stream=None, want=None):
    """The keyed full-width call and, per d and variant, the keyed rounding call
    against want_w; returns want_w."""
    nkeys, k, l, n = ahat.shape
    q = ntt.param_info(ps)["q"]
    npoly = batch * k
    if want is None:
        want = _want_w(ntt, dev, ps, ys, ahat, add, raw, batch)
    where = f"{ps} batch {batch} k {k} l {l} nkeys {nkeys} add {add is not None}"
    kbuf = keys = None
    if raw is not None:
        kbuf = torch.full((batch + 2 * NGUARD,), GARBAGE32, dtype=torch.int32, device=dev)
        keys = kbuf[NGUARD:NGUARD + batch]
        keys.copy_(torch.from_numpy(raw.view(np.int32)).to(dev))
    ins = [*ys, ahat] + ([] if add is None else [add]) + ([] if kbuf is None else [kbuf])
    before = [t.clone() for t in ins]

    def sync():
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize(dev)

    obuf = torch.full(((npoly + 2) * n,), GARBAGE32, dtype=torch.int32, device=dev)
    out = obuf[n:n + npoly * n]
    sync()
    ntt.poly_mul_ntt_kl_keyed(out, ys, ahat, keys, ps, add=add, stream=stream)
    sync()
    assert bool((obuf[:n] == GARBAGE32).all()) and bool((obuf[-n:] == GARBAGE32).all()), f"{where}: store outside out"
    assert np.array_equal(ntt.to_numpy_u32(out).reshape(batch, k, n), want), f"{where}: full width"
    for d in ds:
        want_hi, want_norms = M.poly_round(want.reshape(npoly, n), q, d)
        for variant in variants:
            hbuf = torch.full((npoly * n + 2 * n,), GARBAGE8, dtype=torch.uint8, device=dev)
            nbuf = torch.full((2 * npoly + 2 * NGUARD,), GARBAGE32, dtype=torch.int32, device=dev)
            hi, norms = hbuf[n:n + npoly * n], nbuf[NGUARD:NGUARD + 2 * npoly]
            sync()
            ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys, ps, d, hi=hi if "hi" in variant else None,
                                            norms=norms if "norms" in variant else None, add=add, stream=stream)
            sync()
            tag = f"{where} d {d} {variant}"
            assert bool((hbuf[:n] == GARBAGE8).all()) and bool((hbuf[-n:] == GARBAGE8).all()), f"{tag}: store outside hi"
            assert bool((nbuf[:NGUARD] == GARBAGE32).all()) and bool((nbuf[-NGUARD:] == GARBAGE32).all()), \
                f"{tag}: store outside norms"
            if "hi" in variant:
                assert np.array_equal(hi.cpu().numpy().view(np.int8).reshape(npoly, n), want_hi), f"{tag}: hi"
            else:
                assert bool((hi == GARBAGE8).all()), f"{tag}: hi written though not asked for"
            if "norms" in variant:
                assert np.array_equal(ntt.to_numpy_u32(norms).reshape(npoly, 2), want_norms), f"{tag}: norms"
            else:
                assert bool((norms == GARBAGE32).all()), f"{tag}: norms written though not asked for"
    for t, b in zip(ins, before):
        assert torch.equal(t, b), f"{where}: input changed"
    return want


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("l", (1, 2))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_exact_small_batches(ntt, dev, ps, k, l, with_add):
    p = _pool(ntt, dev, ps)
    ds = (M.OWN_D[ps], M.min_d(p["q"]))
    for batch in _small_batches(ntt, ps):
        for pattern in ("mixed", "all2", "none"):
            nkeys = batch if pattern == "none" else NKEYS
            ys, ahat, add = _operands(p, batch, k, l, nkeys)
            _check(ntt, dev, ps, ys, ahat, add if with_add else None, _keys(pattern, batch, nkeys), batch, ds)


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("l", (1, 2))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_one_key_equals_the_unkeyed_call(ntt, dev, ps, l, with_add):
    """All indices 0 with nkeys = 1: the unkeyed entry points, bit for bit."""
    p = _pool(ntt, dev, ps)
    n, k, d = p["n"], 5, M.OWN_D[ps]
    for batch in _small_batches(ntt, ps):
        ys, ahat, add = _operands(p, batch, k, l, 1)
        add = add if with_add else None
        rows = ahat[0].contiguous()
        w = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
        ntt.poly_mul_ntt_kl(w, ys, rows, ps, add=add)
        hi = torch.empty(batch * k * n, dtype=torch.int8, device=dev)
        norms = torch.empty(batch * k * 2, dtype=torch.int32, device=dev)
        ntt.poly_mul_ntt_kl_round(ys, rows, ps, d, hi=hi, norms=norms, add=add)
        for raw in (_keys("zeros", batch, 1), None):
            keys = None if raw is None else ntt.from_numpy_u32(raw, dev)
            w2, hi2, norms2 = torch.empty_like(w), torch.empty_like(hi), torch.empty_like(norms)
            ntt.poly_mul_ntt_kl_keyed(w2, ys, ahat, keys, ps, add=add)
            ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys, ps, d, hi=hi2, norms=norms2, add=add)
            assert torch.equal(w2, w) and torch.equal(hi2, hi) and torch.equal(norms2, norms), f"{ps} batch {batch} l {l}"


@pytest.mark.parametrize("l", (1, 2))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_an_index_beyond_the_last_key_is_the_last_key(ntt, dev, ps, l):
    p = _pool(ntt, dev, ps)
    k, d = 5, M.OWN_D[ps]
    for batch in (7, max(_small_batches(ntt, ps))):
        ys, ahat, add = _operands(p, batch, k, l, NKEYS)
        raw = _keys("beyond", batch, NKEYS)
        want = _check(ntt, dev, ps, ys, ahat, add, raw, batch, (d,))
        # ... which is what the clamped indices give
        clamped = np.minimum(raw, NKEYS - 1).astype(np.uint32)
        assert np.array_equal(_check(ntt, dev, ps, ys, ahat, add, clamped, batch, (d,)), want)
        # keys = None with fewer keys than messages: messages >= 2 use key 1
        ys, ahat, add = _operands(p, batch, k, l, 2)
        want = _check(ntt, dev, ps, ys, ahat, add, None, batch, (d,))
        explicit = np.minimum(np.arange(batch), 1).astype(np.uint32)
        assert np.array_equal(_check(ntt, dev, ps, ys, ahat, add, explicit, batch, (d,)), want)


@pytest.mark.parametrize("variant", ("hi", "norms"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_one_output(ntt, dev, ps, variant):
    p = _pool(ntt, dev, ps)
    for batch, k, l in ((7, 5, 2), (3, 5, 1)):
        ys, ahat, add = _operands(p, batch, k, l, NKEYS)
        _check(ntt, dev, ps, ys, ahat, add, _keys("mixed", batch, NKEYS), batch, (M.OWN_D[ps],), (variant,))


@pytest.mark.parametrize("ps,k,above", (("ref", 4, 1025), ("p-I", 4, 1025), ("p-III", 5, 363)))
def test_just_above_the_split_threshold(ntt, dev, ps, k, above):
    """One work unit per message, the keys changing inside a workgroup's chunk."""
    assert ntt.mul_kl_shape(ps, 2)["split_max"] + 1 == above
    n, nkeys = ntt.param_info(ps)["n"], 4
    ys = [torch.empty(above * n, dtype=torch.int32, device=dev) for _ in range(2)]
    ahat = torch.empty((nkeys, k, 2, n), dtype=torch.int32, device=dev)
    add = torch.empty(above * k * n, dtype=torch.int32, device=dev)
    for i, t in enumerate((*ys, ahat, add)):
        ntt.fill_uniform(t, ps, 0x4E7AB + i)
    _check(ntt, dev, ps, ys, ahat, add, _keys("mixed", above, nkeys), above, (M.OWN_D[ps],))
    want = _check(ntt, dev, ps, ys, ahat, None, _keys("cycle", above, nkeys), above, (M.OWN_D[ps],))
    # keys = None with nkeys = batch, all keys' blocks equal to those of b % 4: the same products
    wide = ahat.repeat((above + nkeys - 1) // nkeys, 1, 1, 1)[:above].contiguous()
    _check(ntt, dev, ps, ys, wide, None, None, above, (M.OWN_D[ps],), want=want)


def test_keygen_form(ntt, dev):
    """l = 1, keys = None, nkeys = batch: t_b = a_b s_b + e_b, one a per key."""
    ps = "p-I"
    p = _pool(ntt, dev, ps)
    batch, k, n = 7, 4, p["n"]
    ys, ahat, add = _operands(p, batch, k, 1, batch)
    want = _check(ntt, dev, ps, ys, ahat, add, None, batch, (M.OWN_D[ps],))
    for b in range(batch):
        t = torch.empty(k * n, dtype=torch.int32, device=dev)
        ntt.poly_mul_ntt_k(t, ys[0].view(batch, n)[b].contiguous(), ahat[b].contiguous().view(-1), ps,
                           add=add.view(batch, k, n)[b].contiguous())
        assert np.array_equal(ntt.to_numpy_u32(t).reshape(k, n), want[b]), b


def test_keys_may_overlap_an_input(ntt, dev):
    """d_key inside y_1's buffer (legal: only the outputs keep clear of it)."""
    ps = "p-III"
    batch, k = 7, 5
    p = _pool(ntt, dev, ps)
    n = p["n"]
    ys, ahat, add = _operands(p, batch, k, 2, NKEYS)
    raw = _keys("mixed", batch, NKEYS)
    y1 = ys[1].clone()
    y1[:batch] = torch.from_numpy(raw.view(np.int32)).to(dev)   # y_1's first coefficients are the indices
    want = _want_w(ntt, dev, ps, [ys[0], y1], ahat, add, raw, batch)
    out = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
    ntt.poly_mul_ntt_kl_keyed(out, [ys[0], y1], ahat, y1[:batch], ps, add=add)
    assert np.array_equal(ntt.to_numpy_u32(out).reshape(batch, k, n), want)


def test_non_default_stream(ntt, dev):
    ps = "p-III"
    p = _pool(ntt, dev, ps)
    ys, ahat, add = _operands(p, 7, 5, 2, NKEYS)
    _check(ntt, dev, ps, ys, ahat, add, _keys("mixed", 7, NKEYS), 7, (M.OWN_D[ps],), stream=torch.cuda.Stream(device=dev))


def test_wrapper_checks(ntt, dev):
    ps = "p-III"
    p = _pool(ntt, dev, ps)
    n = p["n"]
    ys, ahat, add = _operands(p, 3, 5, 2, NKEYS)
    keys = ntt.from_numpy_u32(_keys("mixed", 3, NKEYS), dev)
    hi = torch.empty(15 * n, dtype=torch.uint8, device=dev)
    norms = torch.empty(30, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys, ps, 24)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys, ps, 24, hi=hi[:-16])
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys, ps, 24, norms=norms[:-2])
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat.view(-1), keys, ps, 24, norms=norms)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys[:-1], ps, 24, norms=norms)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys.cpu(), ps, 24, norms=norms)
    with pytest.raises(ValueError):
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, keys.to(torch.int64), ps, 24, norms=norms)
    with pytest.raises(ntt.NTTError):   # an output over the indices
        ntt.poly_mul_ntt_kl_round_keyed(ys, ahat, norms[:3], ps, 24, norms=norms)
    with pytest.raises(ntt.NTTError):   # an output over the later keys' blocks, clear of key 0's
        ntt.poly_mul_ntt_kl_keyed(ahat.view(-1)[-15 * n:], ys, ahat, keys, ps)
