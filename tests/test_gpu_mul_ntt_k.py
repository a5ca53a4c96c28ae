"""poly_mul_ntt_k on the GPU, bit-exact against the CPU oracle:

    want[b, i] = (O.poly_mul(a_i, y_b, ps) + e[b, i]) % q,   ahat = O.poly_ntt(a, ps)

Per parameter set one pool of operands (y_b all different, a_i all different,
edge values 0 and q - 1 in every operand) and its products are computed once
and sliced by every small case.  The small batches straddle a workgroup's
tail (W waves per workgroup from ntt_mul_k_shape, UPW polynomials per wave),
the odd ones leave the n = 1024 half-wave tail; every output buffer sits
between guard words.  Large batches are made on the device and compared with
poly_mul_ntt over a broadcast, or row by row with the oracle.
"""
import numpy as np
import pytest
import torch

from conftest import PARAM_SETS

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 8)
K_POOL = max(KS)
GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
_POOL = {}


def _upw(n):
    return 2 if n == 1024 else 1   # polynomials per wave unit (Lane::UPW)


def _small_batches(ntt, ps):
    n = ntt.param_info(ps)["n"]
    full = ntt.mul_k_shape(ps)["waves"] * _upw(n)
    return sorted({1, 2, 3, 7, full - 1, full, full + 1})


def _pool(ntt, O, ps):
    """Operands and products shared by the small cases of one parameter set:
    y [B, n], a / ahat [K_POOL, n], e [B, K_POOL, n], prod[b, i] = a_i * y_b."""
    if ps not in _POOL:
        info = ntt.param_info(ps)
        n, q = info["n"], info["q"]
        B = max(_small_batches(ntt, ps))
        rng = np.random.default_rng(0x5EED0 + n + q % 1000)
        y = rng.integers(0, q, (B, n), dtype=np.uint32)
        a = rng.integers(0, q, (K_POOL, n), dtype=np.uint32)
        e = rng.integers(0, q, (B, K_POOL, n), dtype=np.uint32)
        for arr in (y, a, e):   # edge values in every operand
            flat = arr.reshape(-1, n)
            flat[:, 0], flat[:, 1], flat[:, n - 1], flat[:, n - 2] = 0, q - 1, q - 1, 0
        flat = e.reshape(-1, n)
        flat[0, :], flat[-1, :] = q - 1, 0
        prod = np.stack([O.poly_mul(np.broadcast_to(a[i], (B, n)), y, ps) for i in range(K_POOL)], axis=1)
        for arr in (y, a, e, prod):
            arr.setflags(write=False)
        ahat = O.poly_ntt(a, ps)
        ahat.setflags(write=False)
        _POOL[ps] = dict(n=n, q=q, y=y, a=a, ahat=ahat, e=e, prod=prod)
    return _POOL[ps]


def _want(p, batch, k, with_add):
    w = p["prod"][:batch, :k].astype(np.uint64)
    if with_add:
        w = (w + p["e"][:batch, :k]) % p["q"]
    return w.astype(np.uint32)


def _guarded(dev, words, n):
    buf = torch.full((words + 2 * n,), GUARD, dtype=torch.int32, device=dev)
    return buf, buf[n:-n]


def _run(ntt, dev, ps, y, ahat, e=None, inplace=False, stream=None):
    """One call on host operands y [B, n], ahat [k, n], e [B, k, n] or None;
    returns (out as uint32 [B, k, n], device y, device ahat)."""
    n = y.shape[1]
    B, k = y.shape[0], ahat.shape[0]
    ty, ta = ntt.from_numpy_u32(np.array(y), dev), ntt.from_numpy_u32(np.array(ahat), dev)
    buf, out = _guarded(dev, B * k * n, n)
    add = None
    if e is not None:
        if inplace:
            out.copy_(ntt.from_numpy_u32(np.array(e), dev).view(-1))
            add = out
        else:
            add = ntt.from_numpy_u32(np.array(e), dev)
    ntt.poly_mul_ntt_k(out, ty, ta, ps, add=add, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert bool((buf[:n] == GUARD).all()) and bool((buf[-n:] == GUARD).all()), "store outside the output buffer"
    return ntt.to_numpy_u32(out).reshape(B, k, n), ty, ta


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_exact_small_batches(ntt, oracle, dev, ps, k, with_add):
    p = _pool(ntt, oracle, ps)
    for batch in _small_batches(ntt, ps):
        got, _, _ = _run(ntt, dev, ps, p["y"][:batch], p["ahat"][:k], p["e"][:batch, :k] if with_add else None)
        assert np.array_equal(got, _want(p, batch, k, with_add)), f"{ps} batch {batch} k {k}"


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_row_independence(ntt, oracle, dev, ps):
    """Every (b, i) cell of [batch][k][n] holds a_i * y_b: the a_i all differ
    and so do the y_b, so a row written at stride n instead of k*n (the
    n = 1024 half-wave pair at batch 2) lands in a cell that expects another
    product."""
    p = _pool(ntt, oracle, ps)
    k = 5
    assert len({p["a"][i].tobytes() for i in range(k)}) == k
    for batch in (2, 3):
        assert len({p["y"][b].tobytes() for b in range(batch)}) == batch
        got, _, _ = _run(ntt, dev, ps, p["y"][:batch], p["ahat"][:k])
        want = _want(p, batch, k, False)
        assert len({want[b, i].tobytes() for b in range(batch) for i in range(k)}) == batch * k
        assert np.array_equal(got, want)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_lazy_inputs(ntt, oracle, dev, ps):
    """+q on a random half of the entries of y, ahat and add (all < 2q): the
    result is unchanged and canonical."""
    p = _pool(ntt, oracle, ps)
    q, k, batch = p["q"], 5, 7
    rng = np.random.default_rng(77)

    def lazy(x):
        return (x + np.where(rng.integers(0, 2, x.shape) == 1, q, 0)).astype(np.uint32)

    y, ahat, e = lazy(p["y"][:batch]), lazy(p["ahat"][:k]), lazy(p["e"][:batch, :k])
    assert max(int(y.max()), int(ahat.max()), int(e.max())) < 2 * q and int(e.max()) >= q
    got, _, _ = _run(ntt, dev, ps, y, ahat, e)
    assert int(got.max()) < q
    assert np.array_equal(got, _want(p, batch, k, True))
    got, _, _ = _run(ntt, dev, ps, y, ahat)
    assert np.array_equal(got, _want(p, batch, k, False))


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_inplace_accumulate(ntt, oracle, dev, ps):
    """add is out: equal to the out-of-place result; y and ahat untouched."""
    p = _pool(ntt, oracle, ps)
    k = 5
    for batch in (3, max(_small_batches(ntt, ps))):
        y, ahat, e = p["y"][:batch], p["ahat"][:k], p["e"][:batch, :k]
        oop, _, _ = _run(ntt, dev, ps, y, ahat, e)
        inp, ty, ta = _run(ntt, dev, ps, y, ahat, e, inplace=True)
        assert np.array_equal(inp, oop)
        assert np.array_equal(inp, _want(p, batch, k, True))
        assert np.array_equal(ntt.to_numpy_u32(ty).reshape(y.shape), y)
        assert np.array_equal(ntt.to_numpy_u32(ta).reshape(ahat.shape), ahat)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_agrees_with_poly_mul_ntt(ntt, dev, ps):
    """Over a batch above poly_mul_ntt's small-batch switch, out[:, i] equals
    poly_mul_ntt(y, broadcast(ahat_i)) for every row."""
    n = ntt.param_info(ps)["n"]
    sw = ntt.small_batch_max(ps, "mul_ntt")
    batch, k = (2 * sw + 3) if sw else 4099, 5
    ty = torch.empty(batch * n, dtype=torch.int32, device=dev)
    ta = torch.empty(k * n, dtype=torch.int32, device=dev)
    ntt.fill_uniform(ty, ps, 0xA11CE)
    ntt.fill_uniform(ta, ps, 0xB0B)
    out = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
    ntt.poly_mul_ntt_k(out, ty, ta, ps)
    o3 = out.view(batch, k, n)
    c = torch.empty(batch * n, dtype=torch.int32, device=dev)
    for i in range(k):
        bc = ta.view(k, n)[i].expand(batch, n).contiguous()
        ntt.poly_mul_ntt(c, ty, bc.view(-1), ps)
        assert torch.equal(o3[:, i], c.view(batch, n)), f"{ps} row {i}"


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_chunk_loop(ntt, oracle, dev, ps):
    """A batch at which every workgroup walks its chunk of work units more
    than once (units >= 2 * waves * CUs * 4, the launch shape's workgroups per
    CU), k = 2; sampled rows regenerated on the host."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    min_wg_per_cu = 4   # NTT_MIN_WG_PER_CU
    units = 2 * ntt.mul_k_shape(ps)["waves"] * cus * min_wg_per_cu
    batch, k = units * _upw(n) + 1, 2
    ty = torch.empty(batch * n, dtype=torch.int32, device=dev)
    te = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
    ntt.fill_uniform(ty, ps, 0xC0FFEE)
    ntt.fill_uniform(te, ps, 0xFACADE)
    a = oracle.fill_uniform(k, ps, 0xDECAF, 0)
    ta = ntt.from_numpy_u32(oracle.poly_ntt(a, ps), dev)
    out = torch.empty_like(te)
    ntt.poly_mul_ntt_k(out, ty, ta, ps, add=te)
    rows = sorted({0, 1, batch // 2, batch - 2, batch - 1} |
                  set(np.random.default_rng(batch).integers(0, batch, 25).tolist()))
    ri = torch.tensor(rows, device=dev)
    got = ntt.to_numpy_u32(out.view(batch, k, n)[ri])
    ys = np.concatenate([oracle.fill_uniform(1, ps, 0xC0FFEE, r) for r in rows])
    es = np.stack([oracle.fill_uniform(k, ps, 0xFACADE, r * k) for r in rows])
    for i in range(k):
        want = (oracle.poly_mul(np.broadcast_to(a[i], ys.shape), ys, ps).astype(np.uint64) + es[:, i]) % q
        assert np.array_equal(got[:, i], want.astype(np.uint32)), f"{ps} row {i}"
    assert int(out.max()) < q and int(out.min()) >= 0


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_non_default_stream(ntt, oracle, dev, ps):
    p = _pool(ntt, oracle, ps)
    batch, k = 7, 5
    y, ahat, e = p["y"][:batch], p["ahat"][:k], p["e"][:batch, :k]
    base, _, _ = _run(ntt, dev, ps, y, ahat, e)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    got, _, _ = _run(ntt, dev, ps, y, ahat, e, stream=s)
    assert np.array_equal(got, base)
    assert np.array_equal(got, _want(p, batch, k, True))


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_both_sides_of_the_launch_shape_switch(ntt, oracle, dev, ps, with_add):
    """One batch on each side of ntt_mul_k_shape's split_max (rows spread over
    k workgroups up to it, one work unit per polynomial above), k = 5, exact
    over the whole output."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    sw, k = ntt.mul_k_shape(ps)["split_max"], 5
    a = oracle.fill_uniform(k, ps, 0x51DE, 0)
    ahat = oracle.poly_ntt(a, ps)
    for batch in ((sw, sw + 1) if sw else (4099,)):
        y = oracle.fill_uniform(batch, ps, 0x5EED, 0)
        e = oracle.fill_uniform(batch * k, ps, 0xADD, 0).reshape(batch, k, n) if with_add else None
        got, _, _ = _run(ntt, dev, ps, y, ahat, e)
        want = np.stack([oracle.poly_mul(np.broadcast_to(a[i], y.shape), y, ps) for i in range(k)], axis=1)
        if with_add:
            want = ((want.astype(np.uint64) + e) % q).astype(np.uint32)
        assert np.array_equal(got, want), f"{ps} batch {batch}"
