"""poly_mul_ntt_kl on the GPU, bit-exact against the CPU oracle:

    want[b, i] = (sum_j O.poly_mul(a_ij, y_j[b], ps) + e[b, i]) % q,   ahat = O.poly_ntt(a, ps)

Per parameter set one pool of operands (every y_j[b] and every a_ij
different, edge values 0 and q - 1 in every operand) and its products are
computed once and sliced by every small case.  The small batches straddle a
workgroup's tail (W waves per workgroup from ntt_mul_kl_shape, UPW polynomials
per wave), the odd ones leave the n = 1024 half-wave tail; every output buffer
sits between guard words.  Large batches are made on the device and compared
with the two poly_mul_ntt_k launches the fused one replaces, and row by row
with the oracle.
"""
import numpy as np
import pytest
import torch

from conftest import PARAM_SETS

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 8)
K_POOL = max(KS)
L = 2
GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
_POOL = {}


def _upw(n):
    return 2 if n == 1024 else 1   # polynomials per wave unit (Lane::UPW)


def _small_batches(ntt, ps):
    n = ntt.param_info(ps)["n"]
    full = ntt.mul_kl_shape(ps, L)["waves"] * _upw(n)
    return sorted({1, 2, 3, 7, full - 1, full, full + 1})


def _pool(ntt, O, ps):
    """Operands and products shared by the small cases of one parameter set:
    y [L, B, n], a / ahat [K_POOL, L, n], e [B, K_POOL, n],
    prod[j, b, i] = a_ij * y_j[b]."""
    if ps not in _POOL:
        info = ntt.param_info(ps)
        n, q = info["n"], info["q"]
        B = max(_small_batches(ntt, ps))
        rng = np.random.default_rng(0x5EED1 + n + q % 1000)
        y = rng.integers(0, q, (L, B, n), dtype=np.uint32)
        a = rng.integers(0, q, (K_POOL, L, n), dtype=np.uint32)
        e = rng.integers(0, q, (B, K_POOL, n), dtype=np.uint32)
        for arr in (y, a, e):   # edge values in every operand
            flat = arr.reshape(-1, n)
            flat[:, 0], flat[:, 1], flat[:, n - 1], flat[:, n - 2] = 0, q - 1, q - 1, 0
        flat = e.reshape(-1, n)
        flat[0, :], flat[-1, :] = q - 1, 0
        assert len({r.tobytes() for r in y.reshape(-1, n)}) == L * B
        assert len({r.tobytes() for r in a.reshape(-1, n)}) == K_POOL * L
        prod = np.stack([np.stack([O.poly_mul(np.broadcast_to(a[i, j], (B, n)), y[j], ps) for i in range(K_POOL)], axis=1)
                         for j in range(L)])
        ahat = O.poly_ntt(a.reshape(-1, n), ps).reshape(a.shape)
        for arr in (y, a, e, prod, ahat):
            arr.setflags(write=False)
        _POOL[ps] = dict(n=n, q=q, y=y, a=a, ahat=ahat, e=e, prod=prod)
    return _POOL[ps]


def _want(p, batch, k, with_add, js=(0, 1)):
    w = sum(p["prod"][j, :batch, :k].astype(np.uint64) for j in js)
    if with_add:
        w = w + p["e"][:batch, :k]
    return (w % p["q"]).astype(np.uint32)


def _guarded(dev, words, n):
    buf = torch.full((words + 2 * n,), GUARD, dtype=torch.int32, device=dev)
    return buf, buf[n:-n]


def _launch(ntt, dev, ps, tys, ta, B, k, n, e=None, inplace=False, stream=None):
    """One call on device operands; returns out as uint32 [B, k, n]."""
    buf, out = _guarded(dev, B * k * n, n)
    add = None
    if e is not None:
        if inplace:
            out.copy_(ntt.from_numpy_u32(np.array(e), dev).view(-1))
            add = out
        else:
            add = ntt.from_numpy_u32(np.array(e), dev)
    ntt.poly_mul_ntt_kl(out, tys, ta, ps, add=add, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert bool((buf[:n] == GUARD).all()) and bool((buf[-n:] == GUARD).all()), "store outside the output buffer"
    return ntt.to_numpy_u32(out).reshape(B, k, n)


def _run(ntt, dev, ps, ys, ahat, e=None, inplace=False, stream=None):
    """One call on host operands ys = l arrays [B, n], ahat [k, l, n], e
    [B, k, n] or None; returns (out as uint32 [B, k, n], device ys, device ahat)."""
    B, n = ys[0].shape
    k = ahat.shape[0]
    tys = [ntt.from_numpy_u32(np.array(y), dev) for y in ys]
    ta = ntt.from_numpy_u32(np.array(ahat), dev)
    return _launch(ntt, dev, ps, tys, ta, B, k, n, e, inplace, stream), tys, ta


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_exact_small_batches(ntt, oracle, dev, ps, k, with_add):
    p = _pool(ntt, oracle, ps)
    for batch in _small_batches(ntt, ps):
        got, _, _ = _run(ntt, dev, ps, [p["y"][0, :batch], p["y"][1, :batch]], p["ahat"][:k],
                         p["e"][:batch, :k] if with_add else None)
        assert np.array_equal(got, _want(p, batch, k, with_add)), f"{ps} batch {batch} k {k}"


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_operand_pairing(ntt, oracle, dev, ps):
    """y_1 = 0 leaves a_i0 * y_0, y_0 = 0 leaves a_i1 * y_1: a swapped j or a
    wrong [k][l][n] stride pairs an input with another polynomial."""
    p = _pool(ntt, oracle, ps)
    n, k = p["n"], 5
    for batch in (3, max(_small_batches(ntt, ps))):
        zero = np.zeros((batch, n), dtype=np.uint32)
        for j in (0, 1):
            ys = [zero, zero]
            ys[j] = p["y"][j, :batch]
            got, tys, ta = _run(ntt, dev, ps, ys, p["ahat"][:k])
            assert np.array_equal(got, _want(p, batch, k, False, js=(j,))), f"{ps} batch {batch} j {j}"
            one = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
            ntt.poly_mul_ntt_k(one, tys[j], ta.view(k, L, n)[:, j].contiguous().view(-1), ps)
            assert np.array_equal(got, ntt.to_numpy_u32(one).reshape(got.shape))


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_l1_is_poly_mul_ntt_k(ntt, oracle, dev, ps, with_add):
    p = _pool(ntt, oracle, ps)
    n, k = p["n"], 5
    for batch in (3, max(_small_batches(ntt, ps))):
        y, ahat = p["y"][0, :batch], np.ascontiguousarray(p["ahat"][:k, 0])
        e = p["e"][:batch, :k] if with_add else None
        got, tys, ta = _run(ntt, dev, ps, [y], ahat.reshape(k, 1, n), e)
        one = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
        ntt.poly_mul_ntt_k(one, tys[0], ta, ps, add=None if e is None else ntt.from_numpy_u32(np.array(e), dev))
        assert np.array_equal(got, ntt.to_numpy_u32(one).reshape(got.shape))
        assert np.array_equal(got, _want(p, batch, k, with_add, js=(0,)))


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_lazy_inputs(ntt, oracle, dev, ps):
    """+q on a random half of the entries of every operand (all < 2q): the
    result is unchanged and canonical."""
    p = _pool(ntt, oracle, ps)
    q, k, batch = p["q"], 5, 7
    rng = np.random.default_rng(78)

    def lazy(x):
        return (x + np.where(rng.integers(0, 2, x.shape) == 1, q, 0)).astype(np.uint32)

    ys, ahat, e = [lazy(p["y"][0, :batch]), lazy(p["y"][1, :batch])], lazy(p["ahat"][:k]), lazy(p["e"][:batch, :k])
    assert max(int(ys[0].max()), int(ys[1].max()), int(ahat.max()), int(e.max())) < 2 * q
    assert min(int(ys[0].max()), int(ys[1].max()), int(ahat.max()), int(e.max())) >= q
    got, _, _ = _run(ntt, dev, ps, ys, ahat, e)
    assert int(got.max()) < q
    assert np.array_equal(got, _want(p, batch, k, True))
    got, _, _ = _run(ntt, dev, ps, ys, ahat)
    assert np.array_equal(got, _want(p, batch, k, False))


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_worst_case_2q_minus_1(ntt, oracle, dev, ps):
    """Every entry of y_0, y_1, ahat and add is 2q - 1, the largest the
    contract admits: the case in which an unreduced sum of products, or an
    unreduced sum with the addend, overflows."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    k, batch = 8, 3
    top = np.uint32(2 * q - 1)
    y = np.full((batch, n), top, dtype=np.uint32)
    ahat = np.full((k, L, n), top, dtype=np.uint32)
    e = np.full((batch, k, n), top, dtype=np.uint32)
    a = oracle.poly_invntt((ahat % q).reshape(-1, n), ps).reshape(ahat.shape)
    yr = y % q
    want = sum(np.stack([oracle.poly_mul(np.broadcast_to(a[i, j], yr.shape), yr, ps) for i in range(k)], axis=1)
               .astype(np.uint64) for j in range(L))
    got, _, _ = _run(ntt, dev, ps, [y, y], ahat, e)
    assert np.array_equal(got, ((want + e % q) % q).astype(np.uint32))
    got, _, _ = _run(ntt, dev, ps, [y, y], ahat)
    assert np.array_equal(got, (want % q).astype(np.uint32))


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_inplace_accumulate(ntt, oracle, dev, ps):
    """add is out: equal to the out-of-place result; ys and ahat untouched."""
    p = _pool(ntt, oracle, ps)
    k = 5
    for batch in (3, max(_small_batches(ntt, ps))):
        ys, ahat, e = [p["y"][0, :batch], p["y"][1, :batch]], p["ahat"][:k], p["e"][:batch, :k]
        oop, _, _ = _run(ntt, dev, ps, ys, ahat, e)
        inp, tys, ta = _run(ntt, dev, ps, ys, ahat, e, inplace=True)
        assert np.array_equal(inp, oop)
        assert np.array_equal(inp, _want(p, batch, k, True))
        for j in range(L):
            assert np.array_equal(ntt.to_numpy_u32(tys[j]).reshape(ys[j].shape), ys[j])
        assert np.array_equal(ntt.to_numpy_u32(ta).reshape(ahat.shape), ahat)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_pointer_forms(ntt, oracle, dev, ps):
    """ys as two allocations, as two views of one allocation, and the same
    tensor twice (out = (a_i0 + a_i1) * y)."""
    p = _pool(ntt, oracle, ps)
    n, q, k, batch = p["n"], p["q"], 5, 7
    y, ahat, e = p["y"][:, :batch], p["ahat"][:k], p["e"][:batch, :k]
    want = _want(p, batch, k, True)
    sep, _, ta = _run(ntt, dev, ps, [y[0], y[1]], ahat, e)
    assert np.array_equal(sep, want)
    both = ntt.from_numpy_u32(np.ascontiguousarray(y), dev).view(L, batch * n)
    assert both[1].data_ptr() == both[0].data_ptr() + batch * n * 4
    views = _launch(ntt, dev, ps, [both[0], both[1]], ta, batch, k, n, e)
    assert np.array_equal(views, want)
    same = _launch(ntt, dev, ps, [both[0], both[0]], ta, batch, k, n, e)
    asum = ((p["a"][:k, 0].astype(np.uint64) + p["a"][:k, 1]) % q).astype(np.uint32)
    w = np.stack([oracle.poly_mul(np.broadcast_to(asum[i], y[0].shape), y[0], ps) for i in range(k)], axis=1)
    assert np.array_equal(same, ((w.astype(np.uint64) + e) % q).astype(np.uint32))
    # add may overlap an input: k = 1, add is y_0 itself (out = a_00 y_0 + a_01 y_1 + y_0)
    buf, out = _guarded(dev, batch * n, n)
    ntt.poly_mul_ntt_kl(out, [both[0], both[1]], ta.view(k, L, n)[:1].contiguous().view(-1), ps, add=both[0])
    assert bool((buf[:n] == GUARD).all()) and bool((buf[-n:] == GUARD).all())
    w = (p["prod"][0, :batch, 0].astype(np.uint64) + p["prod"][1, :batch, 0] + y[0]) % q
    assert np.array_equal(ntt.to_numpy_u32(out).reshape(batch, n), w.astype(np.uint32))


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_non_default_stream(ntt, oracle, dev, ps):
    p = _pool(ntt, oracle, ps)
    batch, k = 7, 5
    ys, ahat, e = [p["y"][0, :batch], p["y"][1, :batch]], p["ahat"][:k], p["e"][:batch, :k]
    base, _, _ = _run(ntt, dev, ps, ys, ahat, e)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    got, _, _ = _run(ntt, dev, ps, ys, ahat, e, stream=s)
    assert np.array_equal(got, base)
    assert np.array_equal(got, _want(p, batch, k, True))


@pytest.mark.parametrize("with_add", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("ps", PARAM_SETS)
def test_both_sides_of_the_launch_shape_switch(ntt, oracle, dev, ps, with_add):
    """One batch on each side of ntt_mul_kl_shape's split_max (rows spread
    over k workgroups up to it, one work unit per b above), k = 5, exact over
    the whole output."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    sw, k = ntt.mul_kl_shape(ps, L)["split_max"], 5
    a = oracle.fill_uniform(k * L, ps, 0x51DF, 0).reshape(k, L, n)
    ahat = oracle.poly_ntt(a.reshape(-1, n), ps).reshape(a.shape)
    for batch in ((sw, sw + 1) if sw else (4099,)):
        ys = [oracle.fill_uniform(batch, ps, 0x5EED + j, 0) for j in range(L)]
        e = oracle.fill_uniform(batch * k, ps, 0xADD, 0).reshape(batch, k, n) if with_add else None
        got, _, _ = _run(ntt, dev, ps, ys, ahat, e)
        want = sum(np.stack([oracle.poly_mul(np.broadcast_to(a[i, j], ys[j].shape), ys[j], ps) for i in range(k)], axis=1)
                   .astype(np.uint64) for j in range(L))
        if with_add:
            want = want + e
        assert np.array_equal(got, (want % q).astype(np.uint32)), f"{ps} batch {batch}"


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_chunk_loop(ntt, oracle, dev, ps):
    """A batch at which every workgroup walks its chunk of work units more
    than once (units >= 2 * waves * CUs * 4, the launch shape's workgroups per
    CU), k = 2, with an addend: the whole output equals the two poly_mul_ntt_k
    launches it replaces; sampled rows regenerated on the host."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    min_wg_per_cu = 4   # NTT_MIN_WG_PER_CU
    units = 2 * ntt.mul_kl_shape(ps, L)["waves"] * cus * min_wg_per_cu
    batch, k = units * _upw(n) + 1, 2
    seeds = (0xC0FFEE, 0xC0FFEF)
    tys = [torch.empty(batch * n, dtype=torch.int32, device=dev) for _ in range(L)]
    te = torch.empty(batch * k * n, dtype=torch.int32, device=dev)
    for t, seed in zip(tys, seeds):
        ntt.fill_uniform(t, ps, seed)
    ntt.fill_uniform(te, ps, 0xFACADE)
    a = oracle.fill_uniform(k * L, ps, 0xDECAF, 0).reshape(k, L, n)
    ahat = oracle.poly_ntt(a.reshape(-1, n), ps).reshape(a.shape)
    ta = ntt.from_numpy_u32(ahat, dev)
    out = torch.empty_like(te)
    ntt.poly_mul_ntt_kl(out, tys, ta, ps, add=te)
    two = torch.empty_like(te)
    ntt.poly_mul_ntt_k(two, tys[1], ntt.from_numpy_u32(np.ascontiguousarray(ahat[:, 1]), dev), ps, add=te)
    ntt.poly_mul_ntt_k(two, tys[0], ntt.from_numpy_u32(np.ascontiguousarray(ahat[:, 0]), dev), ps, add=two)
    assert torch.equal(out, two)
    rows = sorted({0, 1, batch - 2, batch - 1} | set(np.random.default_rng(batch).integers(0, batch, 25).tolist()))
    ri = torch.tensor(rows, device=dev)
    got = ntt.to_numpy_u32(out.view(batch, k, n)[ri])
    ys = [np.concatenate([oracle.fill_uniform(1, ps, seed, r) for r in rows]) for seed in seeds]
    es = np.stack([oracle.fill_uniform(k, ps, 0xFACADE, r * k) for r in rows])
    for i in range(k):
        want = sum(oracle.poly_mul(np.broadcast_to(a[i, j], ys[j].shape), ys[j], ps).astype(np.uint64) for j in range(L))
        assert np.array_equal(got[:, i], ((want + es[:, i]) % q).astype(np.uint32)), f"{ps} row {i}"


@pytest.mark.parametrize("ps,k,h", (("p-I", 4, 25), ("p-III", 5, 40)))
def test_verify_identity(ntt, oracle, dev, ps, k, h):
    """qTESLA verification on the library's launches: with t_i = a_i s + e_i
    and z = y + s c,  a_i z - t_i c = a_i y - e_i c.  c comes out of
    poly_scatter, the fused launch takes ys = (z, c) and rows (a_i-hat,
    q - t_i-hat)."""
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    batch = 5
    rng = np.random.default_rng(0x7E51A + n)

    def small(shape):
        return (rng.integers(-2, 3, shape) % q).astype(np.uint32)

    def mul(x, yb):   # x one polynomial, yb [batch, n]
        return oracle.poly_mul(np.broadcast_to(x, yb.shape), yb, ps).astype(np.uint64)

    a = rng.integers(0, q, (k, n), dtype=np.uint32)
    s, e = small((1, n)), small((k, n))
    t = ((mul(s[0], a) + e) % q).astype(np.uint32)
    # h distinct positions per polynomial, 0 and n - 1 among them, in random order
    pos = np.stack([rng.permutation(np.concatenate(([0, n - 1], 1 + rng.permutation(n - 2)[:h - 2])))
                    for _ in range(batch)]).astype(np.uint32)
    val = np.where(rng.integers(0, 2, (batch, h)) == 1, 1, q - 1).astype(np.uint32)
    c = np.zeros((batch, n), dtype=np.uint32)
    for b in range(batch):
        c[b, pos[b]] = val[b]
    tc = torch.full((batch * n,), GUARD, dtype=torch.int32, device=dev)
    ntt.poly_scatter(tc, ntt.from_numpy_u32(pos, dev), ntt.from_numpy_u32(val, dev), ps)
    assert np.array_equal(ntt.to_numpy_u32(tc).reshape(batch, n), c)
    y = rng.integers(0, q, (batch, n), dtype=np.uint32)
    z = ((y + mul(s[0], c)) % q).astype(np.uint32)
    rows = np.stack([oracle.poly_ntt(a, ps), q - oracle.poly_ntt(t, ps)], axis=1).astype(np.uint32)
    want = np.stack([(mul(a[i], y) + q - mul(e[i], c) % q) % q for i in range(k)], axis=1).astype(np.uint32)
    got = _launch(ntt, dev, ps, [ntt.from_numpy_u32(z, dev), tc], ntt.from_numpy_u32(rows, dev), batch, k, n)
    assert np.array_equal(got, want)
