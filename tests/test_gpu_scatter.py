"""poly_scatter on the GPU, exact against a numpy scatter: all five parameter
sets, h from one entry to a full permutation, values 0, q - 1 and lazy ones
in [q, 2q), some positions >= n (ignored), the output prefilled with garbage
(every word must be written) and held between guard words."""
import numpy as np
import pytest
import torch

from conftest import LARGE_SETS, PARAM_SETS

pytestmark = pytest.mark.gpu

GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))
GARBAGE = int(np.uint32(0xDEADBEEF).view(np.int32))


@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("ps", PARAM_SETS + LARGE_SETS)
def test_scatter_exact(ntt, dev, ps, batch):
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(0x5CA77E4 + n + batch)
    for h in (1, 25, 40, n):
        # distinct in-range positions; h = n: a full permutation
        pos = np.stack([rng.permutation(n)[:h] for _ in range(batch)]).astype(np.uint32)
        val = rng.integers(0, 2 * q, (batch, h), dtype=np.uint32)
        val[:, 0] = q - 1
        if h > 1:
            val[:, 1::7] = 0
            val[:, 2::7] = rng.integers(q, 2 * q, val[:, 2::7].shape, dtype=np.uint32)   # lazy
            # every 5th entry out of range: n, just above it, and the largest 32-bit values
            bad = np.array([n, n + 1, 2 * n, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
            pos[:, 3::5] = rng.choice(bad, pos[:, 3::5].shape)
        want = np.zeros((batch, n), dtype=np.uint32)
        for b in range(batch):
            ok = pos[b] < n
            want[b, pos[b][ok]] = val[b][ok] % q
        buf = torch.full((batch * n + 2 * n,), GUARD, dtype=torch.int32, device=dev)
        out = buf[n:-n]
        out.fill_(GARBAGE)
        tp, tv = ntt.from_numpy_u32(pos, dev), ntt.from_numpy_u32(val, dev)
        ntt.poly_scatter(out, tp, tv, ps)
        assert np.array_equal(ntt.to_numpy_u32(out).reshape(batch, n), want), f"{ps} batch {batch} h {h}"
        assert bool((buf[:n] == GUARD).all()) and bool((buf[-n:] == GUARD).all()), "store outside the output buffer"
        assert np.array_equal(ntt.to_numpy_u32(tp), pos) and np.array_equal(ntt.to_numpy_u32(tv), val)


def test_scatter_non_default_stream(ntt, dev):
    ps, batch, h = "p-III", 3, 40
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    rng = np.random.default_rng(41)
    pos = np.stack([rng.permutation(n)[:h] for _ in range(batch)]).astype(np.uint32)
    val = np.where(rng.integers(0, 2, (batch, h)) == 1, 1, q - 1).astype(np.uint32)
    want = np.zeros((batch, n), dtype=np.uint32)
    for b in range(batch):
        want[b, pos[b]] = val[b]
    out = torch.full((batch * n,), GARBAGE, dtype=torch.int32, device=dev)
    tp, tv = ntt.from_numpy_u32(pos, dev), ntt.from_numpy_u32(val, dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    ntt.poly_scatter(out, tp, tv, ps, stream=s)
    s.synchronize()
    assert np.array_equal(ntt.to_numpy_u32(out).reshape(batch, n), want)
