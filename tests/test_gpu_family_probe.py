"""Every compiled transform and product kernel against the CPU oracle,
bit-exact, whether or not the measured switch table routes any batch to it.

csrc/ntt_kernels.hip instantiates, per parameter set, transform kind and
product, the radix-4 / 8 / 16 one-polynomial-per-workgroup kernels and the
batch kernels; the entry points run the one kLatTier (csrc/ntt_lat.hpp)
selects.  At the table this was written against, the entry points reach 29 of
the 60 one-polynomial transform instantiations (counted from
ntt_small_batch_radix by test_family_probe_abi.py::test_routed_instantiations),
never run k_ntt_fwd / k_ntt_inv in place at n = 1024 below 2^26 polynomials,
and walk the batch kernels' chunk loop at the lengths the device's CU count
gives.  The test-only library lib/libqtesla_ntt_family.so
(tools/family_probe.hip: the product's headers and launch lines, with the
family and the chunk length named by the caller) reaches all of them:

  test_parity              the probe is the product: for every reachable cell
                           of family_cells.cells(), the probe with the cell's
                           family and the product's chunk rule gives the entry
                           point's bytes, and its shapes are what the ABI reports
  test_one_polynomial      all (ps, kind, radix) and k_poly_mul_lat, batches 3
                           and 23 (two rounds of the eleven input classes and
                           one more; these kernels index by blockIdx.x only)
  test_batch_kernel_chunks every batch kernel at chunk 1, 2, 3, 5 and 16, at
                           the batches of family_probe.walk_batches: two full
                           workgroups and one that stops mid-chunk in a pass
                           with idle waves (an odd batch at n = 1024: the last
                           unit holds one polynomial), two full ones, one unit
  test_side_stream         one case of each on a stream of their own

Inputs are family_cells' (ntt_fill_uniform, then row r rewritten by class
r mod 11), rebuilt on the host; row r of an operand does not depend on the
batch, so the oracle runs once per (ps, op) on the largest batch and is
sliced.  Per output buffer, family_check.Ctx.check: guard polynomials on both
sides untouched, every word below q, every row the oracle's, identical inputs
give identical rows.  Transforms run out of place (input unchanged) and in
place; products non-aliased, c = a, c = b and, for mul, a = b = c.
"""
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

import family_cells as fc
import family_probe as fp
from family_check import GUARD, Ctx

pytestmark = pytest.mark.gpu

Cell = namedtuple("Cell", "ps op batch")
SEED = 0xFA3117            # first operand's fill seed (second: SEED + 1), the same for every batch
SMALL = (3, 23)            # test_one_polynomial's batches


def _library():
    """The product library at collection time (family_cells.cells parametrizes test_parity)."""
    import os
    import ntt_amd
    if not os.path.exists(ntt_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ntt_amd.lib()
    return ntt_amd


@pytest.fixture(scope="module")
def probe(ntt):
    return fp.load(ntt)


# ---------------------------------------------------------------- the oracle, once per (ps, op)
_ROWS = {}    # ps -> number of rows the references cover
_WANT = {}    # (ps, op) -> [rows, n] uint32


def _rows(probe, ntt, ps):
    """The largest batch any test here runs at `ps`."""
    if ps not in _ROWS:
        m = max(SMALL)
        for op in fp.OPS:
            for c in fp.CHUNKS:
                rc, sh = fp.shape(probe, 0, op, ntt.PARAM_SETS[ps], 1, chunk=c)
                assert rc == ntt.NTT_OK
                m = max(m, max(b for b, _ in fp.walk_batches(sh["per"], fp.upw(ps), c)))
        _ROWS[ps] = m
    return _ROWS[ps]


def _want(probe, ntt, oracle, ps, op, batch):
    """Rows 0 .. batch - 1 of the oracle's result for `op` ("mul_sq": a = b = c)."""
    if (ps, op) not in _WANT:
        rows = _rows(probe, ntt, ps)
        q = oracle.params(ps)["q"]
        idx = np.arange(rows)
        xr = fc.reduce_np(fc.host_rows(oracle, ps, SEED, idx, rows), q)
        if op in fp.PRODUCTS:
            br = fc.reduce_np(fc.host_rows(oracle, ps, SEED + 1, idx, rows, second=True), q)
        brv = ntt.tables(ps)["bitrev_tbl"]
        _WANT[(ps, op)] = {
            "fwd": lambda: oracle.poly_ntt(xr, ps),
            "inv": lambda: oracle.poly_invntt(xr, ps),
            "fwd_br": lambda: oracle.poly_ntt(xr, ps)[:, brv],
            "inv_br": lambda: oracle.poly_invntt(np.ascontiguousarray(xr[:, brv]), ps),
            "mul": lambda: oracle.poly_mul(xr, br, ps),
            # b is b-hat: any words below 2q; the product is a * INTT(b-hat mod q)
            "mul_ntt": lambda: oracle.poly_mul(xr, oracle.poly_invntt(br, ps), ps),
            "mul_sq": lambda: oracle.poly_mul(xr, xr, ps),
        }[op]()
    assert batch <= len(_WANT[(ps, op)])
    return _WANT[(ps, op)][:batch]


# ---------------------------------------------------------------- one launch configuration, every aliasing
def _transform(probe, ntt, oracle, dev, ps, kind, family, chunk, batch):
    c = Ctx(ntt, oracle, dev, Cell(ps, kind, batch), seed=SEED)
    what = f"{ps} {kind} {fp.family_id(family)} chunk {chunk} batch {batch}"
    x, _ = c.operand(SEED)
    keep = x.clone()
    if kind == "bitrev":
        # out[t] = in[brv(t)] on any 32-bit words: the lazy inputs come out as they went in
        brv = torch.as_tensor(ntt.tables(ps)["bitrev_tbl"].astype(np.int64), device=dev)
        want = keep.view(batch, c.n)[:, brv].contiguous().view(-1)
        for inplace in (False, True):
            buf, y = c.guarded()
            if inplace:
                y.copy_(x)
            assert fp.xform(probe, ntt, family, kind, ps, y, y if inplace else x, chunk) == ntt.NTT_OK
            assert torch.equal(x, keep), f"{what}: out-of-place call changed its input"
            assert bool((buf[:c.n] == GUARD).all()) and bool((buf[-c.n:] == GUARD).all()), f"{what}: store outside the buffer"
            assert torch.equal(y, want), f"{what} {'in place' if inplace else 'out of place'}: not the permutation"
        return
    want = _want(probe, ntt, oracle, ps, kind, batch)
    buf, y = c.guarded()
    assert fp.xform(probe, ntt, family, kind, ps, y, x, chunk) == ntt.NTT_OK
    assert torch.equal(x, keep), f"{what}: out-of-place call changed its input"
    c.check(f"{what} out of place", buf, y, want, [False])
    buf, y = c.guarded()
    y.copy_(x)
    assert fp.xform(probe, ntt, family, kind, ps, y, y, chunk) == ntt.NTT_OK
    c.check(f"{what} in place (d_out == d_in)", buf, y, want, [False])


def _product(probe, ntt, oracle, dev, ps, op, family, chunk, batch):
    c = Ctx(ntt, oracle, dev, Cell(ps, op, batch), seed=SEED)
    what = f"{ps} {op} {fp.family_id(family)} chunk {chunk} batch {batch}"
    a, _ = c.operand(SEED)
    b, _ = c.operand(SEED + 1, second=True)
    want = _want(probe, ntt, oracle, ps, op, batch)
    ka, kb = a.clone(), b.clone()

    def call(out, x, y):
        assert fp.mul(probe, ntt, family, op, ps, out, x, y, chunk) == ntt.NTT_OK

    buf, out = c.guarded()
    call(out, a, b)
    assert torch.equal(a, ka) and torch.equal(b, kb), f"{what}: non-aliased call changed an input"
    c.check(f"{what} non-aliased", buf, out, want, [False, True])
    buf, out = c.guarded()
    out.copy_(a)
    call(out, out, b)
    assert torch.equal(b, kb)
    c.check(f"{what} c aliasing a", buf, out, want, [False, True])
    buf, out = c.guarded()
    out.copy_(b)
    call(out, a, out)
    assert torch.equal(a, ka)
    c.check(f"{what} c aliasing b", buf, out, want, [False, True])
    if op == "mul":
        buf, out = c.guarded()
        out.copy_(a)
        call(out, out, out)
        c.check(f"{what} a = b = c", buf, out, _want(probe, ntt, oracle, ps, "mul_sq", batch), [False])


def _run(probe, ntt, oracle, dev, ps, op, family, chunk, batch):
    (_product if op in fp.PRODUCTS else _transform)(probe, ntt, oracle, dev, ps, op, family, chunk, batch)


# ---------------------------------------------------------------- a. parity with the entry points
_ENTRY = {"fwd": "poly_ntt", "inv": "poly_invntt", "fwd_oop": "poly_ntt_oop", "inv_oop": "poly_invntt_oop",
          "fwd_br": "poly_ntt_bitrev", "inv_br": "poly_invntt_bitrev", "mul": "poly_mul", "mul_ntt": "poly_mul_ntt"}
CLASSES_UP_TO = 1 << 16   # above it the operands are the plain fill (the class rule indexes the whole tensor)


def _parity_params():
    return [pytest.param(c, id=fc.cell_id(c)) for c in fc.cells(_library()) if fc.reachable(c)]


@pytest.mark.parametrize("cell", _parity_params())
def test_parity(ntt, probe, dev, cell):
    """The probe with the cell's family and chunk 0 gives the entry point's bytes."""
    ps, op, batch = cell.ps, cell.op, cell.batch
    assert ntt.small_batch_radix(ps, op, batch) == cell.radix
    family = cell.radix.bit_length() - 1 if cell.radix else 0
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]

    def operand(seed, second=False):
        t = torch.empty(batch * n, dtype=torch.int32, device=dev)
        ntt.fill_uniform(t, ps, seed)
        if batch <= CLASSES_UP_TO:
            fc.apply_classes_torch(t.view(batch, n), q, second)
        return t

    x = operand(SEED)
    entry = getattr(ntt, _ENTRY[op])
    kind = op.replace("_oop", "")
    if op in ("fwd", "inv"):            # in place
        mine = x.clone()
        entry(x, ps)
        assert fp.xform(probe, ntt, family, kind, ps, mine, mine) == ntt.NTT_OK
        theirs = x
    elif op in fp.PRODUCTS:
        b = operand(SEED + 1, second=True)
        theirs, mine = torch.empty_like(x), torch.empty_like(x)
        entry(theirs, x, b, ps)
        assert fp.mul(probe, ntt, family, op, ps, mine, x, b) == ntt.NTT_OK
    else:
        theirs, mine = torch.empty_like(x), torch.empty_like(x)
        entry(theirs, x, ps)
        assert fp.xform(probe, ntt, family, kind, ps, mine, x) == ntt.NTT_OK
    assert torch.equal(mine, theirs), f"{fc.cell_id(cell)} batch {batch}: the probe's bytes differ from {_ENTRY[op]}'s"
    assert ntt.sync_expiries() == 0 and fp.sync_expiries(probe) == 0


def test_parity_shapes(ntt, probe, dev):
    """What the ABI reports of a launch is what the probe launches: the
    constants in ntt_build_info(), ntt_small_batch_radix's family for every
    cell, and launch_shape() at this device's CU count."""
    info = ntt.build_info()
    got = {k: int(v) for k, v in re.findall(r"\b(wg|mul_wg|ppw<|min_wg/cu)=(\d+)", info)}
    k = fp.consts(probe)
    assert got["min_wg/cu"] == k["min_wg_per_cu"] and got["ppw<"] == k["ppw_max"] == fp.CHUNK_MAX
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for ps in fp.ALL_SETS:
        psi = ntt.PARAM_SETS[ps]
        for op in fp.OPS:
            for batch in (1, 7, 2817, 131073, 1 << 20):
                rc, sh = fp.shape(probe, 0, op, psi, batch)
                assert rc == ntt.NTT_OK and sh == fp.expected_shape(ps, op, batch, cus), (ps, op, batch, sh, cus)
        if ps in fp.PARAM_SETS:
            assert fp.shape(probe, 0, "fwd", psi, 7)[1]["block"] == got["wg"]
            assert fp.shape(probe, 0, "mul_ntt", psi, 7)[1]["block"] == got["mul_wg"]
    for c in fc.cells(ntt):
        if c.radix:
            rc, sh = fp.shape(probe, c.radix.bit_length() - 1, c.op.replace("_oop", ""), ntt.PARAM_SETS[c.ps], c.batch)
            n = ntt.param_info(c.ps)["n"]
            threads = n // c.radix if (n, c.radix) != (8192, 4) else 1024
            assert rc == ntt.NTT_OK and sh == dict(grid=c.batch, block=threads, chunk=1, per=1), c


# ---------------------------------------------------------------- b. every one-polynomial instantiation
def _one_poly_params():
    inst = sorted((i for i in fp.instantiations() if i[2]), key=lambda i: i[2])   # one radix after the other
    return [pytest.param(*i, id=f"{i[0]}-{i[1]}-{fp.family_id(i[2])}") for i in inst]


@pytest.mark.parametrize("ps,op,family", _one_poly_params())
def test_one_polynomial(ntt, probe, oracle, dev, ps, op, family):
    for batch in SMALL:
        _run(probe, ntt, oracle, dev, ps, op, family, 0, batch)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- c. the batch kernels' chunk walk
def _chunk_params():
    return [pytest.param(ps, op, c, id=f"{ps}-{op}-batch-chunk{c}")
            for ps, op, f in fp.instantiations() if not f for c in fp.CHUNKS]


@pytest.mark.parametrize("ps,op,chunk", _chunk_params())
def test_batch_kernel_chunks(ntt, probe, oracle, dev, ps, op, chunk):
    rc, sh = fp.shape(probe, 0, op, ntt.PARAM_SETS[ps], 1, chunk=chunk)
    assert rc == ntt.NTT_OK
    for batch, grid in fp.walk_batches(sh["per"], fp.upw(ps), chunk):
        rc, at = fp.shape(probe, 0, op, ntt.PARAM_SETS[ps], batch, chunk=chunk)
        assert rc == ntt.NTT_OK and at["grid"] == grid, (batch, at)
        _run(probe, ntt, oracle, dev, ps, op, 0, chunk, batch)
    torch.cuda.synchronize()
    assert fp.sync_expiries(probe) == 0   # the n = 8192 products' slot barriers never expired


# ---------------------------------------------------------------- d. on a stream of their own
@pytest.mark.parametrize("ps,op,family,chunk,batch", [("p-III", "inv_br", 3, 0, 23), ("p-I", "fwd", 0, 3, None),
                                                      ("p-III-8192", "mul", 0, 2, None)],
                         ids=["p-III-inv_br-radix8", "p-I-fwd-batch-chunk3", "p-III-8192-mul-batch-chunk2"])
def test_side_stream(ntt, probe, oracle, dev, ps, op, family, chunk, batch):
    """The launches go to the stream they are given: everything (fills, the
    probe's launches, the checks) runs on a side stream while the default
    stream is idle; the wrappers pass the current stream."""
    if batch is None:
        rc, sh = fp.shape(probe, 0, op, ntt.PARAM_SETS[ps], 1, chunk=chunk)
        assert rc == ntt.NTT_OK
        batch = fp.walk_batches(sh["per"], fp.upw(ps), chunk)[0][0]
    _want(probe, ntt, oracle, ps, op, batch)   # the oracle's (host) work first
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        assert ntt._stream(None, dev) == s.cuda_stream
        _run(probe, ntt, oracle, dev, ps, op, family, chunk, batch)
    s.synchronize()
    assert fp.sync_expiries(probe) == 0
