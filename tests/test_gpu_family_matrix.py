"""Every kernel family of every entry point against the CPU oracle, bit-exact,
on edge, lazy ([q, 2q)), aliasing and tail contracts.

A call runs one of four kernel families (csrc/ntt_lat.hpp's switch table):
the radix-4, radix-8 or radix-16 one-polynomial-per-workgroup kernels or the
batch kernels.  Which one serves a batch comes from measured sweeps and moves
with them, so no batch here is written down: family_cells.cells() asks the
library (ntt_small_batch_max / ntt_small_batch_radix) for the smallest batch
that reaches each family and still leaves a ragged tail, one cell per
(parameter set, entry point, family).  tests/test_family_cells.py pins the
enumeration, the input classes and the oracle on them without a GPU.

Inputs are made on the device (ntt_fill_uniform, then row r rewritten by
class r mod K: the largest allowed input 2q-1 everywhere, canonical and lazy
coefficients mixed, all in [q, 2q), uniform, 0, q-1, single and alternating
2q-1, the reference's operand pattern); the host rebuilds any row by the same
rule.  Expected values are the oracle's on the input reduced mod q
(include/qtesla_ntt.h: inputs in [0, 2q) give the exact canonical result).
Per cell: the oracle on every row (sampled rows above 4096), every output
word below q over the whole batch, identical inputs give identical rows, the
inverse entry point of the same kind gives back the reduced input, inputs of
out-of-place calls are unchanged, and one polynomial of guard words before
and after every output buffer is untouched.
"""
import numpy as np
import pytest
import torch

import family_cells as fc
from family_check import GUARD, Ctx as _Ctx   # shared with test_gpu_family_probe.py

pytestmark = pytest.mark.gpu


def _library():
    """The product library at collection time (the cells parametrize the test)."""
    import os
    import ntt_amd
    if not os.path.exists(ntt_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ntt_amd.lib()
    return ntt_amd


def _params():
    out = []
    for c in fc.cells(_library()):
        marks = () if fc.reachable(c) else pytest.mark.skip(
            reason=f"first batch of the family, {c.batch}, is above MAX_TEST_BATCH; these kernels run in place, at "
                   f"small batches, in test_gpu_family_probe.py::test_batch_kernel_chunks")
        out.append(pytest.param(c, id=fc.cell_id(c), marks=marks))
    return out


_XFORM = {"fwd": "poly_ntt", "inv": "poly_invntt", "fwd_oop": "poly_ntt_oop", "inv_oop": "poly_invntt_oop",
          "fwd_br": "poly_ntt_bitrev", "inv_br": "poly_invntt_bitrev"}
_INVERSE = {"fwd": "inv", "inv": "fwd", "fwd_oop": "inv_oop", "inv_oop": "fwd_oop", "fwd_br": "inv_br", "inv_br": "fwd_br"}


def _transform_cell(c, ntt, oracle):
    ps, op = c.ps, c.op
    brv = ntt.tables(ps)["bitrev_tbl"]
    x, xr = c.operand(c.seed)
    want = {"fwd": lambda: oracle.poly_ntt(xr, ps), "inv": lambda: oracle.poly_invntt(xr, ps),
            "fwd_br": lambda: oracle.poly_ntt(xr, ps)[:, brv],
            "inv_br": lambda: oracle.poly_invntt(np.ascontiguousarray(xr[:, brv]), ps)}[op.replace("_oop", "")]()
    call = getattr(ntt, _XFORM[op])
    back = getattr(ntt, _XFORM[_INVERSE[op]])
    buf, y = c.guarded()
    if op in ("fwd", "inv"):
        y.copy_(x)
        call(y, ps)
        c.check(f"{op} in place", buf, y, want, [False])
        back(y, ps)
        assert bool((buf[:c.n] == GUARD).all()) and bool((buf[-c.n:] == GUARD).all())
        assert torch.equal(y, c.reduced(x)), f"{_INVERSE[op]}({op}(x)) != x mod q"
        return
    keep = x.clone()
    call(y, x, ps)
    assert torch.equal(x, keep), f"{op}: out-of-place call changed its input"
    c.check(f"{op} out of place", buf, y, want, [False])
    z = torch.empty_like(x)
    back(z, y, ps)
    assert torch.equal(z, c.reduced(x)), f"{_INVERSE[op]}({op}(x)) != x mod q"
    del z
    if op in ("fwd_br", "inv_br"):
        buf2, y2 = c.guarded()
        y2.copy_(x)
        call(y2, y2, ps)
        c.check(f"{op} with d_out == d_in", buf2, y2, want, [False])


def _product_cell(c, ntt, oracle):
    ps, op = c.ps, c.op
    a, ar = c.operand(c.seed)
    b, br = c.operand(c.seed + 1, second=True)
    if op == "mul":
        call = ntt.poly_mul
        want = oracle.poly_mul(ar, br, ps)
    else:
        # b is b-hat: any words below 2q; the product is a * INTT(b-hat mod q)
        call = ntt.poly_mul_ntt
        want = oracle.poly_mul(ar, oracle.poly_invntt(br, ps), ps)
    ka, kb = a.clone(), b.clone()
    buf, out = c.guarded()
    call(out, a, b, ps)
    assert torch.equal(a, ka) and torch.equal(b, kb), f"{op}: non-aliased call changed an input"
    c.check(f"{op} non-aliased", buf, out, want, [False, True])
    buf, out = c.guarded()
    out.copy_(a)
    call(out, out, b, ps)
    assert torch.equal(b, kb)
    c.check(f"{op} c aliasing a", buf, out, want, [False, True])
    buf, out = c.guarded()
    out.copy_(b)
    call(out, a, out, ps)
    assert torch.equal(a, ka)
    c.check(f"{op} c aliasing b", buf, out, want, [False, True])
    if op == "mul":
        buf, out = c.guarded()
        out.copy_(a)
        call(out, out, out, ps)
        c.check("mul a = b = c", buf, out, oracle.poly_mul(ar, ar, ps), [False])


@pytest.mark.parametrize("cell", _params())
def test_family_cell(ntt, oracle, dev, cell):
    assert ntt.small_batch_radix(cell.ps, cell.op, cell.batch) == cell.radix   # the batch selects the family
    c = _Ctx(ntt, oracle, dev, cell)
    if cell.op in _XFORM:
        _transform_cell(c, ntt, oracle)
    else:
        _product_cell(c, ntt, oracle)
    torch.cuda.synchronize()
    assert ntt.sync_expiries() == 0
