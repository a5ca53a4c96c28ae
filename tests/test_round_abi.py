"""poly_round / poly_mul_ntt_kl_round without a GPU: the numpy model against
qTESLA's two written forms of the rounding, and both entry points' argument
validation with fake pointers (validation fails before any GPU work)."""
import ctypes

import numpy as np
import pytest

import round_model as M

SETS = ("ref", "p-I", "p-III", "p-III-4096", "p-III-8192")
MIN_D = {"ref": 16, "p-I": 21, "p-III": 22, "p-III-4096": 22, "p-III-8192": 22}
# the issue's table: hi range at the smallest allowed d and at the set's own d
HMAX = {"ref": (64, 1), "p-I": (82, 41), "p-III": (102, 26), "p-III-4096": (102, 26), "p-III-8192": (102, 26)}


@pytest.mark.parametrize("ps", SETS)
def test_model_equals_both_qtesla_forms(ntt, ps):
    q = ntt.param_info(ps)["q"]
    rng = np.random.default_rng(q % 9973)
    for d in (MIN_D[ps], M.OWN_D[ps]):
        x = np.concatenate([M.edge_values(q, d), rng.integers(0, 2 * q, 1 << 14, dtype=np.uint32)])
        c, lo, hi = M.split(x, q, d)
        assert np.array_equal(hi, M.hi_shift_form(x, q, d))
        assert np.array_equal(hi, M.hi_mask_form(x, q, d))
        assert np.array_equal(hi * (1 << d) + lo, c)
        assert np.all(lo > -(1 << (d - 1))) and np.all(lo <= (1 << (d - 1)))
        assert np.all(np.abs(c) <= (q - 1) // 2)
        assert np.array_equal(c % q, x.astype(np.int64) % q)
        assert hi.max() <= M.hmax(q, d) and hi.min() >= -M.hmax(q, d) - 1


@pytest.mark.parametrize("ps", SETS)
def test_hmax_table(ntt, ps):
    q = ntt.param_info(ps)["q"]
    assert M.min_d(q) == MIN_D[ps]
    assert (M.hmax(q, MIN_D[ps]), M.hmax(q, M.OWN_D[ps])) == HMAX[ps]
    assert M.hmax(q, MIN_D[ps] - 1) > 127
    # the bound is attained: x = (q-1)/2 has the largest hi
    assert int(M.split(np.array([(q - 1) // 2]), q, MIN_D[ps])[2][0]) == M.hmax(q, MIN_D[ps])


def test_python_constants_unchanged(ntt):
    assert "round" not in ntt.SWITCH_OPS and len(ntt.PARAM_SETS) == 5


FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap


def _bufs():
    return dict(hi=FAKE, norms=FAKE + FAR, w=FAKE + 2 * FAR)


@pytest.mark.parametrize("ps", SETS)
def test_poly_round_validation(ntt, ps):
    L = ntt.lib()
    i, n = ntt.PARAM_SETS[ps], ntt.param_info(ps)["n"]
    own, lowd = M.OWN_D[ps], MIN_D[ps] - 1
    b = _bufs()
    hi, norms, w = b["hi"], b["norms"], b["w"]
    E = ntt
    assert L.poly_round(hi, norms, w, 1, 0, i, None) == E.NTT_ERR_PARAM
    assert L.poly_round(hi, norms, w, 1, 31, i, None) == E.NTT_ERR_PARAM
    assert L.poly_round(hi, norms, w, 1, own, 5, None) == E.NTT_ERR_PARAM
    assert L.poly_round(hi, norms, w, 1, lowd, i, None) == E.NTT_ERR_PARAM
    assert L.poly_round(hi, None, w, 1, lowd, i, None) == E.NTT_ERR_PARAM
    # norms alone: any d in 1 .. 30 is accepted, so the call gets as far as the next check
    # (every call here must fail validation: a valid one would launch on fake pointers)
    assert L.poly_round(None, norms, w + 4, 1, lowd, i, None) == E.NTT_ERR_ALIGN
    assert L.poly_round(None, None, w, 1, own, i, None) == E.NTT_ERR_NULL
    assert L.poly_round(hi, norms, None, 1, own, i, None) == E.NTT_ERR_NULL
    assert L.poly_round(hi, norms, w + 4, 1, own, i, None) == E.NTT_ERR_ALIGN
    assert L.poly_round(hi + 4, norms, w, 1, own, i, None) == E.NTT_ERR_ALIGN
    assert L.poly_round(hi, norms + 4, w, 1, own, i, None) == E.NTT_ERR_ALIGN
    assert L.poly_round(hi, norms, w, 1 << 31, own, i, None) == E.NTT_ERR_SIZE
    batch = 3
    wb, hb, nb = batch * n * 4, batch * n, batch * 8
    # each output against the input, by one word at either end, and against each other
    assert L.poly_round(w + wb - 16, norms, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(w - hb + 16, norms, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(hi, w + wb - 8, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(hi, w - nb + 8, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(hi, hi + hb - 8, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(hi, hi - nb + 8, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(hi, hi, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    assert L.poly_round(w, None, w, batch, own, i, None) == E.NTT_ERR_ALIAS
    for args in ((hi, norms, w), (None, None, None), (hi + 1, norms + 1, w + 1)):
        assert L.poly_round(*args, 0, own, i, None) == E.NTT_OK   # empty batch is a no-op
    assert L.poly_round(hi, norms, w, 0, 0, i, None) == E.NTT_ERR_PARAM


@pytest.mark.parametrize("ps", SETS)
def test_poly_round_first_defect_decides(ntt, ps):
    """Two defects at once (the order is ABI): PARAM, NULL of w, SIZE, then the
    outputs (both NULL, d against hi, alignment, hi / norms overlap), then w's
    alignment and the outputs against w."""
    L = ntt.lib()
    E = ntt
    i, n = ntt.PARAM_SETS[ps], ntt.param_info(ps)["n"]
    own, lowd = M.OWN_D[ps], MIN_D[ps] - 1
    b = _bufs()
    hi, norms, w = b["hi"], b["norms"], b["w"]
    assert L.poly_round(hi + 4, norms, None, 1, own, i, None) == E.NTT_ERR_NULL
    assert L.poly_round(hi + 4, norms, w, 1 << 31, own, i, None) == E.NTT_ERR_SIZE
    assert L.poly_round(None, None, w + 4, 1 << 31, own, i, None) == E.NTT_ERR_SIZE
    assert L.poly_round(None, None, w + 4, 1, own, i, None) == E.NTT_ERR_NULL
    assert L.poly_round(hi + 4, norms, w, 1, lowd, i, None) == E.NTT_ERR_PARAM     # d before the outputs' alignment
    assert L.poly_round(hi + 4, norms, None, 1, 31, i, None) == E.NTT_ERR_PARAM
    assert L.poly_round(hi + 4, hi, w, 3, own, i, None) == E.NTT_ERR_ALIGN         # alignment before the outputs' overlap
    assert L.poly_round(hi, hi, w + 4, 3, own, i, None) == E.NTT_ERR_ALIAS         # the outputs' overlap before w's alignment
    assert L.poly_round(None, w + 8, w + 8, 3, own, i, None) == E.NTT_ERR_ALIGN    # w's alignment before its aliasing


def _ys(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


@pytest.mark.parametrize("ps", ("ref", "p-I", "p-III"))
def test_fused_first_defect_decides(ntt, ps):
    """poly_mul_ntt_kl_round follows poly_round's order, not poly_mul_ntt_kl's:
    the inputs' NULLs, SIZE, the outputs' checks, and only then the inputs'
    alignment and the overlaps."""
    L = ntt.lib()
    E = ntt
    i, n = ntt.PARAM_SETS[ps], ntt.param_info(ps)["n"]
    own, lowd = M.OWN_D[ps], MIN_D[ps] - 1
    hi, norms = FAKE, FAKE + FAR
    y0, y1, ahat, add = (FAKE + j * FAR for j in range(2, 6))
    bad = _ys(y0, y1 + 2)

    def call(hi=hi, norms=norms, ys=bad, ahat=ahat, add=add, batch=3, k=5, l=2, d=own, ps=i):
        return L.poly_mul_ntt_kl_round(hi, norms, ys, ahat, add, batch, k, l, d, ps, None)

    assert call() == E.NTT_ERR_ALIGN                         # y_1 misaligned, nothing else
    assert call(hi=None, norms=None) == E.NTT_ERR_NULL
    assert call(hi=hi + 4) == E.NTT_ERR_ALIGN
    assert call(d=lowd) == E.NTT_ERR_PARAM                   # d too small for hi: before y_1's alignment
    assert call(d=lowd, hi=None) == E.NTT_ERR_ALIGN          # ... accepted without hi: y_1's alignment
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    assert call(batch=1 << 31, hi=None, norms=None) == E.NTT_ERR_SIZE
    assert call(ahat=None, hi=None, norms=None) == E.NTT_ERR_NULL
    assert call(norms=hi) == E.NTT_ERR_ALIAS                 # the outputs' overlap before y_1's alignment
    assert call(hi=y0) == E.NTT_ERR_ALIGN                    # y_1's alignment before an output over an input
    assert call(k=9, hi=None, norms=None) == E.NTT_ERR_PARAM
    assert call(ys=_ys(y0 + 2, None), l=1, hi=None, norms=None) == E.NTT_ERR_NULL   # l = 1 reads d_y[0] only
    assert call(ys=_ys(y0 + 2, None), l=1) == E.NTT_ERR_ALIGN


@pytest.mark.parametrize("ps", ("ref", "p-I", "p-III"))
def test_fused_validation(ntt, ps):
    L = ntt.lib()
    E = ntt
    i, n = ntt.PARAM_SETS[ps], ntt.param_info(ps)["n"]
    own, lowd = M.OWN_D[ps], MIN_D[ps] - 1
    hi, norms = FAKE, FAKE + FAR
    y0, y1, ahat, add = (FAKE + j * FAR for j in range(2, 6))
    ys = _ys(y0, y1)

    def call(hi=hi, norms=norms, ys=ys, ahat=ahat, add=add, batch=3, k=5, l=2, d=own, ps=i):
        return L.poly_mul_ntt_kl_round(hi, norms, ys, ahat, add, batch, k, l, d, ps, None)

    assert call(d=0) == E.NTT_ERR_PARAM
    assert call(d=31) == E.NTT_ERR_PARAM
    assert call(d=lowd) == E.NTT_ERR_PARAM
    assert call(d=lowd, norms=None) == E.NTT_ERR_PARAM
    # without d_hi the small d is accepted: the call gets as far as the next check (every
    # call here must fail validation: a valid one would launch on fake pointers)
    assert call(d=lowd, hi=None, ahat=ahat + 2) == E.NTT_ERR_ALIGN
    for bad_ps in (3, 4, 5, -1):
        assert call(ps=bad_ps) == E.NTT_ERR_PARAM   # n > 2048, unknown
    for k in (0, 9):
        assert call(k=k) == E.NTT_ERR_PARAM
    for l in (0, 3):
        assert call(l=l) == E.NTT_ERR_PARAM
    assert call(hi=None, norms=None) == E.NTT_ERR_NULL
    assert call(ys=None) == E.NTT_ERR_NULL
    assert call(ys=_ys(y0, None)) == E.NTT_ERR_NULL
    assert call(ys=_ys(None, y1)) == E.NTT_ERR_NULL
    assert call(ahat=None) == E.NTT_ERR_NULL
    assert call(ys=_ys(y0, None), l=1, ahat=ahat + 2) == E.NTT_ERR_ALIGN   # l = 1 reads d_y[0] only
    assert call(hi=hi + 4) == E.NTT_ERR_ALIGN
    assert call(norms=norms + 4) == E.NTT_ERR_ALIGN
    assert call(ys=_ys(y0 + 2, y1)) == E.NTT_ERR_ALIGN
    assert call(ys=_ys(y0, y1 + 2)) == E.NTT_ERR_ALIGN
    assert call(add=add + 2) == E.NTT_ERR_ALIGN
    assert call(batch=1 << 31) == E.NTT_ERR_SIZE
    batch, k, l = 3, 5, 2
    row = n * 4
    sizes = {"y0": batch * row, "y1": batch * row, "ahat": k * l * row, "add": batch * k * row}
    where = {"y0": y0, "y1": y1, "ahat": ahat, "add": add}
    hb, nb = batch * k * n, batch * k * 8
    for name, base in where.items():
        # one word of overlap at either end of the input, for each output
        assert call(hi=base + sizes[name] - 16) == E.NTT_ERR_ALIAS, name
        assert call(hi=base - hb + 16) == E.NTT_ERR_ALIAS, name
        assert call(norms=base + sizes[name] - 8) == E.NTT_ERR_ALIAS, name
        assert call(norms=base - nb + 8) == E.NTT_ERR_ALIAS, name
        assert call(hi=base, norms=None) == E.NTT_ERR_ALIAS, name   # equal is an overlap too: nothing is in place
        assert call(hi=None, norms=base) == E.NTT_ERR_ALIAS, name
    assert call(norms=hi + hb - 8) == E.NTT_ERR_ALIAS
    assert call(norms=hi - nb + 8) == E.NTT_ERR_ALIAS
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, hi=None, norms=None, ys=None, ahat=None, add=None) == E.NTT_OK
    assert call(batch=0, d=0) == E.NTT_ERR_PARAM
