"""poly_mul_ntt_kl_keyed and poly_mul_ntt_kl_round_keyed validate their
arguments before any GPU work (fake pointers that are never dereferenced; the
d_y array itself is real host memory, as the ABI asks), in the order of the
unkeyed entry point of the same name, and the Python wrappers reject wrong
shapes.  Every call here must fail validation or have an empty batch: a valid
one would launch on fake pointers."""
import ctypes
import re

import pytest

import round_model as M

FAKE = 0x10000000   # never dereferenced: validation comes first
FAR = 0x40000000    # regions well apart from FAKE
K_MAX, L_MAX = 8, 2
OUT, HI, NORMS = FAKE, FAKE, FAKE + FAR
Y0, Y1, AHAT, ADD, KEY = (FAKE + j * FAR for j in range(2, 7))
SETS = (0, 1, 2)
OWN_D = {0: M.OWN_D["ref"], 1: M.OWN_D["p-I"], 2: M.OWN_D["p-III"]}


def _ys(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _full(ntt, out=OUT, ys=(Y0, Y1), ahat=AHAT, key=KEY, nkeys=3, add=ADD, batch=3, k=5, l=2, ps=2):
    return ntt.lib().poly_mul_ntt_kl_keyed(out, None if ys is None else _ys(*ys), ahat, key, nkeys, add, batch, k, l, ps, None)


def _round(ntt, hi=HI, norms=NORMS, ys=(Y0, Y1), ahat=AHAT, key=KEY, nkeys=3, add=ADD, batch=3, k=5, l=2, d=None, ps=2):
    return ntt.lib().poly_mul_ntt_kl_round_keyed(hi, norms, None if ys is None else _ys(*ys), ahat, key, nkeys, add, batch,
                                                 k, l, OWN_D[ps] if d is None else d, ps, None)


def test_header_limits_match_binding(ntt):
    src = open(ntt.HEADER_PATH).read()
    assert int(re.search(r"#define NTT_MUL_KEYS_MAX (\d+)", src).group(1)) == ntt.MUL_KEYS_MAX == 2 ** 31 - 1
    assert int(re.search(r"#define NTT_MUL_L_MAX (\d+)", src).group(1)) == ntt.MUL_L_MAX == L_MAX
    assert int(re.search(r"#define NTT_MUL_K_MAX (\d+)", src).group(1)) == ntt.MUL_K_MAX == K_MAX
    for name in ("poly_mul_ntt_kl_keyed", "poly_mul_ntt_kl_round_keyed"):
        assert re.search(r"\bint %s\(" % name, src)


@pytest.mark.parametrize("call", (_full, _round), ids=("full", "round"))
def test_param(ntt, call):
    for batch in (1, 0):
        for ps in (-1, 3, 4, 5):   # unknown, and the n = 4096 / 8192 sets
            for l in (1, 2):
                assert call(ntt, batch=batch, l=l, ps=ps, **({"d": 24} if call is _round else {})) == ntt.NTT_ERR_PARAM
        for ps in SETS:
            for k in (0, -1, K_MAX + 1):
                assert call(ntt, batch=batch, k=k, ps=ps) == ntt.NTT_ERR_PARAM
            for l in (0, -1, L_MAX + 1):
                assert call(ntt, batch=batch, l=l, ys=(Y0, Y1, Y1), ps=ps) == ntt.NTT_ERR_PARAM
            # no keys at all: PARAM, also for an empty batch and before any NULL
            assert call(ntt, batch=batch, nkeys=0, ps=ps) == ntt.NTT_ERR_PARAM
            assert call(ntt, batch=batch, nkeys=0, ahat=None, key=None, ps=ps) == ntt.NTT_ERR_PARAM
    for ps in SETS:
        for d in (0, 31, M.min_d(ntt.param_info(ps)["q"]) - 1):
            assert _round(ntt, d=d, ps=ps) == ntt.NTT_ERR_PARAM


@pytest.mark.parametrize("call", (_full, _round), ids=("full", "round"))
def test_empty_batch_touches_nothing(ntt, call):
    for ps in SETS:
        for l in (1, 2):
            outs = {"out": None} if call is _full else {"hi": None, "norms": None}
            assert call(ntt, ys=None, ahat=None, key=None, add=None, batch=0, l=l, ps=ps, **outs) == ntt.NTT_OK
            assert call(ntt, ys=(None, Y1 + 1), ahat=AHAT + 1, key=KEY + 1, nkeys=1 << 31, add=ADD + 2, batch=0, l=l,
                        ps=ps) == ntt.NTT_OK


@pytest.mark.parametrize("call", (_full, _round), ids=("full", "round"))
def test_null_align_size(ntt, call):
    for ps in SETS:
        if call is _full:
            assert call(ntt, out=None, ps=ps) == ntt.NTT_ERR_NULL
        else:
            assert call(ntt, hi=None, norms=None, ps=ps) == ntt.NTT_ERR_NULL
        assert call(ntt, ys=None, ps=ps) == ntt.NTT_ERR_NULL
        assert call(ntt, ys=(None, Y1), ps=ps) == ntt.NTT_ERR_NULL
        assert call(ntt, ys=(Y0, None), ps=ps) == ntt.NTT_ERR_NULL
        assert call(ntt, ys=(None,), l=1, ps=ps) == ntt.NTT_ERR_NULL
        assert call(ntt, ahat=None, ps=ps) == ntt.NTT_ERR_NULL
        # d_key NULL is accepted: the call gets as far as the next defect
        assert call(ntt, key=None, add=ADD + 2, ps=ps) == ntt.NTT_ERR_ALIGN
        assert call(ntt, key=None, nkeys=1 << 31, ps=ps) == ntt.NTT_ERR_SIZE
        for bad in (1, 2, 3):
            assert call(ntt, key=KEY + bad, ps=ps) == ntt.NTT_ERR_ALIGN
            assert call(ntt, ys=(Y0, Y1 + bad), ps=ps) == ntt.NTT_ERR_ALIGN
            assert call(ntt, ahat=AHAT + bad, ps=ps) == ntt.NTT_ERR_ALIGN
            assert call(ntt, add=ADD + bad, ps=ps) == ntt.NTT_ERR_ALIGN
        assert call(ntt, batch=1 << 31, ps=ps) == ntt.NTT_ERR_SIZE
        assert call(ntt, nkeys=1 << 31, ps=ps) == ntt.NTT_ERR_SIZE
        assert call(ntt, nkeys=(1 << 31) - 1, key=KEY + 2, ps=ps) == ntt.NTT_ERR_ALIGN   # the largest nkeys is served
        # l = 1 never reads d_y[1]
        assert call(ntt, ys=(Y0, None), l=1, key=KEY + 2, ps=ps) == ntt.NTT_ERR_ALIGN


def test_first_defect_decides_full(ntt):
    """poly_mul_ntt_kl's order: PARAM, NULL, ALIGN, SIZE, ALIAS."""
    E = ntt
    for ps in SETS:
        for l in (1, 2):
            assert _full(ntt, nkeys=0, out=None, l=l, ps=ps) == E.NTT_ERR_PARAM
            assert _full(ntt, k=0, key=KEY + 1, l=l, ps=ps) == E.NTT_ERR_PARAM
            assert _full(ntt, out=None, key=KEY + 1, l=l, ps=ps) == E.NTT_ERR_NULL
            assert _full(ntt, ahat=None, nkeys=1 << 31, l=l, ps=ps) == E.NTT_ERR_NULL
            assert _full(ntt, ys=(None, Y1), batch=1 << 31, out=OUT + 2, l=l, ps=ps) == E.NTT_ERR_NULL
            assert _full(ntt, key=KEY + 2, nkeys=1 << 31, l=l, ps=ps) == E.NTT_ERR_ALIGN
            assert _full(ntt, key=KEY + 2, batch=1 << 31, l=l, ps=ps) == E.NTT_ERR_ALIGN
            assert _full(ntt, key=OUT + 2, l=l, ps=ps) == E.NTT_ERR_ALIGN                 # misaligned and overlapping
            assert _full(ntt, key=OUT, nkeys=1 << 31, l=l, ps=ps) == E.NTT_ERR_SIZE       # too many keys, and an output over d_key
            assert _full(ntt, ahat=OUT, batch=1 << 31, l=l, ps=ps) == E.NTT_ERR_SIZE
            assert _full(ntt, key=OUT, l=l, ps=ps) == E.NTT_ERR_ALIAS
    assert _full(ntt, out=None, key=KEY + 1, nkeys=0, ps=4) == E.NTT_ERR_PARAM


def test_first_defect_decides_round(ntt):
    """poly_mul_ntt_kl_round's order: PARAM, the inputs' NULLs, SIZE, the
    outputs' checks (NULL, d's byte range, ALIGN, their overlap), then the
    inputs' alignment -- d_key's with them -- and the overlaps."""
    E = ntt
    for ps in SETS:
        lowd = M.min_d(ntt.param_info(ps)["q"]) - 1
        bad = dict(key=KEY + 2, ps=ps)
        assert _round(ntt, **bad) == E.NTT_ERR_ALIGN                              # d_key misaligned, nothing else
        assert _round(ntt, nkeys=0, hi=None, norms=None, **bad) == E.NTT_ERR_PARAM
        assert _round(ntt, hi=None, norms=None, **bad) == E.NTT_ERR_NULL
        assert _round(ntt, ahat=None, nkeys=1 << 31, **bad) == E.NTT_ERR_NULL
        assert _round(ntt, nkeys=1 << 31, **bad) == E.NTT_ERR_SIZE                # SIZE before d_key's alignment
        assert _round(ntt, nkeys=1 << 31, hi=None, norms=None, **bad) == E.NTT_ERR_SIZE
        assert _round(ntt, batch=1 << 31, hi=HI + 4, **bad) == E.NTT_ERR_SIZE
        assert _round(ntt, d=lowd, **bad) == E.NTT_ERR_PARAM                      # d too small for hi: before d_key's alignment
        assert _round(ntt, d=lowd, hi=None, **bad) == E.NTT_ERR_ALIGN             # ... accepted without hi
        assert _round(ntt, hi=HI + 4, **bad) == E.NTT_ERR_ALIGN
        assert _round(ntt, norms=HI, **bad) == E.NTT_ERR_ALIAS                    # the outputs' overlap before d_key's alignment
        assert _round(ntt, hi=Y0, **bad) == E.NTT_ERR_ALIGN                       # d_key's alignment before an output over an input
        assert _round(ntt, hi=KEY, ps=ps) == E.NTT_ERR_ALIAS
        assert _round(ntt, ys=(Y0 + 2, None), l=1, hi=None, norms=None, ps=ps) == E.NTT_ERR_NULL   # l = 1 reads d_y[0] only


@pytest.mark.parametrize("l", (1, 2))
def test_alias_rules_full(ntt, l):
    for ps in SETS:
        n = ntt.param_info(ps)["n"]
        row, batch, k, nkeys = 4 * n, 3, 5, 3
        obytes, block = batch * k * row, k * l * row
        # out against d_ahat's whole extent, nkeys blocks: its first word, its
        # last word (inside key nkeys - 1's block, far outside key 0's), equality
        for a in (OUT, OUT + obytes - 4, OUT - nkeys * block + 4, OUT - (nkeys - 1) * block):
            assert _full(ntt, ahat=a, nkeys=nkeys, batch=batch, k=k, l=l, ps=ps) == ntt.NTT_ERR_ALIAS
        # the last placement puts out at the start of key nkeys - 1's block, clear of
        # key 0's: a check of one key's k*l*n words would let it through
        assert OUT - (nkeys - 1) * block + block <= OUT
        # out against d_key's batch words
        for key in (OUT, OUT + obytes - 4, OUT - batch * 4 + 4, OUT + row):
            assert _full(ntt, key=key, batch=batch, k=k, l=l, ps=ps) == ntt.NTT_ERR_ALIAS
        # ... and against the inputs of the unkeyed call, as there
        for y in (OUT, OUT + obytes - 4, OUT - batch * row + 4):
            assert _full(ntt, ys=(y, Y1), batch=batch, k=k, l=l, ps=ps) == ntt.NTT_ERR_ALIAS
        for add in (OUT + 4, OUT + obytes - 4, OUT - obytes + 4):
            assert _full(ntt, add=add, batch=batch, k=k, l=l, ps=ps) == ntt.NTT_ERR_ALIAS
        # (d_key over another input is legal, so such a call launches: tests/test_gpu_mul_ntt_kl_keyed.py)


@pytest.mark.parametrize("l", (1, 2))
def test_alias_rules_round(ntt, l):
    for ps in SETS:
        n = ntt.param_info(ps)["n"]
        row, batch, k, nkeys = 4 * n, 3, 5, 3
        hb, nb, block = batch * k * n, batch * k * 8, k * l * row
        sizes = {"ahat": nkeys * block, "key": batch * 4, "y0": batch * row, "add": batch * k * row}
        where = {"ahat": AHAT, "key": KEY, "y0": Y0, "add": ADD}

        def call(**kw):
            return _round(ntt, nkeys=nkeys, batch=batch, k=k, l=l, ps=ps, **kw)

        for name, base in where.items():
            # one word of overlap at either end of the input, for each output
            assert call(hi=base + sizes[name] - (16 if sizes[name] % 16 == 0 else sizes[name] % 16)) == ntt.NTT_ERR_ALIAS, name
            assert call(hi=base - hb + 16) == ntt.NTT_ERR_ALIAS, name
            assert call(norms=base + sizes[name] - (8 if sizes[name] % 8 == 0 else sizes[name] % 8)) == ntt.NTT_ERR_ALIAS, name
            assert call(norms=base - nb + 8) == ntt.NTT_ERR_ALIAS, name
            assert call(hi=base, norms=None) == ntt.NTT_ERR_ALIAS, name
            assert call(hi=None, norms=base) == ntt.NTT_ERR_ALIAS, name
        # an output inside key nkeys - 1's block, outside key 0's
        assert call(hi=AHAT + (nkeys - 1) * block + 16) == ntt.NTT_ERR_ALIAS
        assert call(norms=AHAT + nkeys * block - 8, hi=None) == ntt.NTT_ERR_ALIAS
        assert call(norms=HI + hb - 8) == ntt.NTT_ERR_ALIAS   # the outputs against each other


def test_wrapper_rejects_wrong_shapes(ntt):
    torch = pytest.importorskip("torch")
    for ps in ("ref", "p-III"):
        n = ntt.param_info(ps)["n"]
        batch, k, nkeys = 3, 5, 2

        def t(*shape, dtype=torch.int32):
            return torch.zeros(shape, dtype=dtype)

        y, ahat, out, keys = t(batch * n), t(nkeys, k, 2, n), t(batch * k * n), t(batch)
        hi = t(batch * k * n, dtype=torch.int8)
        for call in (lambda ys, a, ky, **kw: ntt.poly_mul_ntt_kl_keyed(kw.pop("out", out), ys, a, ky, ps, **kw),
                     lambda ys, a, ky, **kw: ntt.poly_mul_ntt_kl_round_keyed(ys, a, ky, ps, 24, hi=hi, **kw)):
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(k, 2, n), keys)              # 3-D: the unkeyed call's rows
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(nkeys * k * 2 * n), keys)    # flat
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(nkeys, k, 1, n), keys)       # l = 1 rows for two ys
            with pytest.raises(ValueError, match="^ahat:"):
                call([y], ahat, keys)
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(0, k, 2, n), keys)
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(nkeys, 9, 2, n), keys)
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(nkeys, k, 2, n + 4), keys)
            with pytest.raises(ValueError, match="^ahat:"):
                call([y, y], t(nkeys, k, 4, n)[:, :, ::2], keys)   # not contiguous
            with pytest.raises(ValueError, match="^keys:"):
                call([y, y], ahat, t(batch + 1))
            with pytest.raises(ValueError, match="^keys:"):
                call([y, y], ahat, t(batch - 1))
            with pytest.raises(ValueError, match="^keys:"):
                call([y, y], ahat, t(batch, 1))
            with pytest.raises(ValueError, match="^keys:"):
                call([y, y], ahat, t(batch, dtype=torch.int64))
            with pytest.raises(ValueError, match="^keys:"):
                call([y, y], ahat, t(batch, dtype=torch.uint8))
            with pytest.raises(ValueError, match="^ys:"):
                call([y, t(batch * n + n)], ahat, keys)
            with pytest.raises(ValueError, match="^add:"):
                call([y, y], ahat, keys, add=t(batch * n))
            with pytest.raises(ValueError, match="device tensors only"):   # right shapes, CPU tensors: no fallback
                call([y, y], ahat, keys)
            with pytest.raises(ValueError, match="device tensors only"):
                call([y, y], ahat, None)
        with pytest.raises(ValueError, match="^out:"):
            ntt.poly_mul_ntt_kl_keyed(t(batch * k * n - n), [y, y], ahat, keys, ps)
