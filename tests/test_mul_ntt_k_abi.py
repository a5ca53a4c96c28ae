"""poly_mul_ntt_k validates its arguments before any GPU work (fake pointers
that are never dereferenced), and the Python wrapper rejects wrong shapes."""
import re

import pytest

FAKE = 0x10000000   # never dereferenced: validation comes first
FAR = 0x40000000    # regions well apart from FAKE
K_MAX = 8


def _call(ntt, out, y, ahat, add, batch, k, ps):
    return ntt.lib().poly_mul_ntt_k(out, y, ahat, add, batch, k, ps, None)


def test_header_limit_matches_binding(ntt):
    src = open(ntt.HEADER_PATH).read()
    assert int(re.search(r"#define NTT_MUL_K_MAX (\d+)", src).group(1)) == ntt.MUL_K_MAX == K_MAX


def test_param_set_and_k_range(ntt):
    out, y, ahat = FAKE, FAR, 2 * FAR
    for ps in (-1, 3, 4, 5):   # unknown, and the n = 4096 / 8192 sets
        assert _call(ntt, out, y, ahat, None, 1, 1, ps) == ntt.NTT_ERR_PARAM
        assert _call(ntt, out, y, ahat, None, 0, 1, ps) == ntt.NTT_ERR_PARAM
    for ps in (0, 1, 2):
        for k in (0, -1, K_MAX + 1):
            assert _call(ntt, out, y, ahat, None, 1, k, ps) == ntt.NTT_ERR_PARAM
            assert _call(ntt, out, y, ahat, None, 0, k, ps) == ntt.NTT_ERR_PARAM


def test_empty_batch_touches_nothing(ntt):
    for ps in (0, 1, 2):
        assert _call(ntt, None, None, None, None, 0, 1, ps) == ntt.NTT_OK
        assert _call(ntt, FAKE + 2, FAKE, FAKE, FAKE + 1, 0, K_MAX, ps) == ntt.NTT_OK


def test_null_align_size(ntt):
    out, y, ahat = FAKE, FAR, 2 * FAR
    for ps in (0, 1, 2):
        assert _call(ntt, None, y, ahat, None, 1, 4, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, None, ahat, None, 1, 4, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, y, None, None, 1, 4, ps) == ntt.NTT_ERR_NULL
        for bad in (1, 2, 3):
            assert _call(ntt, out + bad, y, ahat, None, 1, 4, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, y + bad, ahat, None, 1, 4, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, y, ahat + bad, None, 1, 4, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, y, ahat, 3 * FAR + bad, 1, 4, ps) == ntt.NTT_ERR_ALIGN
        assert _call(ntt, out, y, ahat, None, 1 << 31, 1, ps) == ntt.NTT_ERR_SIZE
        assert _call(ntt, None, y, ahat, None, 1 << 31, 1, ps) == ntt.NTT_ERR_NULL   # NULL before size


def test_first_defect_decides(ntt):
    """Two defects at once: PARAM, NULL, ALIGN, SIZE, ALIAS in that order (ABI)."""
    out, y, ahat, add = FAKE, FAR, 2 * FAR, 3 * FAR
    for ps in (0, 1, 2):
        assert _call(ntt, None, y + 1, ahat, None, 1, 4, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out + 2, y, None, None, 1 << 31, 4, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, y, ahat, add + 2, 1 << 31, 4, ps) == ntt.NTT_ERR_ALIGN
        assert _call(ntt, out, out + 2, ahat, None, 3, 4, ps) == ntt.NTT_ERR_ALIGN   # misaligned and overlapping
        assert _call(ntt, out, out, ahat, None, 1 << 31, 4, ps) == ntt.NTT_ERR_SIZE
        assert _call(ntt, None, y, ahat, None, 1, 0, ps) == ntt.NTT_ERR_PARAM
    assert _call(ntt, None, y + 1, ahat, None, 1, 4, 3) == ntt.NTT_ERR_PARAM


def test_alias_rules(ntt):
    for ps in (0, 1, 2):
        n = ntt.param_info(ps)["n"]
        row, batch, k = 4 * n, 3, 5
        obytes = batch * k * row
        out = FAKE
        y_ok, a_ok = FAR, 2 * FAR
        # out against y (batch*n words) and ahat (k*n words): any overlap, equality included
        for y in (out, out + row, out + obytes - 4, out - batch * row + 4):
            assert _call(ntt, out, y, a_ok, None, batch, k, ps) == ntt.NTT_ERR_ALIAS
        for a in (out, out + row, out + obytes - 4, out - k * row + 4):
            assert _call(ntt, out, y_ok, a, None, batch, k, ps) == ntt.NTT_ERR_ALIAS
        # add: equal to out is the in-place form, a partial overlap is rejected
        for add in (out + 4, out + row, out - row, out + obytes - 4, out - obytes + 4):
            assert _call(ntt, out, y_ok, a_ok, add, batch, k, ps) == ntt.NTT_ERR_ALIAS


def test_launch_shape_query(ntt):
    import ctypes
    L = ntt.lib()
    v, w = ctypes.c_size_t(), ctypes.c_int()
    for ps in (-1, 3, 4, 5):
        assert L.ntt_mul_k_shape(ps, ctypes.byref(v), ctypes.byref(w)) == ntt.NTT_ERR_PARAM
    for name in ("ref", "p-I", "p-III"):
        assert L.ntt_mul_k_shape(ntt.PARAM_SETS[name], None, None) == ntt.NTT_OK
        shape = ntt.mul_k_shape(name)
        assert shape["waves"] >= 1 and 0 <= shape["split_max"] < 2 ** 31


def test_wrapper_rejects_wrong_shapes(ntt):
    torch = pytest.importorskip("torch")
    for ps in ("ref", "p-III"):
        n = ntt.param_info(ps)["n"]
        batch, k = 3, 5

        def t(words):
            return torch.zeros(words, dtype=torch.int32)

        y, ahat, out = t(batch * n), t(k * n), t(batch * k * n)
        with pytest.raises(ValueError, match="^out:"):
            ntt.poly_mul_ntt_k(t(batch * k * n - n), y, ahat, ps)
        with pytest.raises(ValueError, match="^out:"):
            ntt.poly_mul_ntt_k(t(batch * n), y, ahat, ps)
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_k(out, y, t(k * n + 4), ps)
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_k(out, y, t(0), ps)
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_k(t(batch * 9 * n), y, t(9 * n), ps)
        with pytest.raises(ValueError, match="^y:"):
            ntt.poly_mul_ntt_k(out, t(batch * n + 4), ahat, ps)
        with pytest.raises(ValueError, match="^add:"):
            ntt.poly_mul_ntt_k(out, y, ahat, ps, add=t(batch * n))
        with pytest.raises(ValueError, match="device tensors only"):   # right shapes, CPU tensors: no fallback
            ntt.poly_mul_ntt_k(out, y, ahat, ps, add=out)
