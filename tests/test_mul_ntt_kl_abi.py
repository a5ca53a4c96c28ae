"""poly_mul_ntt_kl and poly_scatter validate their arguments before any GPU
work (fake pointers that are never dereferenced; the d_y array itself is real
host memory, as the ABI asks), and the Python wrappers reject wrong shapes."""
import ctypes
import re

import pytest

FAKE = 0x10000000   # never dereferenced: validation comes first
FAR = 0x40000000    # regions well apart from FAKE
K_MAX, L_MAX = 8, 2


def _ys(*ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _call(ntt, out, ys, ahat, add, batch, k, l, ps):
    return ntt.lib().poly_mul_ntt_kl(out, None if ys is None else _ys(*ys), ahat, add, batch, k, l, ps, None)


def test_header_limit_matches_binding(ntt):
    src = open(ntt.HEADER_PATH).read()
    assert int(re.search(r"#define NTT_MUL_L_MAX (\d+)", src).group(1)) == ntt.MUL_L_MAX == L_MAX


def test_param_set_k_and_l_range(ntt):
    out, ys, ahat = FAKE, (FAR, 2 * FAR), 3 * FAR
    for batch in (1, 0):
        for ps in (-1, 3, 4, 5):   # unknown, and the n = 4096 / 8192 sets
            assert _call(ntt, out, ys, ahat, None, batch, 1, 2, ps) == ntt.NTT_ERR_PARAM
            assert _call(ntt, out, ys, ahat, None, batch, 1, 1, ps) == ntt.NTT_ERR_PARAM
        for ps in (0, 1, 2):
            for k in (0, -1, K_MAX + 1):
                assert _call(ntt, out, ys, ahat, None, batch, k, 2, ps) == ntt.NTT_ERR_PARAM
                assert _call(ntt, out, ys, ahat, None, batch, k, 1, ps) == ntt.NTT_ERR_PARAM
            for l in (0, -1, L_MAX + 1):
                assert _call(ntt, out, ys + (4 * FAR,), ahat, None, batch, 4, l, ps) == ntt.NTT_ERR_PARAM


def test_empty_batch_touches_nothing(ntt):
    for ps in (0, 1, 2):
        for l in (1, 2):
            assert _call(ntt, None, None, None, None, 0, 1, l, ps) == ntt.NTT_OK
            assert _call(ntt, FAKE + 2, (None, FAKE + 1), FAKE, FAKE + 1, 0, K_MAX, l, ps) == ntt.NTT_OK


def test_null_align_size(ntt):
    out, y0, y1, ahat = FAKE, FAR, 2 * FAR, 3 * FAR
    for ps in (0, 1, 2):
        assert _call(ntt, None, (y0, y1), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, None, ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, (None, y1), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, (y0, None), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, (None,), ahat, None, 1, 4, 1, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, (y0, y1), None, None, 1, 4, 2, ps) == ntt.NTT_ERR_NULL
        for bad in (1, 2, 3):
            assert _call(ntt, out + bad, (y0, y1), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, (y0 + bad, y1), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, (y0, y1 + bad), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, (y0, y1), ahat + bad, None, 1, 4, 2, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, (y0, y1), ahat, 5 * FAR + bad, 1, 4, 2, ps) == ntt.NTT_ERR_ALIGN
        assert _call(ntt, out, (y0, y1), ahat, None, 1 << 31, 1, 2, ps) == ntt.NTT_ERR_SIZE
        assert _call(ntt, out, (y0, y1 + 1), ahat, None, 1 << 31, 1, 2, ps) == ntt.NTT_ERR_ALIGN   # alignment before size
        assert _call(ntt, out, (y0, None), ahat, None, 1 << 31, 1, 2, ps) == ntt.NTT_ERR_NULL      # NULL before size


def test_first_defect_decides(ntt):
    """Two defects at once: PARAM, NULL, ALIGN, SIZE, ALIAS in that order (ABI),
    for l = 2 and for l = 1 (which poly_mul_ntt_k finishes)."""
    out, y0, y1, ahat, add = FAKE, FAR, 2 * FAR, 3 * FAR, 5 * FAR
    for ps in (0, 1, 2):
        for l in (1, 2):
            assert _call(ntt, None, (y0 + 1, y1), ahat, None, 1, 4, l, ps) == ntt.NTT_ERR_NULL
            assert _call(ntt, out + 2, (None, y1), ahat, None, 1 << 31, 4, l, ps) == ntt.NTT_ERR_NULL
            assert _call(ntt, out, (y0, y1), ahat, add + 2, 1 << 31, 4, l, ps) == ntt.NTT_ERR_ALIGN
            assert _call(ntt, out, (out + 2, y1), ahat, None, 3, 4, l, ps) == ntt.NTT_ERR_ALIGN   # misaligned and overlapping
            assert _call(ntt, out, (out, y1), ahat, None, 1 << 31, 4, l, ps) == ntt.NTT_ERR_SIZE
            assert _call(ntt, None, (y0, y1), ahat, None, 1, 0, l, ps) == ntt.NTT_ERR_PARAM
        assert _call(ntt, None, (y0, y1 + 1), ahat, None, 1, 4, 2, ps) == ntt.NTT_ERR_NULL
        assert _call(ntt, out, (y0, out), ahat, add + 1, 3, 4, 2, ps) == ntt.NTT_ERR_ALIGN
        # l = 1 never reads d_y[1]
        assert _call(ntt, out, (y0, None), ahat, add + 1, 3, 4, 1, ps) == ntt.NTT_ERR_ALIGN
    assert _call(ntt, None, (y0 + 1, y1), ahat, None, 1, 4, 2, 4) == ntt.NTT_ERR_PARAM


def test_alias_rules(ntt):
    for ps in (0, 1, 2):
        n = ntt.param_info(ps)["n"]
        row, batch, k, l = 4 * n, 3, 5, 2
        obytes = batch * k * row
        out = FAKE
        y_ok, y1_ok, a_ok = FAR, 2 * FAR, 3 * FAR
        # out against y_0 and y_1 (batch*n words each): equality, first word, last word
        for y in (out, out + obytes - 4, out - batch * row + 4, out + row):
            assert _call(ntt, out, (y, y1_ok), a_ok, None, batch, k, l, ps) == ntt.NTT_ERR_ALIAS
            assert _call(ntt, out, (y_ok, y), a_ok, None, batch, k, l, ps) == ntt.NTT_ERR_ALIAS
        # ... and the full k*l*n words of ahat: its last word on out's first is
        # k*l*row - 4 below out, outside a k*n-word extent
        for a in (out, out + obytes - 4, out - k * l * row + 4, out + row):
            assert _call(ntt, out, (y_ok, y1_ok), a, None, batch, k, l, ps) == ntt.NTT_ERR_ALIAS
        assert k * l * row - 4 >= k * row
        # add: equal to out is the in-place form, a partial overlap is rejected
        for add in (out + 4, out + row, out - row, out + obytes - 4, out - obytes + 4):
            assert _call(ntt, out, (y_ok, y1_ok), a_ok, add, batch, k, l, ps) == ntt.NTT_ERR_ALIAS


# The legal overlaps (y_0 == y_1, add overlapping an input) get past validation
# and launch, so they are run on real buffers: tests/test_gpu_mul_ntt_kl.py,
# test_pointer_forms.


def test_launch_shape_query(ntt):
    L = ntt.lib()
    v, w = ctypes.c_size_t(), ctypes.c_int()
    for ps in (-1, 3, 4, 5):
        for l in (1, 2):
            assert L.ntt_mul_kl_shape(ps, l, ctypes.byref(v), ctypes.byref(w)) == ntt.NTT_ERR_PARAM
    for name in ("ref", "p-I", "p-III"):
        for l in (0, -1, L_MAX + 1):
            assert L.ntt_mul_kl_shape(ntt.PARAM_SETS[name], l, ctypes.byref(v), ctypes.byref(w)) == ntt.NTT_ERR_PARAM
        assert L.ntt_mul_kl_shape(ntt.PARAM_SETS[name], 2, None, None) == ntt.NTT_OK
        shape = ntt.mul_kl_shape(name, 2)
        assert shape["waves"] >= 1 and 0 <= shape["split_max"] < 2 ** 31
        assert ntt.mul_kl_shape(name, 1) == ntt.mul_k_shape(name)


def test_wrapper_rejects_wrong_shapes(ntt):
    torch = pytest.importorskip("torch")
    for ps in ("ref", "p-III"):
        n = ntt.param_info(ps)["n"]
        batch, k = 3, 5

        def t(words):
            return torch.zeros(words, dtype=torch.int32)

        y, ahat, out = t(batch * n), t(k * 2 * n), t(batch * k * n)
        with pytest.raises(ValueError, match="^out:"):
            ntt.poly_mul_ntt_kl(t(batch * k * n - n), [y, y], ahat, ps)
        with pytest.raises(ValueError, match="^out:"):
            ntt.poly_mul_ntt_kl(t(batch * n), [y, y], ahat, ps)
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_kl(out, [y, y], t(k * 2 * n + 4), ps)
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_kl(out, [y, y], t(k * n), ps)   # k*n words are not k rows of l = 2
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_kl(out, [y, y], t(0), ps)
        with pytest.raises(ValueError, match="^ahat:"):
            ntt.poly_mul_ntt_kl(t(batch * 9 * n), [y, y], t(9 * 2 * n), ps)
        with pytest.raises(ValueError, match="^ys:"):
            ntt.poly_mul_ntt_kl(out, [], ahat, ps)
        with pytest.raises(ValueError, match="^ys:"):
            ntt.poly_mul_ntt_kl(out, [y, y, y], ahat, ps)
        with pytest.raises(ValueError, match="^ys:"):
            ntt.poly_mul_ntt_kl(out, [y, t(batch * n + n)], ahat, ps)
        with pytest.raises(ValueError, match="^ys:"):
            ntt.poly_mul_ntt_kl(out, [t(batch * n + 4), y], ahat, ps)
        with pytest.raises(ValueError, match="^add:"):
            ntt.poly_mul_ntt_kl(out, [y, y], ahat, ps, add=t(batch * n))
        with pytest.raises(ValueError, match="device tensors only"):   # right shapes, CPU tensors: no fallback
            ntt.poly_mul_ntt_kl(out, [y, y], ahat, ps, add=out)
        with pytest.raises(ValueError, match="^out:"):
            ntt.poly_scatter(t(batch * n + 4), t(batch * 25), t(batch * 25), ps)
        with pytest.raises(ValueError, match="^pos:"):
            ntt.poly_scatter(t(batch * n), t(batch * 25 + 1), t(batch * 25 + 1), ps)
        with pytest.raises(ValueError, match="^pos:"):
            ntt.poly_scatter(t(batch * n), t(0), t(0), ps)
        with pytest.raises(ValueError, match="^pos:"):
            ntt.poly_scatter(t(batch * n), t(batch * (n + 1)), t(batch * (n + 1)), ps)
        with pytest.raises(ValueError, match="^val:"):
            ntt.poly_scatter(t(batch * n), t(batch * 25), t(batch * 24), ps)
        with pytest.raises(ValueError, match="device tensors only"):
            ntt.poly_scatter(t(batch * n), t(batch * 25), t(batch * 25), ps)


def _scatter(ntt, out, pos, val, batch, h, ps):
    return ntt.lib().poly_scatter(out, pos, val, batch, h, ps, None)


def test_scatter_validation(ntt):
    out, pos, val = FAKE, FAR, 2 * FAR
    for ps in (-1, 5):
        assert _scatter(ntt, out, pos, val, 1, 1, ps) == ntt.NTT_ERR_PARAM
    for ps in range(5):   # all five sets
        n = ntt.param_info(ps)["n"]
        for batch in (1, 0):
            for h in (0, -1, n + 1):
                assert _scatter(ntt, out, pos, val, batch, h, ps) == ntt.NTT_ERR_PARAM
        assert _scatter(ntt, None, None, None, 0, 1, ps) == ntt.NTT_OK
        assert _scatter(ntt, FAKE + 1, FAKE, FAKE, 0, n, ps) == ntt.NTT_OK
        assert _scatter(ntt, None, pos, val, 1, 25, ps) == ntt.NTT_ERR_NULL
        assert _scatter(ntt, out, None, val, 1, 25, ps) == ntt.NTT_ERR_NULL
        assert _scatter(ntt, out, pos, None, 1, 25, ps) == ntt.NTT_ERR_NULL
        for bad in (1, 2, 3):
            assert _scatter(ntt, out + bad, pos, val, 1, 25, ps) == ntt.NTT_ERR_ALIGN
            assert _scatter(ntt, out, pos + bad, val, 1, 25, ps) == ntt.NTT_ERR_ALIGN
            assert _scatter(ntt, out, pos, val + bad, 1, 25, ps) == ntt.NTT_ERR_ALIGN
        assert _scatter(ntt, out, pos, val, 1 << 31, 25, ps) == ntt.NTT_ERR_SIZE
        batch, h = 3, 25
        obytes, lbytes = batch * n * 4, batch * h * 4
        for p in (out, out + obytes - 4, out - lbytes + 4, out + 4 * n):
            assert _scatter(ntt, out, p, val, batch, h, ps) == ntt.NTT_ERR_ALIAS
            assert _scatter(ntt, out, pos, p, batch, h, ps) == ntt.NTT_ERR_ALIAS
