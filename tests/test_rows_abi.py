"""ntt_rows_over, ntt_rows_differ, ntt_select and ntt_rows_move without a GPU:
the four symbols and their prototypes, the entry points' argument validation
with fake pointers (validation fails before any GPU work), every NTT_ERR_* and
each limit on both sides, the documented order of checks, the empty batch, and
the Python wrappers' own checks (dtypes and shapes come before the devices, so
CPU tensors reach them)."""
import ctypes

import pytest
import torch

FAKE = 0x100000   # never dereferenced
FAR = 0x40000000  # 1 GiB apart: no two fake buffers overlap
P0, P1, P2, P3, P4, P5 = (FAKE + i * FAR for i in range(6))
BIG = 1 << 31     # one row too many


def bounds(*vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


B1 = bounds(7)


def test_symbols_and_header(ntt):
    L = ntt.lib()
    for name in ("ntt_rows_over", "ntt_rows_differ", "ntt_select", "ntt_rows_move"):
        assert getattr(L, name).argtypes is not None
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    with open(ntt.HEADER_PATH) as f:
        src = f.read()
    assert "#define NTT_ROWS_M_MAX 16" in src and ntt.ROWS_M_MAX == 16
    import re
    h = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    for proto in (
            "int ntt_rows_over(uint32_t *d_flag, const void *d_vals, int width, int m, const uint64_t *bounds , "
            "int accumulate, size_t batch, void *stream);",
            "int ntt_rows_differ(uint32_t *d_flag, const uint8_t *d_a, size_t a_stride, const uint8_t *d_b, size_t b_stride, "
            "size_t row_bytes, int accumulate, size_t batch, void *stream);",
            "int ntt_select(uint32_t *d_idx, uint32_t *d_count, const uint32_t *d_flag, int want, uint32_t *d_bump, "
            "size_t batch, void *stream);",
            "int ntt_rows_move(uint8_t *d_dst, size_t dst_stride, const uint32_t *d_dst_idx, size_t dst_rows, "
            "const uint8_t *d_src, size_t src_stride, const uint32_t *d_src_idx, size_t src_rows, size_t row_bytes, "
            "const uint32_t *d_count, size_t count, void *stream);"):
        assert proto in h, proto


# ------------------------------------------------------------ ntt_rows_over

def _over(ntt):
    L = ntt.lib()

    def call(flag=P0, vals=P1, width=32, m=1, bnd=B1, accumulate=0, batch=3):
        return L.ntt_rows_over(flag, vals, width, m, bnd, accumulate, batch, None)
    return call


def test_rows_over_validation(ntt):
    """every call here must fail validation or be an empty batch: a valid one would launch on fake pointers"""
    E, call = ntt, _over(ntt)
    for kw in (dict(width=0), dict(width=16), dict(width=33), dict(width=128), dict(m=0), dict(m=17), dict(m=-1),
               dict(accumulate=2), dict(accumulate=-1)):
        assert call(**kw) == E.NTT_ERR_PARAM, kw
    # the accepted side of each limit: the call gets as far as the next check
    for kw in (dict(width=32), dict(width=64), dict(m=1), dict(m=16), dict(accumulate=0), dict(accumulate=1)):
        assert call(flag=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(flag=None), dict(vals=None), dict(bnd=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(flag=P0 + 2), dict(flag=P0 + 1), dict(vals=P1 + 2), dict(vals=P1 + 4, width=64), dict(vals=P1 + 1, width=64)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(vals=P1 + 4, width=32, batch=BIG) == E.NTT_ERR_SIZE    # a word-aligned uint32 row passes the alignment
    assert call(vals=P1 + 8, width=64, batch=BIG) == E.NTT_ERR_SIZE
    assert call(batch=BIG) == E.NTT_ERR_SIZE
    assert call(batch=BIG - 1, flag=P1) == E.NTT_ERR_ALIAS             # the largest batch passes the size check
    batch, m = 3, 2
    for width in (32, 64):
        vb = batch * m * width // 8
        for flag in (P1, P1 + vb - 4, P1 - 4 * batch + 4):              # equal, and one word at either end
            assert call(flag=flag, width=width, m=m, bnd=bounds(1, 2), batch=batch) == E.NTT_ERR_ALIAS, (width, hex(flag))
    # empty batch: a no-op whatever the pointers, after the parameter checks
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, flag=None, vals=None, bnd=None) == E.NTT_OK
    assert call(batch=0, flag=P0 + 1, vals=P0 + 1) == E.NTT_OK
    assert call(batch=0, width=8) == E.NTT_ERR_PARAM
    assert call(batch=0, m=17) == E.NTT_ERR_PARAM
    assert call(batch=0, accumulate=2) == E.NTT_ERR_PARAM


def test_rows_over_first_defect_decides(ntt):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the order is ABI"""
    E, call = ntt, _over(ntt)
    assert call(width=16, flag=None) == E.NTT_ERR_PARAM
    assert call(m=17, batch=BIG) == E.NTT_ERR_PARAM
    assert call(bnd=None, flag=P0 + 2) == E.NTT_ERR_NULL
    assert call(vals=None, batch=BIG) == E.NTT_ERR_NULL
    assert call(flag=P0 + 2, batch=BIG) == E.NTT_ERR_ALIGN
    assert call(flag=P1 + 2) == E.NTT_ERR_ALIGN
    assert call(flag=P1, batch=BIG) == E.NTT_ERR_SIZE
    assert call(flag=P1) == E.NTT_ERR_ALIAS


# ---------------------------------------------------------- ntt_rows_differ

def _differ(ntt):
    L = ntt.lib()

    def call(flag=P0, a=P1, a_stride=32, b=P2, b_stride=32, row_bytes=32, accumulate=0, batch=3):
        return L.ntt_rows_differ(flag, a, a_stride, b, b_stride, row_bytes, accumulate, batch, None)
    return call


def test_rows_differ_validation(ntt):
    E, call = ntt, _differ(ntt)
    for kw in (dict(row_bytes=0, a_stride=4, b_stride=4), dict(row_bytes=2), dict(row_bytes=30), dict(row_bytes=33, a_stride=36, b_stride=36),
               dict(a_stride=28), dict(b_stride=28), dict(a_stride=34), dict(b_stride=38), dict(a_stride=0), dict(accumulate=2),
               dict(accumulate=-1)):
        assert call(**kw) == E.NTT_ERR_PARAM, kw
    for kw in (dict(row_bytes=4), dict(row_bytes=32), dict(a_stride=32), dict(a_stride=36), dict(b_stride=5664), dict(accumulate=1),
               dict(row_bytes=4, a_stride=4, b_stride=4)):
        assert call(flag=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(flag=None), dict(a=None), dict(b=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(flag=P0 + 2), dict(a=P1 + 1), dict(a=P1 + 2), dict(b=P2 + 3)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(a=P1 + 4, b=P2 + 4, batch=BIG) == E.NTT_ERR_SIZE       # word alignment is enough
    assert call(batch=BIG - 1, flag=P1) == E.NTT_ERR_ALIAS
    batch, stride, row = 3, 40, 32
    extent = (batch - 1) * stride + row
    for which in ("a", "b"):
        base = P1 if which == "a" else P2
        for flag in (base, base + extent - 4, base - 4 * batch + 4):
            kw = dict(flag=flag, batch=batch, row_bytes=row, **{which + "_stride": stride})
            assert call(**kw) == E.NTT_ERR_ALIAS, (which, hex(flag))
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, flag=None, a=None, b=None) == E.NTT_OK
    assert call(batch=0, flag=P0 + 1, a=P0 + 1, b=P0 + 1) == E.NTT_OK
    assert call(batch=0, row_bytes=2) == E.NTT_ERR_PARAM
    assert call(batch=0, a_stride=28) == E.NTT_ERR_PARAM
    assert call(batch=0, accumulate=2) == E.NTT_ERR_PARAM


def test_rows_differ_order_and_overlapping_inputs(ntt):
    E, call = ntt, _differ(ntt)
    assert call(row_bytes=2, flag=None) == E.NTT_ERR_PARAM
    assert call(a_stride=28, batch=BIG) == E.NTT_ERR_PARAM
    assert call(a=None, flag=P0 + 2) == E.NTT_ERR_NULL
    assert call(b=None, batch=BIG) == E.NTT_ERR_NULL
    assert call(a=P1 + 2, batch=BIG) == E.NTT_ERR_ALIGN
    assert call(flag=P1 + 2) == E.NTT_ERR_ALIGN
    assert call(flag=P2, batch=BIG) == E.NTT_ERR_SIZE
    assert call(flag=P2) == E.NTT_ERR_ALIAS
    # the inputs may overlap each other, wholly or partly: only the flag is held apart
    assert call(a=P1, b=P1, flag=P1) == E.NTT_ERR_ALIAS
    assert call(a=P1, b=P1, batch=BIG) == E.NTT_ERR_SIZE
    assert call(a=P1, b=P1 + 8, batch=BIG) == E.NTT_ERR_SIZE


# --------------------------------------------------------------- ntt_select

def _select(ntt):
    L = ntt.lib()

    def call(idx=P0, count=P1, flag=P2, want=0, bump=P3, batch=3):
        return L.ntt_select(idx, count, flag, want, bump, batch, None)
    return call


def test_select_validation(ntt):
    E, call = ntt, _select(ntt)
    for want in (-1, 2):
        assert call(want=want) == E.NTT_ERR_PARAM
    for want in (0, 1):
        assert call(want=want, idx=None) == E.NTT_ERR_NULL
    for kw in (dict(idx=None), dict(count=None), dict(flag=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    assert call(bump=None, batch=BIG) == E.NTT_ERR_SIZE                # bump may be NULL
    for kw in (dict(idx=P0 + 2), dict(count=P1 + 1), dict(flag=P2 + 2), dict(bump=P3 + 2)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(batch=BIG) == E.NTT_ERR_SIZE
    assert call(batch=BIG - 1, idx=P2) == E.NTT_ERR_ALIAS
    batch = 5
    names = {"idx": (P0, 4 * batch), "count": (P1, 4), "flag": (P2, 4 * batch), "bump": (P3, 4 * batch)}
    for x, (bx, sx) in names.items():
        for y, (by, sy) in names.items():
            if x == y:
                continue
            for px in (by, by + sy - 4, by - sx + 4):    # equal starts, and one word at either end
                assert call(batch=batch, **{x: px}) == E.NTT_ERR_ALIAS, (x, y, hex(px))
    assert call(batch=0) == E.NTT_OK
    assert call(batch=0, idx=None, count=None, flag=None, bump=None) == E.NTT_OK
    assert call(batch=0, idx=P0 + 1, count=P0 + 1) == E.NTT_OK
    assert call(batch=0, want=2) == E.NTT_ERR_PARAM


def test_select_first_defect_decides(ntt):
    E, call = ntt, _select(ntt)
    assert call(want=2, idx=None) == E.NTT_ERR_PARAM
    assert call(want=2, batch=BIG) == E.NTT_ERR_PARAM
    assert call(count=None, idx=P0 + 2) == E.NTT_ERR_NULL
    assert call(flag=None, batch=BIG) == E.NTT_ERR_NULL
    assert call(bump=P3 + 2, batch=BIG) == E.NTT_ERR_ALIGN
    assert call(idx=P2 + 2) == E.NTT_ERR_ALIGN
    assert call(idx=P2, batch=BIG) == E.NTT_ERR_SIZE
    assert call(idx=P2) == E.NTT_ERR_ALIAS


# ------------------------------------------------------------ ntt_rows_move

def _move(ntt):
    L = ntt.lib()

    def call(dst=P0, dst_stride=32, dst_idx=P1, dst_rows=8, src=P2, src_stride=32, src_idx=P3, src_rows=8, row_bytes=32,
             dcount=P4, count=3):
        return L.ntt_rows_move(dst, dst_stride, dst_idx, dst_rows, src, src_stride, src_idx, src_rows, row_bytes, dcount, count,
                               None)
    return call


def test_rows_move_validation(ntt):
    E, call = ntt, _move(ntt)
    for kw in (dict(row_bytes=0, dst_stride=4, src_stride=4), dict(row_bytes=2), dict(row_bytes=30), dict(dst_stride=28),
               dict(src_stride=28), dict(dst_stride=34), dict(src_stride=38), dict(src_stride=0)):
        assert call(**kw) == E.NTT_ERR_PARAM, kw
    for kw in (dict(row_bytes=4), dict(row_bytes=12), dict(dst_stride=36), dict(src_stride=5664),
               dict(row_bytes=4, dst_stride=4, src_stride=4)):
        assert call(dst=None, **kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(dst=None), dict(src=None)):
        assert call(**kw) == E.NTT_ERR_NULL, kw
    for kw in (dict(dst_idx=None), dict(src_idx=None), dict(dcount=None), dict(dst_idx=None, src_idx=None, dcount=None)):
        assert call(count=BIG, **kw) == E.NTT_ERR_SIZE, kw            # each of the three may be NULL
    for kw in (dict(dst=P0 + 2), dict(src=P2 + 1), dict(dst_idx=P1 + 2), dict(src_idx=P3 + 2), dict(dcount=P4 + 2)):
        assert call(**kw) == E.NTT_ERR_ALIGN, kw
    assert call(dst=P0 + 4, src=P2 + 4, count=BIG) == E.NTT_ERR_SIZE   # word alignment is enough
    for kw in (dict(count=BIG), dict(dst_rows=BIG), dict(src_rows=BIG)):
        assert call(**kw) == E.NTT_ERR_SIZE, kw
    for kw in (dict(count=BIG - 1), dict(dst_rows=BIG - 1, dst_stride=4, row_bytes=4, src_stride=4),
               dict(src_rows=BIG - 1, dst_stride=4, row_bytes=4, src_stride=4)):
        assert call(dst=P2, **kw) == E.NTT_ERR_ALIAS, kw                # the largest sizes pass the size check
    rows, stride, row, count = 8, 40, 32, 3
    extent = (rows - 1) * stride + row
    others = {"src": extent, "dst_idx": 4 * count, "src_idx": 4 * count, "dcount": 4}
    base = {"src": P2, "dst_idx": P1, "src_idx": P3, "dcount": P4}
    for name, size in others.items():
        for dst in (base[name], base[name] + size - 4, base[name] - extent + 4):
            kw = dict(dst=dst, dst_stride=stride, src_stride=stride, row_bytes=row, count=count)
            assert call(**kw) == E.NTT_ERR_ALIAS, (name, hex(dst))
    # the inputs may overlap each other
    assert call(src_idx=P1, dcount=P1, count=BIG) == E.NTT_ERR_SIZE
    assert call(src_idx=P1, dcount=P1, dst=P1) == E.NTT_ERR_ALIAS
    assert call(count=0) == E.NTT_OK
    assert call(count=0, dst=None, src=None, dst_idx=None, src_idx=None, dcount=None) == E.NTT_OK
    assert call(count=0, dst=P0 + 1, src=P0 + 1) == E.NTT_OK
    assert call(count=0, row_bytes=2) == E.NTT_ERR_PARAM
    assert call(count=0, dst_stride=28) == E.NTT_ERR_PARAM


def test_rows_move_first_defect_decides(ntt):
    E, call = ntt, _move(ntt)
    assert call(row_bytes=2, dst=None) == E.NTT_ERR_PARAM
    assert call(src_stride=28, count=BIG) == E.NTT_ERR_PARAM
    assert call(src=None, dst=P0 + 2) == E.NTT_ERR_NULL
    assert call(dst=None, count=BIG) == E.NTT_ERR_NULL
    assert call(src_idx=P3 + 2, count=BIG) == E.NTT_ERR_ALIGN
    assert call(dst=P2 + 2) == E.NTT_ERR_ALIGN
    assert call(dst=P2, count=BIG) == E.NTT_ERR_SIZE
    assert call(dst=P2) == E.NTT_ERR_ALIAS


# ------------------------------------------------------------- the wrappers

def test_wrappers_reject_before_the_call(ntt):
    """dtype and shape errors are found on CPU tensors; well-formed CPU tensors are refused as such (no CPU fallback)"""
    i32 = dict(dtype=torch.int32)
    flag, norms, sums = torch.zeros(3, **i32), torch.zeros((3, 2), **i32), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        ntt.rows_over(flag, norms.to(torch.int16), [1, 2])
    with pytest.raises(TypeError):
        ntt.rows_over(flag.to(torch.int64), norms, [1, 2])
    with pytest.raises(ValueError):
        ntt.rows_over(flag, norms, [1])                      # one bound for two values
    with pytest.raises(ValueError):
        ntt.rows_over(flag, norms, [])
    with pytest.raises(ValueError):
        ntt.rows_over(flag, torch.zeros((3, 17), **i32), [0] * 17)
    with pytest.raises(ValueError):
        ntt.rows_over(flag[:2].clone(), norms, [1, 2])
    with pytest.raises(ValueError):
        ntt.rows_over(flag, norms, [1, 1 << 64])
    with pytest.raises(ValueError):
        ntt.rows_over(flag, norms, [-1, 1])
    with pytest.raises(ValueError):
        ntt.rows_over(flag, torch.zeros((3, 4), **i32)[:, :2], [1, 2])   # not contiguous
    with pytest.raises(ValueError):
        ntt.rows_over(torch.zeros(6, **i32)[::2], norms, [1, 2])
    for vals, bnd in ((norms, [1, (1 << 32) - 1]), (sums, [(1 << 64) - 1]), (torch.zeros((3, 4, 2), **i32), [5] * 8)):
        with pytest.raises(ValueError, match="device tensors"):
            ntt.rows_over(flag, vals, bnd, accumulate=True)

    sig, c2 = torch.zeros((3, 2592), dtype=torch.uint8), torch.zeros((3, 32), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ntt.rows_differ(flag, c2, sig[:, 2560:2590])            # 30 bytes: not the other side's 32, not a multiple of 4
    with pytest.raises(ValueError):
        ntt.rows_differ(flag, c2[:, :30], sig[:, 2560:2590])
    with pytest.raises(ValueError):
        ntt.rows_differ(flag, c2[:2], sig[:, 2560:])
    with pytest.raises(ValueError):
        ntt.rows_differ(flag, c2, sig[:, 2560::1][:, ::2][:, :32])   # a row with gaps in itself
    with pytest.raises(ValueError):
        ntt.rows_differ(flag[:2].clone(), c2, sig[:, 2560:])
    with pytest.raises(TypeError):
        ntt.rows_differ(flag.to(torch.uint8), c2, sig[:, 2560:])
    with pytest.raises(ValueError):
        ntt.rows_differ(flag, c2, torch.zeros((3, 2594), dtype=torch.uint8)[:, 2562:])   # rows 2594 bytes apart
    with pytest.raises(ValueError, match="device tensors"):
        ntt.rows_differ(flag, c2, sig[:, 2560:])                # a view of the signature rows is well formed

    idx, count, bump = torch.zeros(3, **i32), torch.zeros(1, **i32), torch.zeros(3, **i32)
    with pytest.raises(ValueError):
        ntt.select(idx[:2].clone(), count, flag, 0)
    with pytest.raises(ValueError):
        ntt.select(idx, torch.zeros(2, **i32), flag, 0)
    with pytest.raises(ValueError):
        ntt.select(idx, count, flag, 2)
    with pytest.raises(ValueError):
        ntt.select(idx, count, flag, 0, bump=bump[:2].clone())
    with pytest.raises(ValueError):
        ntt.select(idx, count, flag.view(3, 1), 0)
    with pytest.raises(TypeError):
        ntt.select(idx, count, flag.to(torch.bool), 0)
    with pytest.raises(TypeError):
        ntt.select(idx, count, flag, 1, bump=bump.to(torch.int64))
    for want, bmp in ((0, None), (True, bump)):
        with pytest.raises(ValueError, match="device tensors"):
            ntt.select(idx, count, flag, want, bump=bmp)

    full, sub = torch.zeros((5, 2592), dtype=torch.uint8), torch.zeros((3, 2560), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ntt.rows_move(full, sub)                                # 2592 against 2560 bytes per row
    with pytest.raises(ValueError):
        ntt.rows_move(full[:, :30], sub[:, :30])
    with pytest.raises(ValueError):
        ntt.rows_move(full[:, :2560], sub, dst_idx=idx, n=4)    # more rows than indices
    with pytest.raises(ValueError):
        ntt.rows_move(full[:, :2560], sub, count=torch.zeros(2, **i32))
    with pytest.raises(TypeError):
        ntt.rows_move(full[:, :2560], sub, src_idx=idx.to(torch.int64))
    with pytest.raises(ValueError):
        ntt.rows_move(full[:, :2560], sub, n=-1)
    with pytest.raises(ValueError):
        ntt.rows_move(torch.zeros(5, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8))   # one byte per row
    for kw in (dict(), dict(dst_idx=idx), dict(src_idx=idx, count=count), dict(dst_idx=idx, src_idx=idx, count=count, n=2)):
        with pytest.raises(ValueError, match="device tensors"):
            ntt.rows_move(full[:, :2560], sub, **kw)
    with pytest.raises(ValueError, match="device tensors"):
        ntt.rows_move(torch.zeros(5, **i32), torch.zeros(3, **i32), dst_idx=idx)   # one int32 per row: the nonces
    with pytest.raises(ValueError, match="device tensors"):
        ntt.rows_move(torch.zeros((5, 8), dtype=torch.int64), torch.zeros((3, 64), dtype=torch.uint8))   # bytes per row decide
