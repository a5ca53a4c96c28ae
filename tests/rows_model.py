"""The four definitions of ntt_rows_over, ntt_rows_differ, ntt_select and
ntt_rows_move (include/qtesla_ntt.h) restated in numpy, one plain loop or one
array expression each: what tests/test_gpu_rows.py compares the device with,
for equality."""
import numpy as np


def rows_over(flag, vals, bounds, accumulate):
    """flag uint32 [batch], vals unsigned [batch][m], bounds m Python ints"""
    over = np.zeros(len(flag), dtype=bool)
    vals = vals.reshape(len(flag), -1)
    assert vals.shape[1] == len(bounds) and vals.dtype in (np.uint32, np.uint64)
    for j, bound in enumerate(bounds):
        over |= vals[:, j].astype(np.uint64) > np.uint64(bound)   # both sides uint64: exact up to 2^64 - 1
    f = over.astype(np.uint32)
    return (flag | f) if accumulate else f


def rows_differ(flag, a, a_stride, b, b_stride, row_bytes, accumulate):
    """a, b uint8 buffers; row r is bytes [r stride, r stride + row_bytes)"""
    f = np.zeros(len(flag), dtype=np.uint32)
    for r in range(len(flag)):
        f[r] = not np.array_equal(a[r * a_stride: r * a_stride + row_bytes], b[r * b_stride: r * b_stride + row_bytes])
    return (flag | f) if accumulate else f


def select(idx, flag, want, bump=None):
    """returns (idx, count, bump): idx keeps its words from count on"""
    chosen = np.flatnonzero((flag != 0) == bool(want)).astype(np.uint32)
    idx = idx.copy()
    idx[:len(chosen)] = chosen
    if bump is not None:
        bump = bump.copy()
        bump[chosen] += 1
    return idx, len(chosen), bump


def rows_move(dst, dst_stride, dst_idx, dst_rows, src, src_stride, src_idx, src_rows, row_bytes, dcount, count):
    """dst, src uint8 buffers; dst_idx / src_idx / dcount None or arrays / an int"""
    dst = dst.copy()
    lim = count if dcount is None else min(count, int(dcount))
    for i in range(lim):
        si = i if src_idx is None else int(src_idx[i])
        di = i if dst_idx is None else int(dst_idx[i])
        if si < src_rows and di < dst_rows:
            dst[di * dst_stride: di * dst_stride + row_bytes] = src[si * src_stride: si * src_stride + row_bytes]
    return dst
