"""Kernel families per (parameter set, entry point) and the input classes of
tests/test_gpu_family_matrix.py, shared with the CPU tests that pin them
(tests/test_family_cells.py) and with test_gpu_parity.py's switch-boundary
test.  Nothing here names a batch of the switch table: every family-selecting
batch is found by asking the library (ntt_small_batch_max /
ntt_small_batch_radix).
"""
from collections import namedtuple

import numpy as np

from conftest import LARGE_SETS, PARAM_SETS

# Batches above this are not run by the tests (2^20 polynomials: 4 GiB at
# n = 1024, the BASELINE batch).  An in-place n = 1024 transform stays on the
# radix-16 kernels up to the launch-size limit of csrc/ntt_lat.hpp (2^26 - 1
# polynomials), so no batch the tests can allocate reaches its batch kernels
# through the entry points; that switch point is pinned by arithmetic
# (test_family_cells.py::test_launch_size_limit), and the kernels themselves
# (k_ntt_fwd / k_ntt_inv, in place, odd batches included) are launched at small
# batches by the test-only probe library: tests/test_gpu_family_probe.py::
# test_batch_kernel_chunks.
MAX_TEST_BATCH = 1 << 20


def families(ntt, ps, op):
    """[(radix, first batch, last batch)] of entry point `op`, in batch order:
    the one-polynomial-per-workgroup tiers (radix 4 / 8 / 16), each found by
    bisection from its first batch, then the batch kernels (radix 0, no last
    batch)."""
    m = ntt.small_batch_max(ps, op)
    out = []
    lo = 1
    while lo <= m:
        r = ntt.small_batch_radix(ps, op, lo)
        a, b = lo, m + 1          # radix(a) == r, radix(b) != r
        while b - a > 1:
            mid = (a + b) // 2
            if ntt.small_batch_radix(ps, op, mid) == r:
                a = mid
            else:
                b = mid
        out.append((r, lo, a))
        lo = b
    out.append((0, m + 1, None))
    return out


def switch_points(ntt, ps, op):
    """Every batch up to MAX_TEST_BATCH at which entry point `op` changes
    kernel family: the last batch of each tier and the first of the next."""
    pts = set()
    for _, first, last in families(ntt, ps, op)[:-1]:
        if first < MAX_TEST_BATCH:
            pts |= {last, last + 1}
    return sorted(p for p in pts if p <= MAX_TEST_BATCH)


Cell = namedtuple("Cell", "ps op radix batch")


def cell_id(c):
    return f"{c.ps}-{c.op}-{'radix%d' % c.radix if c.radix else 'batch'}"


def cells(ntt):
    """One cell per (parameter set, entry point, family): the smallest batch
    that reaches the family and leaves a ragged tail -- a tier's first batch
    but at least 3; one past the last tier for the batch kernels (7 where
    there is no tier), odd as long as the tiers end on even batches."""
    out = []
    for ps in PARAM_SETS + LARGE_SETS:
        for op in ntt.SWITCH_OPS:
            for radix, first, last in families(ntt, ps, op):
                if radix:
                    batch = max(first, 3)
                    assert batch <= last, (ps, op, radix, first, last)
                else:
                    batch = first if first > 1 else 7
                out.append(Cell(ps, op, radix, batch))
    return out


def reachable(c):
    return c.batch <= MAX_TEST_BATCH


# ---------------------------------------------------------------- inputs
# Row r of an operand is the device generator's row (ntt_fill_uniform: u,
# uniform in [0, q)) rewritten by class r mod K; a product's second operand
# takes class (r + r // K) mod K, so that over K^2 rows every pair of classes
# occurs.  The largest input the header allows comes first (the smallest
# cells have 3 rows).
CLASSES = ("all_2q-1",        # 2q-1 in every coefficient
           "mixed",           # u or u + q by a bit of u: canonical and lazy coefficients in one polynomial
           "plus_q",          # u + q: all in [q, 2q)
           "uniform",         # u
           "zero",
           "all_q-1",
           "first_2q-1",      # 2q-1 at index 0 only
           "last_2q-1",       # 2q-1 at index n-1 only
           "alt_0_2q-1",      # 0, 2q-1, 0, 2q-1, ...
           "alt_2q-1_0",
           "init_operand")    # the reference's operand pattern: n/2 - i for i < n/2, then 0
K = len(CLASSES)
MIXED, PLUS_Q, UNIFORM = 1, 2, 3
FROM_FILL = (MIXED, PLUS_Q, UNIFORM)          # rows that differ from row to row
STRUCTURED = tuple(c for c in range(K) if c not in FROM_FILL)
MIX_BIT = 7                                   # "mixed": + q where this bit of u is set


def templates(n, q):
    """[K, n] uint32: the structured classes' rows (zero rows for the classes
    made from the fill)."""
    t = np.zeros((K, n), np.uint32)
    top = 2 * q - 1
    t[CLASSES.index("all_2q-1")] = top
    t[CLASSES.index("all_q-1")] = q - 1
    t[CLASSES.index("first_2q-1"), 0] = top
    t[CLASSES.index("last_2q-1"), n - 1] = top
    t[CLASSES.index("alt_0_2q-1"), 1::2] = top
    t[CLASSES.index("alt_2q-1_0"), 0::2] = top
    t[CLASSES.index("init_operand"), : n // 2] = n // 2 - np.arange(n // 2)
    return t


def row_classes(rows, second=False):
    """Class of each row index (numpy array or torch tensor)."""
    return (rows + rows // K) % K if second else rows % K


def apply_classes_np(u, rows, q, second=False):
    """The operand's rows `rows`, from the generator's rows u [len(rows), n]."""
    u = np.asarray(u, np.uint32)
    rows = np.asarray(rows, np.int64)
    tm = templates(u.shape[1], q)
    cls = row_classes(rows, second)
    out = u.copy()
    for c in range(K):
        sel = cls == c
        if c == UNIFORM or not sel.any():
            continue
        if c == PLUS_Q:
            out[sel] = u[sel] + np.uint32(q)
        elif c == MIXED:
            out[sel] = u[sel] + np.uint32(q) * ((u[sel] >> MIX_BIT) & 1)
        else:
            out[sel] = tm[c]
    return out


def apply_classes_torch(v, q, second=False):
    """The same rule on a [batch, n] int32 tensor holding the generator's
    rows, in place (2q - 1 < 2^31 for every parameter set)."""
    import torch
    batch, n = v.shape
    tm = torch.from_numpy(templates(n, q).view(np.int32)).to(v.device)
    cls = row_classes(torch.arange(batch, device=v.device), second)
    for c in range(K):
        if c == UNIFORM:
            continue
        sel = (cls == c).nonzero().squeeze(1)
        if sel.numel() == 0:
            continue
        if c == PLUS_Q:
            v[sel] = v[sel] + q
        elif c == MIXED:
            w = v[sel]
            v[sel] = w + q * ((w >> MIX_BIT) & 1)
        else:
            v[sel] = tm[c]
    return v


def reduce_np(x, q):
    x = np.asarray(x, np.uint32)
    return np.where(x >= q, x - np.uint32(q), x).astype(np.uint32)


def host_rows(oracle, ps, seed, rows, batch, second=False):
    """Rows `rows` of the operand made from fill seed `seed`, rebuilt on the host."""
    rows = np.asarray(rows, np.int64)
    if len(rows) == batch:
        u = oracle.fill_uniform(batch, ps, seed, 0)
    else:
        u = np.concatenate([oracle.fill_uniform(1, ps, seed, int(r)) for r in rows])
    return apply_classes_np(u, rows, oracle.params(ps)["q"], second)


def sample_rows(batch, seed):
    """Rows compared with the oracle: all of them up to 4096, else the first
    64, the last 64 and 384 seeded random ones."""
    if batch <= 4096:
        return np.arange(batch)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(64), np.arange(batch - 64, batch), rng.integers(64, batch - 64, 384)]))


def identical_groups(batch, operands):
    """Row-index arrays (two rows or more) whose inputs are identical: every
    operand (a `second` flag each) has the same structured class."""
    rows = np.arange(batch)
    key = np.zeros(batch, np.int64)
    ok = np.ones(batch, bool)
    for second in operands:
        cls = row_classes(rows, second)
        ok &= np.isin(cls, STRUCTURED)
        key = key * K + cls
    groups = []
    for k in np.unique(key[ok]):
        idx = rows[ok & (key == k)]
        if len(idx) > 1:
            groups.append(idx)
    return groups
