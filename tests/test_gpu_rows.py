"""ntt_rows_over, ntt_rows_differ, ntt_select and ntt_rows_move on the GPU
against tests/rows_model.py, for equality: every width, row length, alignment
and NULL / non-NULL operand the entry points branch on, values on both sides
of a bound, single flipped bits, index lists with entries out of range, device
counts below, above and equal to zero, sentinels in every word that must not
be written -- and one shape per kernel whose rows outnumber its capped grid,
so that the row loop takes a second step."""
import numpy as np
import pytest
import torch

import rows_model as M

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEF


def to_dev(a, dev):
    """numpy unsigned to a device tensor of the signed dtype of equal width"""
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).to(dev)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def byte_rows(buf, offset, rows, row_bytes, stride):
    """the [rows, row_bytes] view of a flat uint8 device buffer: row r at offset + r stride"""
    return torch.as_strided(buf, (rows, row_bytes), (stride, 1), offset)


# ------------------------------------------------------------------ rows_over

def over_case(width, m, batch):
    """values on both sides of their bounds: (vals, bounds, the type's maximum)"""
    rng = np.random.default_rng(1000 * width + 100 * m + batch)
    dt, top = (np.uint32, (1 << 32) - 1) if width == 32 else (np.uint64, (1 << 64) - 1)
    bounds = [int(x) for x in rng.integers(1, 1 << (width - 2), m)]
    if m > 1:
        bounds[m - 1] = top      # a column that never flags, though it holds the type's maximum itself
    if m > 2:
        bounds[0] = 0            # any non-zero value is over
    # per value: at the bound (not over), one above (over), one below, 0, the maximum, or anything -- the last three
    # rare enough that rows with no value over remain at every m
    kind = rng.choice(6, size=(batch, m), p=[0.5, 0.04, 0.3, 0.1, 0.01, 0.05])
    vals = np.empty((batch, m), dtype=object)
    for j, bound in enumerate(bounds):
        opts = [bound, min(bound + 1, top), max(bound - 1, 0), 0, top, int(rng.integers(0, 1 << 31))]
        vals[:, j] = [opts[t] for t in kind[:, j]]
    return vals.astype(dt), bounds, top, rng


@pytest.mark.parametrize("batch", (1, 65, 1025))
@pytest.mark.parametrize("m", (1, 2, 10, 16))
@pytest.mark.parametrize("width", (32, 64))
def test_rows_over(ntt, dev, width, m, batch):
    vals, bounds, top, rng = over_case(width, m, batch)
    tv = to_dev(vals, dev)
    old = rng.choice(np.array([0, 0, 1, 2, 0x80000000, 5, SENT], dtype=np.uint32), batch)
    want = M.rows_over(old, vals, bounds, False)
    if batch > 1:
        assert want.min() == 0 and want.max() == 1, "the case must hold rows on both sides"
    flag = to_dev(old, dev)                              # garbage that a plain call overwrites
    assert ntt.rows_over(flag, tv, bounds) is flag
    assert np.array_equal(u32(flag), want)
    flag = to_dev(old, dev)                              # earlier flags and foreign bits that accumulate keeps
    ntt.rows_over(flag, tv, bounds, accumulate=True)
    assert np.array_equal(u32(flag), old | want)
    # the maximum as every bound: nothing is over, whatever the values
    ntt.rows_over(flag, tv, [top] * m)
    assert not u32(flag).any()
    if width == 32:                                      # a 64-bit bound above the 32-bit maximum never flags either
        ntt.rows_over(flag, tv, [1 << 40] * m)
        assert not u32(flag).any()
        vals[:] = top
        ntt.rows_over(flag, to_dev(vals, dev), [top - 1] + [top] * (m - 1))
        assert u32(flag).all()


def test_rows_over_shapes_of_the_chain(ntt, dev):
    """[batch][k][2] norms as m = 2 k with alternating bounds, [batch][2] with column 1 skipped, int64 sums"""
    rng = np.random.default_rng(7)
    batch, k = 67, 5
    wn = rng.integers(0, 1000, (batch, k, 2)).astype(np.uint32)
    flag = torch.empty(batch, dtype=torch.int32, device=dev)
    ntt.rows_over(flag, to_dev(wn, dev), [900, 950] * k)
    assert np.array_equal(u32(flag), ((wn[:, :, 0] > 900).any(axis=1) | (wn[:, :, 1] > 950).any(axis=1)).astype(np.uint32))
    zn = rng.integers(0, 1000, (batch, 2)).astype(np.uint32)
    ntt.rows_over(flag, to_dev(zn, dev), [500, (1 << 32) - 1])
    assert np.array_equal(u32(flag), (zn[:, 0] > 500).astype(np.uint32))
    sums = rng.integers(0, 1 << 40, batch).astype(np.uint64)
    ntt.rows_over(flag, to_dev(sums, dev), [1 << 39], accumulate=True)
    assert np.array_equal(u32(flag), ((zn[:, 0] > 500) | (sums > 1 << 39)).astype(np.uint32))


def test_rows_over_more_rows_than_the_grid(ntt, dev):
    batch = 259 * 16 * 256 + 3   # above 16 workgroups of 256 rows for each of up to 259 compute units
    rng = np.random.default_rng(8)
    vals = rng.integers(0, 4, batch).astype(np.uint32)
    flag = torch.full((batch,), 7, dtype=torch.int32, device=dev)
    ntt.rows_over(flag, to_dev(vals, dev), [2])
    assert np.array_equal(u32(flag), (vals > 2).astype(np.uint32))


# ---------------------------------------------------------------- rows_differ

def differ_case(row_bytes, gap_a, gap_b, batch):
    """equal rows with different gap bytes, then single flipped bits: (a, b, strides, offsets, {row: byte}, rng)"""
    rng = np.random.default_rng(row_bytes * 100000 + gap_a * 10 + gap_b + batch)
    sa, sb, off_a, off_b = row_bytes + gap_a, row_bytes + gap_b, 4, 12   # word-aligned bases, not more
    a = rng.integers(0, 256, off_a + batch * sa, dtype=np.uint8)
    b = rng.integers(0, 256, off_b + batch * sb, dtype=np.uint8)         # the gap bytes differ: they must not flag
    for r in range(batch):
        b[off_b + r * sb: off_b + r * sb + row_bytes] = a[off_a + r * sa: off_a + r * sa + row_bytes]
    flipped = {}
    for r in sorted(set(rng.integers(0, batch, max(1, batch // 4)).tolist())):
        where = (0, row_bytes - 1, int(rng.integers(0, row_bytes)))[r % 3]      # the first byte, the last byte, anywhere
        b[off_b + r * sb + where] ^= 1 << int(rng.integers(0, 8))               # a single bit
        flipped[r] = where
    return a, b, sa, sb, off_a, off_b, flipped, rng


@pytest.mark.parametrize("batch", (1, 67, 1025))
@pytest.mark.parametrize("gap_a, gap_b", ((0, 0), (8, 4), (5632, 0)))
@pytest.mark.parametrize("row_bytes", (4, 32, 36))
def test_rows_differ(ntt, dev, row_bytes, gap_a, gap_b, batch):
    a, b, sa, sb, off_a, off_b, flipped, rng = differ_case(row_bytes, gap_a, gap_b, batch)
    if batch >= 3:
        assert {0, row_bytes - 1} <= set(flipped.values())
    old = rng.choice(np.array([0, 0, 1, 2, 0x80000000, SENT], dtype=np.uint32), batch)
    want = M.rows_differ(old, a[off_a:], sa, b[off_b:], sb, row_bytes, False)
    assert np.array_equal(np.flatnonzero(want), np.array(sorted(flipped)))
    ta, tb = to_dev(a, dev), to_dev(b, dev)
    va, vb = byte_rows(ta, off_a, batch, row_bytes, sa), byte_rows(tb, off_b, batch, row_bytes, sb)
    flag = to_dev(old, dev)
    assert ntt.rows_differ(flag, va, vb) is flag
    assert np.array_equal(u32(flag), want)
    flag = to_dev(old, dev)
    ntt.rows_differ(flag, vb, va, accumulate=True)
    assert np.array_equal(u32(flag), old | want)
    ntt.rows_differ(flag, va, va)                         # the inputs may be the same rows: nothing differs
    assert not u32(flag).any()
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)


def test_rows_differ_reads_c_prime_where_it_lies(ntt, dev):
    rng = np.random.default_rng(9)
    batch, zlen = 5, 2560
    sig = torch.from_numpy(rng.integers(0, 256, (batch, zlen + 32), dtype=np.uint8)).to(dev)
    c2 = sig[:, zlen:].clone()
    c2[3, 31] ^= 0x80
    flag = torch.empty(batch, dtype=torch.int32, device=dev)
    ntt.rows_differ(flag, c2, sig[:, zlen:])
    assert flag.tolist() == [0, 0, 0, 1, 0]


def test_rows_differ_more_rows_than_the_grid(ntt, dev):
    batch, row_bytes = 259 * 16 * 4 + 5, 256             # 64 lanes a row, four rows a workgroup
    rng = np.random.default_rng(10)
    a = rng.integers(0, 256, (batch, row_bytes), dtype=np.uint8)
    b = a.copy()
    rows = rng.choice(batch, 500, replace=False)
    b[rows, rng.integers(0, row_bytes, 500)] ^= 4
    b[batch - 1, row_bytes - 1] ^= 1
    flag = torch.empty(batch, dtype=torch.int32, device=dev)
    ntt.rows_differ(flag, to_dev(a, dev), to_dev(b, dev))
    assert np.array_equal(u32(flag), (a != b).any(axis=1).astype(np.uint32))


# --------------------------------------------------------------------- select

PATTERNS = ("zero", "nonzero", "alternating", "random")


def flags_of(pattern, batch, rng):
    if pattern == "zero":
        return np.zeros(batch, dtype=np.uint32)
    if pattern == "nonzero":
        return rng.choice(np.array([1, 2, 0x80000000, SENT], dtype=np.uint32), batch)
    if pattern == "alternating":
        return (np.arange(batch) & 1).astype(np.uint32)
    return rng.choice(np.array([0, 0, 0, 1, 1, 2, 0x80000000, 0xFFFFFFFF], dtype=np.uint32), batch)   # set means not 0


@pytest.mark.parametrize("want", (0, 1))
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("batch", (1, 63, 64, 65, 1023, 1024, 1025, 4097))
def test_select(ntt, dev, batch, pattern, want):
    rng = np.random.default_rng(batch * 10 + PATTERNS.index(pattern) * 2 + want)
    flag = flags_of(pattern, batch, rng)
    idx0 = np.full(batch, SENT, dtype=np.uint32)
    bump0 = rng.integers(0, 256, batch).astype(np.uint32)
    want_idx, want_count, want_bump = M.select(idx0, flag, want, bump0)
    tf = to_dev(flag, dev)
    idx, count, bump = to_dev(idx0, dev), torch.full((1,), -5, dtype=torch.int32, device=dev), to_dev(bump0, dev)
    got = ntt.select(idx, count, tf, want, bump=bump)
    assert got[0] is idx and got[1] is count
    assert int(count) == want_count
    assert np.array_equal(u32(idx), want_idx)             # ascending, and the tail keeps its sentinel
    assert np.array_equal(u32(bump), want_bump)           # raised only where selected
    assert np.array_equal(u32(tf), flag)
    # without bump, and with want as a bool: the same list
    idx2, count2 = to_dev(idx0, dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ntt.select(idx2, count2, tf, bool(want))
    assert int(count2) == want_count and torch.equal(idx2, idx)


# ------------------------------------------------------------------ rows_move

def move_case(ntt, dev, rng, row_bytes, wide, dst_rows, src_rows, count, use_dst_idx, use_src_idx, dcount):
    """one ntt_rows_move against the model: the whole of both buffers is compared, so every stride gap, every
    unselected dst row and the bytes before the first row keep their random sentinels"""
    if wide:       # bases, strides and the row are multiples of 16
        assert row_bytes % 16 == 0
        ds, ss, off_d, off_s = row_bytes + 16, row_bytes + 32, 16, 0
    else:          # multiples of 4 and no more, in at least one operand
        ds, ss, off_d, off_s = row_bytes + 4, row_bytes + (8 if row_bytes % 16 else 0), 4, 8
    dst = rng.integers(0, 256, off_d + dst_rows * ds, dtype=np.uint8)
    src = rng.integers(0, 256, off_s + src_rows * ss, dtype=np.uint8)
    di = rng.permutation(dst_rows + 5)[:count].astype(np.uint32) if use_dst_idx else None     # distinct, some out of range
    si = rng.integers(0, src_rows + 4, count).astype(np.uint32) if use_src_idx else None      # some out of range
    if use_dst_idx and count > 2:
        di[1] = 0xFFFFFFFF
    if use_src_idx and count > 3:
        si[2] = 1 << 31
    want = M.rows_move(dst[off_d:], ds, di, dst_rows, src[off_s:], ss, si, src_rows, row_bytes, dcount, count)
    td, ts = to_dev(dst, dev), to_dev(src, dev)
    vd, vs = byte_rows(td, off_d, dst_rows, row_bytes, ds), byte_rows(ts, off_s, src_rows, row_bytes, ss)
    kw = {}
    if use_dst_idx:
        kw["dst_idx"] = to_dev(di, dev)
    if use_src_idx:
        kw["src_idx"] = to_dev(si, dev)
    if dcount is not None:
        kw["count"] = torch.tensor([dcount], dtype=torch.int32, device=dev)
    assert ntt.rows_move(vd, vs, n=count, **kw) is vd
    got = td.cpu().numpy()
    assert np.array_equal(got[:off_d], dst[:off_d])
    assert np.array_equal(got[off_d:], want), (row_bytes, wide, use_dst_idx, use_src_idx, dcount)
    assert np.array_equal(ts.cpu().numpy(), src)
    return int((got != dst).any())


@pytest.mark.parametrize("row_bytes, wide", ((4, False), (12, False), (16, False), (16, True), (36, False), (5664, False),
                                             (5664, True)))   # 16-byte operands where the row allows them
def test_rows_move(ntt, dev, row_bytes, wide):
    rng = np.random.default_rng(row_bytes * 2 + wide)
    moved = 0
    for use_dst_idx in (False, True):
        for use_src_idx in (False, True):
            # the device's count NULL, below the host's, above it, and 0
            for dcount in (None, 17, 1000, 0):
                moved += move_case(ntt, dev, rng, row_bytes, wide, 41, 37, 29, use_dst_idx, use_src_idx, dcount)
            # the host's count above both sides' rows: the identity skips what is out of range too
            move_case(ntt, dev, rng, row_bytes, wide, 41, 37, 45, use_dst_idx, use_src_idx, None)
    assert moved >= 12    # every case but dcount = 0 moved something
    move_case(ntt, dev, rng, row_bytes, wide, 1, 1, 1, True, True, 1)


def test_rows_move_many_blocks(ntt, dev):
    rng = np.random.default_rng(11)
    move_case(ntt, dev, rng, 12, False, 3100, 3000, 3000, True, True, 2999)
    move_case(ntt, dev, rng, 32, True, 3100, 3000, 3000, True, False, None)


def test_rows_move_more_rows_than_the_grid(ntt, dev):
    rng = np.random.default_rng(12)
    rows = 259 * 16 + 7          # one 4096-byte row a workgroup, above 16 workgroups per compute unit
    move_case(ntt, dev, rng, 4096, True, rows + 3, rows, rows, True, True, rows - 1)


def test_rows_move_other_dtypes_and_views(ntt, dev):
    """one int32 per row (nonces), int32 rows into byte rows, and a column view of wider rows (z and c' of a signature row)"""
    nonces = torch.arange(10, 20, dtype=torch.int32, device=dev)
    out = torch.full((6,), -1, dtype=torch.int32, device=dev)
    idx = torch.tensor([4, 0, 9], dtype=torch.int32, device=dev)
    ntt.rows_move(out, nonces, src_idx=idx)
    assert out.tolist() == [14, 10, 19, -1, -1, -1]
    ntt.rows_move(out, nonces, dst_idx=torch.tensor([5, 3], dtype=torch.int32, device=dev))
    assert out.tolist() == [14, 10, 19, 11, -1, 10]
    sig = torch.zeros((4, 72), dtype=torch.uint8, device=dev)
    c1 = torch.arange(3 * 32, dtype=torch.uint8, device=dev).view(3, 32)
    ntt.rows_move(sig[:, 40:], c1, dst_idx=torch.tensor([3, 1, 0], dtype=torch.int32, device=dev))
    assert torch.equal(sig[[3, 1, 0], 40:], c1) and not bool(sig[:, :40].any()) and not bool(sig[2].any())
    cp = torch.empty((4, 32), dtype=torch.uint8, device=dev)
    ntt.rows_move(cp, sig[:, 40:])                            # no lists: a strided row copy
    assert torch.equal(cp, sig[:, 40:])
    words = torch.empty((4, 8), dtype=torch.int32, device=dev)
    ntt.rows_move(words, cp)
    assert torch.equal(words.view(torch.uint8), cp)
