"""What tests/test_gpu_family_matrix.py relies on, checked without a GPU: the
cells it enumerates from the library's switch functions cover every reachable
kernel family, its input classes are what the oracle is defined on, and the
one-polynomial-per-workgroup tiers never take a batch whose launch would not
fit (csrc/ntt_lat.hpp).
"""
import json
import os

import numpy as np
import pytest

import family_cells as fc
from conftest import LARGE_SETS, PARAM_SETS

ALL_SETS = PARAM_SETS + LARGE_SETS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "switch_families.json")


def _probes():
    """Batches at which the library is asked for its family, independent of
    the bisection in family_cells.families: every multiple of 256 up to 2^15
    and every power of two up to 2^31, with both neighbours."""
    base = set(range(256, (1 << 15) + 1, 256)) | {1 << k for k in range(32)}
    return sorted(b + d for b in base for d in (-1, 0, 1) if 0 < b + d < (1 << 31))


def test_cells_cover_every_reachable_family(ntt):
    cells = fc.cells(ntt)
    run = [c for c in cells if fc.reachable(c)]
    skipped = {(c.ps, c.op, c.radix) for c in cells if not fc.reachable(c)}
    # MAX_TEST_BATCH is a condition, not a measurement: only the batch kernels
    # of the in-place n = 1024 transforms lie above it
    assert skipped == {(ps, op, 0) for ps in ("ref", "p-I") for op in ("fwd", "inv")}
    have = {(c.ps, c.op, c.radix) for c in cells}
    assert len(have) == len(cells)
    for c in cells:
        assert ntt.small_batch_radix(c.ps, c.op, c.batch) == c.radix, c
        assert c.batch >= 3
        if fc.reachable(c) and c.radix == 0:
            assert c.batch % 2 == 1, f"{c}: an even batch leaves no partial wave"
    # every family any probe batch reaches has a cell, and (outside the
    # skipped set) one that runs
    for ps in ALL_SETS:
        n = ntt.param_info(ps)["n"]
        for op in ntt.SWITCH_OPS:
            assert ntt.small_batch_radix(ps, op, ntt.small_batch_max(ps, op) + 1) == 0
            for b in _probes():
                r = ntt.small_batch_radix(ps, op, b)
                assert (ps, op, r) in have, (ps, op, b, r)
                if b <= fc.MAX_TEST_BATCH:
                    assert (ps, op, r) not in skipped, (ps, op, b, r)
            # and no cell allocates more than the switch-boundary test does
            for c in run:
                if (c.ps, c.op) == (ps, op):
                    assert c.batch * n * 4 <= (1 << 30) + 4 * n * 4, c
    print(f"{len(run)} cells run, {len(skipped)} skipped")
    for c in cells:
        print(f"  {fc.cell_id(c):32s} batch {c.batch}{'' if fc.reachable(c) else '  (skipped)'}")
    assert len(run) == 86


def test_oracle_on_every_input_class(oracle):
    """Each input class, reduced mod q, through the oracle: the forward equals
    the O(n^2) definition and the inverse undoes it (one row per class and per
    operand kind, n = 1024); the torch and numpy statements of the class rule
    agree; every class stays below 2q and every lazy class reaches past q."""
    import torch
    rows = np.arange(fc.K * fc.K + 5)
    for ps in ("ref", "p-I"):
        p = oracle.params(ps)
        n, q = p["n"], p["q"]
        assert n == 1024 and 2 * q - 1 < (1 << 31)
        u = oracle.fill_uniform(len(rows), ps, 0xC1A55, 0)
        for second in (False, True):
            x = fc.apply_classes_np(u, rows, q, second)
            t = torch.from_numpy(u.view(np.int32).copy())
            fc.apply_classes_torch(t, q, second)
            assert np.array_equal(t.numpy().view(np.uint32), x)
            cls = fc.row_classes(rows, second)
            assert set(cls.tolist()) == set(range(fc.K))
            assert x.max() == 2 * q - 1 and np.array_equal(x[cls == fc.UNIFORM], u[cls == fc.UNIFORM])
            assert (x[cls == fc.PLUS_Q] >= q).all()
            mixed = x[cls == fc.MIXED]
            assert ((mixed >= q).any(axis=1) & (mixed < q).any(axis=1)).all()
            xr = fc.reduce_np(x, q)
            assert xr.max() < q and np.array_equal(xr.astype(np.uint64) % q, x.astype(np.uint64) % q)
            one = np.array([np.flatnonzero(cls == c)[0] for c in range(fc.K)])   # one row per class
            X = oracle.poly_ntt(xr[one], ps)
            assert np.array_equal(X, oracle.ntt_direct_np(xr[one], ps))
            assert np.array_equal(oracle.poly_invntt(X, ps), xr[one])
        # both operand rules over K^2 rows: every pair of classes occurs
        pairs = set(zip(fc.row_classes(rows).tolist(), fc.row_classes(rows, True).tolist()))
        assert len(pairs) == fc.K * fc.K
        # the rows a few samples rebuild equal the whole batch's
        some = np.array([0, 7, 12, 100])
        assert np.array_equal(fc.host_rows(oracle, ps, 0xC1A55, some, len(rows)), fc.apply_classes_np(u, rows, q)[some])
    groups = fc.identical_groups(3 * fc.K, [False])
    assert len(groups) == len(fc.STRUCTURED) and all(len(set((g % fc.K).tolist())) == 1 for g in groups)


def test_launch_size_limit(ntt):
    """A one-polynomial-per-workgroup launch has grid = batch and n / radix
    threads (n / 8 for radix 4 at n = 8192), and grid x block must fit 32
    bits: no tier takes a batch above that, so from 2^26 polynomials the
    in-place n = 1024 transforms run the batch kernels.  (Arithmetic only: a
    batch that large is a 256 GiB tensor and is run by no test.)  Below
    MAX_TEST_BATCH every batch keeps the family recorded in
    golden/switch_families.json (the switch points of the round-6 table; to
    be regenerated when a measured sweep moves the table)."""
    for ps in ALL_SETS:
        n = ntt.param_info(ps)["n"]
        for op in ntt.SWITCH_OPS:
            for radix, first, last in fc.families(ntt, ps, op)[:-1]:
                assert last * (n // radix) < 1 << 32, (ps, op, radix, last)
            m = ntt.small_batch_max(ps, op)
            assert ntt.small_batch_radix(ps, op, m + 1) == 0
            assert ntt.small_batch_radix(ps, op, (1 << 31) - 1) == 0
    for ps in ("ref", "p-I"):
        for op in ("fwd", "inv"):
            assert ntt.small_batch_radix(ps, op, (1 << 26) - 1) == 16
            assert ntt.small_batch_radix(ps, op, 1 << 26) == 0
            assert ntt.small_batch_max(ps, op) == (1 << 26) - 1
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert recorded["max_test_batch"] == fc.MAX_TEST_BATCH
    assert set(recorded["families"]) == {f"{ps}/{op}" for ps in ALL_SETS for op in ntt.SWITCH_OPS}
    for key, rec in recorded["families"].items():
        ps, op = key.split("/")
        # the same switch points, so every batch between two of them keeps its family too
        assert fc.switch_points(ntt, ps, op) == rec["switch_points"], key
        assert {1, fc.MAX_TEST_BATCH} | set(rec["switch_points"]) == {b for b, _ in rec["radix_at"]}
        for batch, radix in rec["radix_at"]:
            assert ntt.small_batch_radix(ps, op, batch) == radix, (key, batch)
