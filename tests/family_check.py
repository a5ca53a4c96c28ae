"""The per-buffer checks that tests/test_gpu_family_matrix.py and
tests/test_gpu_family_probe.py share: one batch's shapes, its operands made on
the device by family_cells' class rule and rebuilt on the host, guarded output
buffers, and every check of one output buffer against the oracle's rows."""
import numpy as np
import torch

import family_cells as fc

GUARD = int(np.uint32(0xA5A5A5A5).view(np.int32))


class Ctx:
    """One cell's shapes, sampled rows and checks.  `cell` has ps, op and
    batch; `seed`: the fill seed of the first operand (default: by the batch)."""

    def __init__(self, ntt, oracle, dev, cell, seed=None):
        self.ntt, self.oracle, self.dev = ntt, oracle, dev
        self.ps, self.op, self.batch = cell.ps, cell.op, cell.batch
        info = ntt.param_info(cell.ps)
        self.n, self.q = info["n"], info["q"]
        self.seed = 0xFA3117 + 2 * cell.batch if seed is None else seed
        self.rows = fc.sample_rows(cell.batch, self.seed)
        self.ri = torch.as_tensor(self.rows, device=dev)

    def operand(self, seed, second=False):
        """Device operand [batch * n] and its sampled rows reduced mod q (host)."""
        t = torch.empty(self.batch * self.n, dtype=torch.int32, device=self.dev)
        self.ntt.fill_uniform(t, self.ps, seed)
        fc.apply_classes_torch(t.view(self.batch, self.n), self.q, second)
        h = fc.host_rows(self.oracle, self.ps, seed, self.rows, self.batch, second)
        assert np.array_equal(self.ntt.to_numpy_u32(t.view(self.batch, self.n)[self.ri]), h), "device / host input rule"
        return t, fc.reduce_np(h, self.q)

    def guarded(self):
        """A [batch * n] view with one polynomial of guard words on each side."""
        buf = torch.full(((self.batch + 2) * self.n,), GUARD, dtype=torch.int32, device=self.dev)
        return buf, buf[self.n:-self.n]

    def reduced(self, t):
        return torch.where(t >= self.q, t - self.q, t)

    def check(self, what, buf, out, want, operands):
        """Every check of one output buffer; all that fail are reported together."""
        n, q = self.n, self.q
        failed = []
        if not bool((buf[:n] == GUARD).all()):
            failed.append("store below the output buffer")
        if not bool((buf[-n:] == GUARD).all()):
            failed.append("store past the output buffer")
        lo, hi = int(out.min()), int(out.max())
        if not (0 <= lo and hi < q):
            failed.append(f"output word outside [0, q): int32 range [{lo}, {hi}], q = {q}")
        o = out.view(self.batch, n)
        got = self.ntt.to_numpy_u32(o[self.ri])
        bad = np.flatnonzero((got != want).any(axis=1))
        if bad.size:
            classes = sorted({fc.CLASSES[c] for c in fc.row_classes(self.rows[bad]).tolist()})
            failed.append(f"{bad.size} of {len(self.rows)} compared rows differ from the oracle, first rows "
                          f"{self.rows[bad[:8]].tolist()}, first operand's classes {classes}")
        for idx in fc.identical_groups(self.batch, operands):
            g = torch.as_tensor(idx, device=self.dev)
            if not bool((o[g[1:]] == o[g[0]]).all()):
                failed.append(f"identical inputs (row {idx[0]}) gave different rows")
        assert not failed, f"{what}: " + "; ".join(failed)
