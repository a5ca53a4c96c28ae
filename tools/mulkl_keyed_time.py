#!/usr/bin/env python3
"""poly_mul_ntt_kl_round_keyed against poly_mul_ntt_kl_round in one process.

Per set (p-I at k = 4, p-III at k = 5; l = 2, hi only) and batch: HIP events
around single launches, 3 warm-up + 11 timed rounds, median (min - max) in ms.
A round is one launch of each of

  unkeyed    poly_mul_ntt_kl_round on key 0's rows
  one key    keyed, every index 0 (nkeys = 1)
  16 per key keyed, 16 consecutive messages per key (nkeys = batch / 16)
  distinct   keyed, d_key = NULL and nkeys = batch: message b under key b

in that order, so the kernels alternate and a drift of the device reaches all
four alike.  All keys' rows and the inputs are fill_uniform's.  For `distinct`
the rows are read once per message: the algorithmic traffic is
4 k l n (rows) + 4 l n (inputs) + k n (hi) bytes a message, reported as
achieved bytes/s.  The keyed results are compared with the unkeyed call, key by
key where there are few keys, before anything is timed.

  python tools/mulkl_keyed_time.py [--batches 16384,65536]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))

WARMUP, TIMED = 3, 11
SHAPES = {"p-I": (4, 22), "p-III": (5, 24)}   # k, d
L = 2
PER_KEY = 16


def timed_rounds(torch, fns):
    """[(median, min, max)] of each fn, one launch of each per round"""
    ms = [[] for _ in fns]
    for it in range(WARMUP + TIMED):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ms[i].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def run_shape(torch, ntt, dev, ps, batch):
    k, d = SHAPES[ps]
    n = ntt.param_info(ps)["n"]
    ys = [torch.empty(batch * n, dtype=torch.int32, device=dev) for _ in range(L)]
    rows = torch.empty((batch, k, L, n), dtype=torch.int32, device=dev)
    for i, t in enumerate((*ys, rows)):
        ntt.fill_uniform(t, ps, 0x4E7ED00 + i)
    hi = torch.empty((batch, k, n), dtype=torch.int8, device=dev)
    ref = torch.empty_like(hi)
    per16 = (torch.arange(batch, dtype=torch.int32, device=dev) // PER_KEY).contiguous()
    zeros = torch.zeros(batch, dtype=torch.int32, device=dev)
    # correctness first: one key against the unkeyed call; of the other two the first
    # 2 * PER_KEY messages, key by key
    ntt.poly_mul_ntt_kl_round(ys, rows[0], ps, d, hi=ref)
    ntt.poly_mul_ntt_kl_round_keyed(ys, rows[:1], zeros, ps, d, hi=hi)
    assert torch.equal(hi, ref), "one key: keyed differs from unkeyed"
    head = [y[:2 * PER_KEY * n] for y in ys]
    for keys, nkeys, per in ((per16, batch // PER_KEY, PER_KEY), (None, batch, 1)):
        ntt.poly_mul_ntt_kl_round_keyed(ys, rows[:nkeys], keys, ps, d, hi=hi)
        for b0 in range(0, 2 * PER_KEY, per):
            part = [y[b0 * n:(b0 + per) * n] for y in head]
            ntt.poly_mul_ntt_kl_round(part, rows[b0 // per], ps, d, hi=ref[:per])
            assert torch.equal(hi[b0:b0 + per], ref[:per]), f"keyed differs from unkeyed at message {b0}"
    res = timed_rounds(torch, [
        lambda: ntt.poly_mul_ntt_kl_round(ys, rows[0], ps, d, hi=hi),
        lambda: ntt.poly_mul_ntt_kl_round_keyed(ys, rows[:1], zeros, ps, d, hi=hi),
        lambda: ntt.poly_mul_ntt_kl_round_keyed(ys, rows[:batch // PER_KEY], per16, ps, d, hi=hi),
        lambda: ntt.poly_mul_ntt_kl_round_keyed(ys, rows, None, ps, d, hi=hi),
    ])
    (um, ulo, uhi), (om, _, _), (sm, _, _), (dm, _, _) = res
    per_msg = 4 * k * L * n + 4 * L * n + k * n
    print(f"{ps}: k {k}, l {L}, d {d}, hi only, batch {batch}", flush=True)
    for name, (m, lo, up) in zip(("unkeyed", "one key", f"{PER_KEY} per key", "distinct"), res):
        print(f"  {name:12s} {m:8.4f} ms ({lo:.4f} - {up:.4f})  x{m / um:.3f} of unkeyed", flush=True)
    print(f"  one key inside the unkeyed spread: {ulo <= om <= uhi}", flush=True)
    print(f"  distinct: {per_msg} B a message, {per_msg * batch / (dm * 1e-3) / 1e12:.3f} TB/s; "
          f"{(k + L) * batch / (dm * 1e-3) / 1e6:.1f} M transforms/s", flush=True)
    print(f"  {PER_KEY} per key lies {(sm - om) / (dm - om) if dm != om else float('nan'):.3f} of the way "
          "from one key to distinct", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16384,65536")
    args = ap.parse_args()
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "mulkl_keyed_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; HIP events, {WARMUP} warm-up + {TIMED} rounds, "
          "median (min - max)", flush=True)
    for batch in (int(b) for b in args.batches.split(",")):
        assert batch % PER_KEY == 0 and batch >= 2 * PER_KEY
        for ps in SHAPES:
            run_shape(torch, ntt, dev, ps, batch)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
