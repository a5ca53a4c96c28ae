#!/usr/bin/env python3
"""What a caller without ntt_xof has to do: download
the hi bytes of a batch and hash them on the host.  Times the two parts for
qTESLA's H shapes -- the device -> host copy of [batch][k n] bytes into pinned
memory, and hashlib's SHAKE over hi || a 64-byte digest on `--threads`
threads (hashlib releases the GIL for these lengths) -- and checks ntt_xof's
output against the host digests on the way.

  python tools/xof_host_baseline.py [--batch 131072] [--threads 16] [--reps 3]
"""
import argparse
import hashlib
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ntt-gpu-qtesla_amd")]

SHAPES = (("p-I", "shake128", 4 * 1024), ("p-III", "shake256", 5 * 2048))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 17)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import ntt_amd
    dev = torch.device("cuda:0")
    for ps, algo, hlen in SHAPES:
        g = torch.Generator(device=dev).manual_seed(hlen)
        hi = torch.randint(0, 256, (a.batch, hlen), generator=g, dtype=torch.uint8, device=dev)
        G = torch.randint(0, 256, (a.batch, 64), generator=g, dtype=torch.uint8, device=dev)
        out = torch.empty((a.batch, 32), dtype=torch.uint8, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t_dev = []
        for _ in range(a.reps + 1):
            ev[0].record()
            ntt_amd.xof(out, hi, G, algo=algo)
            ev[1].record()
            ev[1].synchronize()
            t_dev.append(ev[0].elapsed_time(ev[1]))
        host_hi = torch.empty((a.batch, hlen), dtype=torch.uint8).pin_memory()
        host_G = G.cpu().numpy()
        t_copy, t_hash = [], []
        fn = getattr(hashlib, algo.replace("shake", "shake_"))
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_hi.copy_(hi)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rows = host_hi.numpy()

            def chunk(r):
                return [fn(rows[b].tobytes() + host_G[b].tobytes()).digest(32) for b in r]

            step = -(-a.batch // (4 * a.threads))
            with ThreadPoolExecutor(a.threads) as ex:
                parts = list(ex.map(chunk, [range(i, min(i + step, a.batch)) for i in range(0, a.batch, step)]))
            t2 = time.perf_counter()
            t_copy.append((t1 - t0) * 1e3)
            t_hash.append((t2 - t1) * 1e3)
        digests = b"".join(d for p in parts for d in p)
        same = out.cpu().numpy().tobytes() == digests
        med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
        print(f"{ps} {algo} batch {a.batch} x ({hlen} + 64) bytes: ntt_xof {med(t_dev[1:]):.3f} ms | host: copy "
              f"{med(t_copy):.1f} ms ({a.batch * hlen / med(t_copy) / 1e6:.1f} GB/s) + hashlib on {a.threads} threads "
              f"{med(t_hash):.1f} ms = {med(t_copy) + med(t_hash):.1f} ms | device == host digests: {same}")
        if not same:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
