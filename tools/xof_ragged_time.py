#!/usr/bin/env python3
"""ntt_xof_ragged against ntt_xof and against itself in one process.

SHAKE256, 64 bytes out, per batch: HIP events around single launches, 3 warm-up
+ 11 timed, median (min - max) in ms, for
  (a) the ragged path itself: equal messages of 1 088 bytes (8 rate blocks) at
      8-aligned offsets, through ntt_xof and through ntt_xof_ragged on the same
      bytes; the ratio is ragged / ntt_xof
  (b) realignment: the same messages at offsets shifted by 1 and by 7 bytes,
      against (a)'s ragged time
  (c) divergence: lengths uniform in [0, 2 176] in random order against the
      same messages sorted by length
and the host path a caller has without it (as tools/xof_host_baseline.py):
hashlib on `--threads` threads over (c)'s batch in host memory, plus the upload
of the [batch][64] digests.  Every launch's digests are checked on the way:
(a) ragged == ntt_xof, (b) == (a), (c) sorted == random permuted, and the host
digests == (c)'s.

  python tools/xof_ragged_time.py [--batches 131072,1048576] [--threads 16] [--host-reps 3]
"""
import argparse
import hashlib
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))

WARMUP, TIMED = 3, 11
ALGO, RATE, OUTLEN = "shake256", 136, 64
EQUAL_LEN = 8 * RATE      # (a), (b)
MAX_LEN = 16 * RATE       # (c)


def timed(torch, fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def show(name, t, base=None, base_name=""):
    ratio = "" if base is None else f"  {t[0] / base[0]:.3f} x {base_name}"
    print(f"  {name:<44}{t[0]:9.4f} ms ({t[1]:.4f} - {t[2]:.4f}){ratio}", flush=True)


def padded(torch, body, front):
    """`front` zero bytes, the body, zero bytes up to a multiple of 8"""
    n = front + body.numel()
    buf = torch.zeros(n + (-n) % 8, dtype=torch.uint8, device=body.device)
    buf[front:n] = body
    return buf


def run_batch(torch, np, ntt, dev, batch, threads, host_reps):
    g = torch.Generator(device=dev).manual_seed(batch)
    print(f"batch {batch}:", flush=True)
    # (a) equal lengths, aligned
    body = torch.randint(0, 256, (batch * EQUAL_LEN,), generator=g, dtype=torch.uint8, device=dev)
    off = torch.arange(batch + 1, dtype=torch.int64, device=dev) * EQUAL_LEN
    want = torch.empty((batch, OUTLEN), dtype=torch.uint8, device=dev)
    got = torch.empty_like(want)
    t_xof = timed(torch, lambda: ntt.xof(want, body.view(batch, EQUAL_LEN), algo=ALGO))
    t_rag = timed(torch, lambda: ntt.xof_ragged(got, body, off, algo=ALGO))
    t_xof2 = timed(torch, lambda: ntt.xof(want, body.view(batch, EQUAL_LEN), algo=ALGO))   # either side of the ragged run
    assert torch.equal(got, want), "(a): ntt_xof_ragged differs from ntt_xof"
    show(f"(a) ntt_xof, {EQUAL_LEN} bytes each", t_xof)
    show("(a) ntt_xof_ragged, the same bytes", t_rag, t_xof, "ntt_xof")
    show("(a) ntt_xof again", t_xof2, t_xof, "ntt_xof")
    # (b) the same messages, every start shifted
    for shift in (1, 7):
        msg = padded(torch, body, shift)
        offs = off + shift
        got.zero_()
        t = timed(torch, lambda: ntt.xof_ragged(got, msg, offs, algo=ALGO))
        assert torch.equal(got, want), f"(b): shift {shift} changes the digests"
        show(f"(b) offsets shifted by {shift}", t, t_rag, "(a) ragged")
        del msg
    del body
    # (c) uneven lengths: random order against sorted by length
    lengths = torch.randint(0, MAX_LEN + 1, (batch,), generator=g, dtype=torch.int64, device=dev)
    off_r = torch.zeros(batch + 1, dtype=torch.int64, device=dev)
    off_r[1:] = lengths.cumsum(0)
    total = int(off_r[-1])
    msg_r = padded(torch, torch.randint(0, 256, (total,), generator=g, dtype=torch.uint8, device=dev), 0)
    order = torch.argsort(lengths, stable=True)
    off_s = torch.zeros_like(off_r)
    off_s[1:] = lengths[order].cumsum(0)
    # the sorted buffer: byte i of sorted message j is byte i of message order[j]
    owner = torch.repeat_interleave(torch.arange(batch, device=dev), lengths[order])
    src = off_r[order][owner] + (torch.arange(total, device=dev) - off_s[owner])
    msg_s = padded(torch, msg_r[src], 0)
    del owner, src
    out_r = torch.empty((batch, OUTLEN), dtype=torch.uint8, device=dev)
    out_s = torch.empty_like(out_r)
    t_r = timed(torch, lambda: ntt.xof_ragged(out_r, msg_r, off_r, algo=ALGO))
    t_s = timed(torch, lambda: ntt.xof_ragged(out_s, msg_s, off_s, algo=ALGO))
    assert torch.equal(out_s, out_r[order]), "(c): sorting the messages changes their digests"
    show(f"(c) lengths 0 .. {MAX_LEN}, sorted by length", t_s)
    show(f"(c) lengths 0 .. {MAX_LEN}, random order", t_r, t_s, "sorted")
    # the host path: hashlib over the same batch in host memory, then the digests' upload
    host = msg_r.cpu().numpy()
    offs = off_r.cpu().numpy()
    digests = torch.empty((batch, OUTLEN), dtype=torch.uint8).pin_memory()
    view = digests.numpy()
    up = torch.empty_like(out_r)
    t_hash, t_copy = [], []
    for _ in range(host_reps):
        def chunk(r):
            for b in r:
                view[b] = np.frombuffer(hashlib.shake_256(host[offs[b]:offs[b + 1]]).digest(OUTLEN), dtype=np.uint8)

        step = -(-batch // (4 * threads))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(chunk, [range(i, min(i + step, batch)) for i in range(0, batch, step)]))
        t1 = time.perf_counter()
        up.copy_(digests)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_hash.append((t1 - t0) * 1e3)
        t_copy.append((t2 - t1) * 1e3)
    assert torch.equal(up, out_r), "host digests differ from the device's"
    h, c = statistics.median(t_hash), statistics.median(t_copy)
    print(f"  host: hashlib on {threads} threads {h:.1f} ms ({h / batch * 1e3:.2f} us a message) + upload of the digests "
          f"{c:.2f} ms = {h + c:.1f} ms, {(h + c) / t_r[0]:.0f} x (c) random order; device == host digests: True", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="131072,1048576")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "xof_ragged_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; {ALGO}, {OUTLEN} bytes out; HIP events, "
          f"{WARMUP} warm-up + {TIMED} launches, median (min - max)", flush=True)
    for batch in (int(b) for b in args.batches.split(",")):
        run_batch(torch, np, ntt, dev, batch, args.threads, args.host_reps)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
