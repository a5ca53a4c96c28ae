#!/usr/bin/env python3
"""The wave-cooperative SHAKE kernels against the one-message-per-lane kernels in one process
(DESIGN.md §5q): the sweep the switch ntt_xof_small_batch_max is set from.

Per shape and batch, path="lane" and path="wave" alternate on one stream: 3
warm-up rounds, then 11 rounds of one launch each between HIP events; median
(min - max) in ms and the ratio wave / lane of the medians.  A row is marked
`wave` when the wave median lies below the lane path's whole range (§5g's
criterion).  Shapes: p-I's H (SHAKE128, 4096 + 64 bytes, 32 out), p-III's H
(SHAKE256, 10240 + 64 bytes, 32 out), a one-block message (64 bytes in, 64
out) with both algorithms; each through xof and, as equal-length messages back
to back, through xof_ragged.  The two paths' digests are compared on the way.

  python tools/xof_wave_time.py [--batches 1,2,64,1024,...] [--shapes H-I,H-III,one128,one256] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))

WARMUP, TIMED = 3, 11
SHAPES = {   # name: algo, len0, len1, outlen
    "H-I": ("shake128", 4096, 64, 32),
    "H-III": ("shake256", 10240, 64, 32),
    "one128": ("shake128", 64, 0, 64),
    "one256": ("shake256", 64, 0, 64),
}
BATCHES = "1,2,64,1024,4096,8192,16384,32768,65536,131072"


def alternate(torch, fns):
    """the callables in turn on the current stream: WARMUP rounds, then TIMED rounds of one timed launch each"""
    ms = [[] for _ in fns]
    for rnd in range(WARMUP + TIMED):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rnd >= WARMUP:
                ms[i].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default=BATCHES)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "xof_wave_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; HIP events, lane / wave alternating, "
        f"{WARMUP} warm-up + {TIMED} rounds, median (min - max) ms")
    say("switch: " + ", ".join(f"{a}{' ragged' if r else ''} {ntt.xof_small_batch_max(a, ragged=r)}"
                               for a in ("shake128", "shake256") for r in (False, True)))
    batches = [int(b) for b in args.batches.split(",")]
    for name in args.shapes.split(","):
        algo, len0, len1, outlen = SHAPES[name]
        total = len0 + len1
        for ragged in (False, True):
            say(f"{name}{' ragged' if ragged else ''}: {algo}, {len0} + {len1} bytes in, {outlen} out")
            say(f"  {'batch':>7}  {'lane':>30}  {'wave':>30}  wave/lane")
            for batch in batches:
                g = torch.Generator(device=dev).manual_seed(batch)
                body = torch.randint(0, 256, (batch, total), generator=g, dtype=torch.uint8, device=dev)
                in0, in1 = body[:, :len0].contiguous(), (body[:, len0:].contiguous() if len1 else None)
                off = torch.arange(batch + 1, dtype=torch.int64, device=dev) * total
                outs = {p: torch.empty((batch, outlen), dtype=torch.uint8, device=dev) for p in ("lane", "wave")}
                if ragged:
                    flat = body.view(-1)
                    fns = [lambda p=p: ntt.xof_ragged(outs[p], flat, off, algo=algo, path=p) for p in outs]
                else:
                    fns = [lambda p=p: ntt.xof(outs[p], in0, in1, algo=algo, path=p) for p in outs]
                lane, wave = alternate(torch, fns)
                assert torch.equal(outs["lane"], outs["wave"]), f"{name} batch {batch}: the paths' digests differ"
                mark = "wave" if wave[0] < lane[1] else ("lane" if lane[0] < wave[1] else "-")
                say(f"  {batch:>7}  {lane[0]:9.4f} ({lane[1]:.4f} - {lane[2]:.4f})  {wave[0]:9.4f} ({wave[1]:.4f} - {wave[2]:.4f})"
                    f"  {wave[0] / lane[0]:8.3f}  {mark}")
                del body, in0, in1, outs
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
