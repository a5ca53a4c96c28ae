#!/usr/bin/env python3
"""poly_pack / poly_unpack against poly_round in one process.

Per shape: HIP events around single launches, 3 warm-up + 11 timed, median
(min - max) in ms and the achieved bytes/s of the median, for
  poly_pack, poly_unpack with maxima, poly_unpack without maxima,
  poly_round with hi only (the yardstick: 5 B per coefficient) and with norms
  only, and the pair poly_unpack without maxima + poly_round(norms) that
  poly_unpack with maxima replaces.
Bytes are the algorithm's: 4 + bits / 8 per coefficient for the wire calls
(4 per maximum on top), 5 for poly_round's hi, 4 for its norms.  The rows are
random bytes, the coefficients their unpacked values.

  python tools/pack_bw.py [--shapes sig|key|all] [--batches 131072,1048576]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))

WARMUP, TIMED = 3, 11
# name: param set, k, bits, signed, poly_round's d
SIG = {"p-I sig": ("p-I", 1, 20, True, 22), "p-III sig": ("p-III", 1, 22, True, 24)}
KEY = {"p-I key": ("p-I", 4, 29, False, 22), "p-III key": ("p-III", 5, 30, False, 24)}
KEY_BATCH = 1 << 14


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


def line(what, t, nbytes):
    med, lo, hi = t
    rate = f"{nbytes / med / 1e9:7.3f} TB/s" if nbytes else "             "
    print(f"  {what:<34} {med:8.4f} ms ({lo:.4f} - {hi:.4f})  {rate}", flush=True)
    return nbytes / med / 1e9 if nbytes else None


def run_shape(torch, ntt, dev, name, batch):
    ps, k, bits, signed, d = {**SIG, **KEY}[name]
    n = ntt.param_info(ps)["n"]
    packed = k * n * bits // 8
    coeffs = batch * k * n
    g = torch.Generator(device=dev).manual_seed(batch + bits)
    rows = torch.randint(0, 256, (batch, packed + 32), generator=g, dtype=torch.uint8, device=dev)
    w = torch.empty((batch, k, n), dtype=torch.int32, device=dev)
    out = torch.empty_like(rows)
    mx = torch.empty(batch * k, dtype=torch.int32, device=dev)
    hi = torch.empty(coeffs, dtype=torch.int8, device=dev)
    norms = torch.empty((batch * k, 2), dtype=torch.int32, device=dev)
    ntt.poly_unpack(w, rows, ps, bits, signed=signed)
    ntt.poly_pack(out, w, ps, bits, signed=signed)
    if signed:   # the byte round trip of the definition, at the size that is timed
        assert torch.equal(out[:, :packed], rows[:, :packed]), "poly_pack(poly_unpack(bytes)) != bytes"
    wire = coeffs * (4 + bits / 8)
    print(f"{name}: {ps}, batch {batch}, k {k}, {bits} bits {'signed' if signed else 'unsigned'}, "
          f"stride {packed + 32}, {coeffs} coefficients", flush=True)
    r = {}
    r["pack"] = line("poly_pack", timed(torch, lambda: ntt.poly_pack(out, w, ps, bits, signed=signed)), wire)
    r["unpack_max"] = line("poly_unpack, maxima",
                           timed(torch, lambda: ntt.poly_unpack(w, rows, ps, bits, signed=signed, maxima=mx)), wire + 4 * batch * k)
    r["unpack"] = line("poly_unpack, no maxima", timed(torch, lambda: ntt.poly_unpack(w, rows, ps, bits, signed=signed)), wire)
    r["round"] = line(f"poly_round, hi only (d = {d})", timed(torch, lambda: ntt.poly_round(w, ps, d, hi=hi)), coeffs * 5)
    line("poly_round, norms only", timed(torch, lambda: ntt.poly_round(w, ps, d, norms=norms)), coeffs * 4)

    def pair():
        ntt.poly_unpack(w, rows, ps, bits, signed=signed)
        ntt.poly_round(w, ps, d, norms=norms)
    line("poly_unpack + poly_round(norms)", timed(torch, pair), 0)
    print("  bytes/s against poly_round's: " +
          ", ".join(f"{key} {r[key] / r['round']:.3f}" for key in ("pack", "unpack_max", "unpack")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all", choices=("sig", "key", "all"))
    ap.add_argument("--batches", default="131072,1048576", help="batches of the signature shapes")
    args = ap.parse_args()
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "pack_bw.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; HIP events, {WARMUP} warm-up + {TIMED} launches, "
          "median (min - max)", flush=True)
    if args.shapes in ("sig", "all"):
        for batch in (int(b) for b in args.batches.split(",")):
            for name in SIG:
                run_shape(torch, ntt, dev, name, batch)
                torch.cuda.empty_cache()
    if args.shapes in ("key", "all"):
        for name in KEY:
            run_shape(torch, ntt, dev, name, KEY_BATCH)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
