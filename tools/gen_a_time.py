#!/usr/bin/env python3
"""poly_gen_a against ntt_xof's per-permutation time in one process.

Per shape and batch: HIP events around single launches, 3 warm-up + 11 timed,
median (min - max) in ms, for
  poly_gen_a at qTESLA's (k, nblocks), dense output, 32-byte seeds, and
  ntt_xof as cshake128_simple(cstm = 0) of XOF_BLOCKS whole rate blocks to 8
  bytes, which is XOF_BLOCKS + 2 permutations a message (the prefix block, the
  blocks, the padding block): the yardstick's ms per permutation at that batch.
A key costs nblocks + 1 + 2 * refills permutations (two to start the first
call, one per further block, two per refill); the yardstick takes the largest
refill count in the batch, since a wave runs until its last lane is done.  The
batch is tests/keccak_model.seeds(8) repeated, so that count comes from the CPU
model (tests/gen_a_model.py) and the first eight keys are compared with it,
every other key with its copy among them.

  python tools/gen_a_time.py [--batches 16384,65536]
"""
import argparse
import functools
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, TIMED = 3, 11
SHAPES = {"p-I": (4, 108), "p-III": (5, 180)}   # k, nblocks (qTESLA's PARAM_GEN_A)
NSEEDS = 8
XOF_BLOCKS = 48


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


@functools.lru_cache(maxsize=None)
def model(k, n, q, nblocks):
    """(the keys of the fixed seeds, their refill counts) by the CPU model"""
    import gen_a_model as M
    import keccak_model as K
    want, refills = [], []
    for sd in K.seeds(NSEEDS):
        st = {}
        want.append(M.gen_a(sd, k, n, q, nblocks, st))
        refills.append(st["refills"])
    return want, refills


def run_shape(torch, np, ntt, dev, ps, batch):
    import keccak_model as K
    k, nblocks = SHAPES[ps]
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    seeds = K.seeds(NSEEDS)
    want, refills = model(k, n, q, nblocks)
    sd = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(NSEEDS, 32)
    ts = torch.from_numpy(np.tile(sd, (batch // NSEEDS, 1))).to(dev)
    a = torch.empty((batch, k, n), dtype=torch.int32, device=dev)
    ntt.poly_gen_a(a, ts, ps, nblocks, k)
    first = ntt.to_numpy_u32(a[:NSEEDS])
    assert np.array_equal(first, np.array(want, dtype=np.uint32)), "poly_gen_a differs from the model"
    assert torch.equal(a.view(batch // NSEEDS, NSEEDS, k, n), a[:NSEEDS].expand(batch // NSEEDS, NSEEDS, k, n)), \
        "equal seeds, different keys"
    perms = nblocks + 1 + 2 * max(refills)
    msg = torch.zeros((batch, 168 * XOF_BLOCKS), dtype=torch.uint8, device=dev)
    msg[:, :32] = ts
    out = torch.empty((batch, 8), dtype=torch.uint8, device=dev)
    gm, glo, ghi = timed(torch, lambda: ntt.poly_gen_a(a, ts, ps, nblocks, k))
    xm, xlo, xhi = timed(torch, lambda: ntt.xof(out, msg, algo="shake128", cstm=0))
    per = xm / (XOF_BLOCKS + 2)
    print(f"{ps}: k {k}, nblocks {nblocks}, batch {batch}, refills {refills} -> {perms} permutations", flush=True)
    print(f"  poly_gen_a                         {gm:8.4f} ms ({glo:.4f} - {ghi:.4f})", flush=True)
    print(f"  ntt_xof, {XOF_BLOCKS + 2} permutations           {xm:8.4f} ms ({xlo:.4f} - {xhi:.4f})  "
          f"{per * 1e3:.3f} us per permutation", flush=True)
    print(f"  yardstick {perms * per:8.4f} ms; measured / yardstick {gm / (perms * per):.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16384,65536")
    args = ap.parse_args()
    import numpy as np
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "gen_a_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    print(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; HIP events, {WARMUP} warm-up + {TIMED} launches, "
          "median (min - max)", flush=True)
    for batch in (int(b) for b in args.batches.split(",")):
        assert batch % NSEEDS == 0
        for ps in SHAPES:
            run_shape(torch, np, ntt, dev, ps, batch)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
