#!/usr/bin/env python3
"""poly_sample_gauss and poly_hsum beside their yardsticks in one process.

Per qTESLA shape (p-I: SHAKE128, 77 x 2 table; p-III: SHAKE256, 110 x 4) and
batch of polynomials: HIP events around single launches, 3 warm-up + 11 timed
rounds, median (min - max) in ms.  A round is one launch of each of

  gauss      poly_sample_gauss, batch polynomials = batch * n / 512 lanes
  xof        ntt_xof with as many lanes, each absorbing a message of P - 2
             rate blocks to 8 bytes under cshake*_simple: P permutations, the
             sampler's count per lane (prefix, seed, and the squeezed blocks
             after the first), so gauss - xof is what the compares and the
             stores cost over the bare permutation chain (xof reads its
             message instead: P - 2 rate blocks a lane)
  sample_y   poly_sample_y at the same batch and the set's bits
  hsum       poly_hsum of the sampler's output at the set's h
  round      poly_round, norms only, of the same data: one read of it, hsum's floor

in that order.  The sampler's first eight polynomials are compared with
tests/gauss_model.py and hsum with a sort before anything is timed.  The text
goes to stdout and to --out (default profiles/gauss/gauss_time.txt).

  python tools/gauss_time.py [--batches 1024,16384] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, TIMED = 3, 11
SHAPES = {"p-I": ("shake128", 77, 2, 25, 20, 22), "p-III": ("shake256", 110, 4, 40, 22, 24)}   # hash, rows, cols, h, bits, d
RATE = {"shake128": 168, "shake256": 136}
NSEEDS = 8


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


def run_shape(torch, np, ntt, dev, ps, batch, say):
    import gauss_model as G
    import keccak_model as K
    algo, rows, cols, h, bits, d = SHAPES[ps]
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    lanes = batch * n // ntt.GAUSS_CHUNK
    blocks = -(-ntt.GAUSS_CHUNK * cols * 4 // RATE[algo])
    perms = blocks + 1   # prefix, seed (gives block 1), one more for every further block
    table = G.cdt_table(8.5, rows, cols)
    cdt = ntt.from_numpy_u32(np.array(table, dtype=np.uint32), dev)
    fixed = K.seeds(NSEEDS)
    sd = np.frombuffer(b"".join(fixed[b % NSEEDS] for b in range(batch)), dtype=np.uint8).reshape(batch, 32)
    seeds = torch.from_numpy(sd.copy()).to(dev)
    out = torch.empty((batch, n), dtype=torch.int32, device=dev)
    y = torch.empty_like(out)
    sums = torch.empty(batch, dtype=torch.int64, device=dev)
    norms = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    msg = torch.zeros((lanes, (perms - 2) * RATE[algo]), dtype=torch.uint8, device=dev)
    dig = torch.empty((lanes, 8), dtype=torch.uint8, device=dev)
    # correctness first
    ntt.poly_sample_gauss(out, seeds, cdt, ps, algo=algo)
    got = ntt.to_numpy_u32(out).reshape(batch, n)
    for b in range(NSEEDS):
        want = np.array(G.sample_gauss(fixed[b], n, q, table, cols, algo, 0), dtype=np.uint32)
        assert np.array_equal(got[b], want), f"polynomial {b} differs from the model"
    assert np.array_equal(got[NSEEDS:], got[np.arange(NSEEDS, batch) % NSEEDS]), "a later polynomial is not its seed's copy"
    ntt.poly_hsum(sums, out, ps, h)
    a = np.sort(np.minimum(got[:NSEEDS].astype(np.int64), q - got[:NSEEDS].astype(np.int64)), axis=1)[:, n - h:].sum(axis=1)
    assert sums.cpu().numpy()[:NSEEDS].tolist() == a.tolist(), "hsum differs from the sort"
    res = timed_rounds(torch, [
        lambda: ntt.poly_sample_gauss(out, seeds, cdt, ps, algo=algo),
        lambda: ntt.xof(dig, msg, algo=algo, cstm=0),
        lambda: ntt.poly_sample_y(y, seeds, ps, bits, algo=algo),
        lambda: ntt.poly_hsum(sums, out, ps, h),
        lambda: ntt.poly_round(out, ps, d, norms=norms),
    ])
    say(f"{ps}: {algo}, table {rows} x {cols}, batch {batch} polynomials = {lanes} lanes, {perms} permutations a lane")
    for name, (m, lo, up) in zip(("gauss", "xof", "sample_y", "hsum", "round"), res):
        say(f"  {name:9s} {m:8.4f} ms ({lo:.4f} - {up:.4f})")
    gm, xm, hm, rm = res[0][0], res[1][0], res[3][0], res[4][0]
    say(f"  gauss / xof {gm / xm:.3f}; per permutation {1e3 * xm / perms:.2f} us (xof), {1e3 * gm / perms:.2f} us (gauss); "
        f"{batch * n / (gm * 1e-3) / 1e9:.3f} G samples/s")
    say(f"  hsum / round {hm / rm:.3f}; hsum reads {4 * n * batch / (hm * 1e-3) / 1e12:.3f} TB/s, round {4 * n * batch / (rm * 1e-3) / 1e12:.3f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss", "gauss_time.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "gauss_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; HIP events, {WARMUP} warm-up + {TIMED} rounds, "
            "median (min - max)")
        for batch in (int(b) for b in args.batches.split(",")):
            assert batch >= NSEEDS
            for ps in SHAPES:
                run_shape(torch, np, ntt, dev, ps, batch, say)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
