#!/usr/bin/env python3
"""poly_unpack_ntt beside the launches it replaces, in one process.

Per qTESLA shape (p-I: k = 4, 29-bit fields; p-III: k = 5, 30-bit fields;
unsigned, negated, pstride = 2 n: slot 1 of the verification rows) and number
of keys: HIP events around single launches, 3 warm-up + 11 timed rounds,
median (min - max) in ms.  A round is one launch of each of

  fused     poly_unpack_ntt, key bytes to q - t-hat in the rows
  unpack    poly_unpack into a [keys, k, n] temporary
  ntt       poly_ntt of that temporary, in place
  negate    rows[:, :, 1, :] = q - t, the torch expression of the round trips
  ntt_oop   poly_ntt_oop alone: a pass that reads 4 n and writes 4 n bytes a
            polynomial, the reference for fused's 30 n / 8 + 4 n

in that order, so every leg meets the cache as the others left it.  Before
anything is timed the fused rows are compared with the chain's modulo q and
the maxima with poly_unpack's.  The text goes to stdout and to --out (default
profiles/unpack_ntt/unpack_ntt_time.txt).

  python tools/unpack_ntt_time.py [--keys 1024,16384] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntt-gpu-qtesla_amd"))

WARMUP, TIMED = 3, 11
SHAPES = {"p-I": (4, 29), "p-III": (5, 30)}   # k, bits


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


def run_shape(torch, ntt, dev, ps, nkeys, say):
    k, bits = SHAPES[ps]
    info = ntt.param_info(ps)
    n, q = info["n"], info["q"]
    tlen = k * n * bits // 8
    g = torch.Generator(device=dev).manual_seed(0x0E5 + n)
    # well-formed keys: canonical t, packed on the device; 32 bytes of seed_a behind them
    t0 = torch.randint(0, q, (nkeys, k, n), generator=g, dtype=torch.int32, device=dev)
    pk = torch.zeros((nkeys, tlen + 32), dtype=torch.uint8, device=dev)
    ntt.poly_pack(pk, t0, ps, bits, signed=False)
    del t0
    rows = torch.zeros((nkeys, k, 2, n), dtype=torch.int32, device=dev)
    chain = torch.zeros_like(rows)
    t = torch.empty((nkeys, k, n), dtype=torch.int32, device=dev)
    o = torch.empty_like(t)
    mx, mx2 = (torch.empty((nkeys, k), dtype=torch.int32, device=dev) for _ in range(2))
    slot1 = rows.view(-1)[n:]

    def fused():
        ntt.poly_unpack_ntt(slot1, pk, ps, bits, k, negate=True, pstride=2 * n, maxima=mx)

    def unpack():
        ntt.poly_unpack(t, pk, ps, bits, signed=False, maxima=mx2)

    def transform():
        ntt.poly_ntt(t.view(nkeys * k, n), ps)

    def negate():
        chain[:, :, 1, :] = q - t

    def ntt_oop():
        ntt.poly_ntt_oop(o, t, ps)

    # correctness first
    fused()
    unpack()
    transform()
    negate()
    assert torch.equal(rows[:, :, 1, :], chain[:, :, 1, :].remainder(q)), "fused rows differ from the chain's"
    assert not bool(rows[:, :, 0, :].any()), "slot 0 written"
    assert torch.equal(mx, mx2), "maxima differ from poly_unpack's"
    res = timed_rounds(torch, [fused, unpack, transform, negate, ntt_oop])
    npoly = nkeys * k
    say(f"{ps}: k = {k}, {bits}-bit fields, {nkeys} keys = {npoly} polynomials of n = {n}")
    for name, (m, lo, up) in zip(("fused", "unpack", "ntt", "negate", "ntt_oop"), res):
        say(f"  {name:8s} {m:8.4f} ms ({lo:.4f} - {up:.4f})")
    (fm, _, _), (um, ulo, uup), (nm, nlo, nup), (gm, _, _), (om, _, _) = res
    spread = max(uup - ulo, nup - nlo)
    margin = um + nm - fm
    say(f"  unpack + ntt {um + nm:.4f} ms, fused {fm:.4f} ms: margin {margin:.4f} ms, larger spread of the two legs "
        f"{spread:.4f} ms -> {'met' if margin > spread else 'NOT met'}; with negate {um + nm + gm:.4f} ms, "
        f"{(um + nm + gm) / fm:.2f} x fused")
    bytes_fused = npoly * n * (bits / 8 + 4)
    say(f"  fused / ntt_oop {fm / om:.3f} (traffic {(bits / 8 + 4) / 8:.3f}); fused moves {bytes_fused / (fm * 1e-3) / 1e12:.3f} TB/s, "
        f"ntt_oop {8 * n * npoly / (om * 1e-3) / 1e12:.3f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="1024,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_ntt", "unpack_ntt_time.txt"))
    args = ap.parse_args()
    import torch
    import ntt_amd as ntt
    assert torch.cuda.is_available(), "unpack_ntt_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"build {ntt.build_hash()}; {torch.cuda.get_device_name(dev)}; HIP events, {WARMUP} warm-up + {TIMED} rounds, "
            "median (min - max)")
        for nkeys in (int(b) for b in args.keys.split(",")):
            for ps in SHAPES:
                run_shape(torch, ntt, dev, ps, nkeys, say)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
