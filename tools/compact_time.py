"""Measurement for DESIGN.md section 5r: the full-batch signing loop against the
compacted one (same build, same seeds, host reads included) at 16 keys x 1 ..
256 messages for p-I and p-III, and ntt_select alone at 2^12, 2^16 and 2^20
flags.  Prints one JSON line per case (profiles/rows/compact_time.txt).

    python tools/compact_time.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as E   # noqa: E402

E._path()
import torch   # noqa: E402
import ntt_amd  # noqa: E402

dev = torch.device("cuda:0")


def full_sign_loop(ref, shat, neg_ehat):
    """device_keygen_round_trip's signing loop as it stands, plus the packing of the signature rows"""
    ps, n, q, batch, zlen, ahat, keys, seeds, G = (ref[nm] for nm in ("ps", "n", "q", "batch", "zlen", "ahat", "keys", "seeds", "G"))
    k, d, h, algo, bits = E.SIGN_SHAPES[ps]
    L = E.KEYGEN_BOUND[ps]
    B = (1 << (bits - 1)) - 1
    bound_z, bound_w, bound_lo = B - L, (q - 1) // 2 - L, (1 << (d - 1)) - L
    nonces = torch.zeros(batch, dtype=torch.int32, device=dev)
    y = torch.empty((batch, n), dtype=torch.int32, device=dev)
    v = torch.empty((batch, k, n), dtype=torch.int32, device=dev)
    hi1 = torch.empty((batch, k, n), dtype=torch.int8, device=dev)
    c1 = torch.empty((batch, 32), dtype=torch.uint8, device=dev)
    pos = torch.empty((batch, h), dtype=torch.int32, device=dev)
    val = torch.empty_like(pos)
    c = torch.empty((batch, n), dtype=torch.int32, device=dev)
    z = torch.empty((batch, 1, n), dtype=torch.int32, device=dev)
    znorms = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    wnorms = torch.empty((batch, k, 2), dtype=torch.int32, device=dev)
    for attempts in range(1, 257):
        ntt_amd.poly_sample_y(y, seeds, ps, bits, algo=algo, nonces=nonces)
        ntt_amd.poly_mul_ntt_kl_keyed(v, [y], ahat, keys, ps)
        ntt_amd.poly_round(v, ps, d, hi=hi1)
        ntt_amd.xof(c1, hi1, G, algo=algo)
        ntt_amd.poly_challenge(pos, val, c1, ps)
        ntt_amd.poly_scatter(c, pos, val, ps)
        ntt_amd.poly_mul_ntt_kl_keyed(z, [c], shat, keys, ps, add=y)
        ntt_amd.poly_round(z, ps, d, norms=znorms)
        ntt_amd.poly_mul_ntt_kl_round_keyed([c], neg_ehat, keys, ps, d, norms=wnorms, add=v)
        rejected = (znorms[:, 0] > bound_z) | (wnorms[:, :, 0] > bound_w).any(dim=1) | (wnorms[:, :, 1] > bound_lo).any(dim=1)
        if not bool(rejected.any()):
            break
        nonces += rejected.to(torch.int32)
    sig = torch.empty((batch, zlen + 32), dtype=torch.uint8, device=dev)
    ntt_amd.poly_pack(sig, z.view(batch, n), ps, bits)
    sig[:, zlen:] = c1
    return sig, nonces, attempts


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


for ps in ("p-I", "p-III"):
    for per_key in (1, 4, 16, 64, 256):
        nkeys = 16
        ref = E.device_keygen_round_trip(ps, nkeys, per_key, dev)
        k = ref["k"]
        n, q = ref["n"], ref["q"]
        shat = ntt_amd.poly_ntt(ref["s"].clone(), ps).view(nkeys, 1, 1, n)
        neg_ehat = (q - ntt_amd.poly_ntt(ref["e"].clone().view(nkeys * k, n), ps)).view(nkeys, k, 1, n).contiguous()
        full = lambda: full_sign_loop(ref, shat, neg_ehat)            # noqa: E731
        comp = lambda: E.compact_sign_loop(ref, shat, neg_ehat)       # noqa: E731
        full(), comp()                                                # warm-up of both, every shape they use
        tf, tc = [], []
        for rep in range(3):                                          # alternating
            (sf, nf, attempts), ev, wall = timed(full)
            tf.append((ev, wall))
            (sc, nc, live), ev, wall = timed(comp)
            tc.append((ev, wall))
            assert torch.equal(sf, sc) and torch.equal(nf, nc) and torch.equal(sf, ref["sig"])
        row = dict(ps=ps, batch=ref["batch"], attempts=attempts, full_message_attempts=attempts * ref["batch"],
                   needed_message_attempts=int((nf + 1).sum()), live=live,
                   full_ms_event=[round(a, 3) for a, _ in tf], full_ms_wall=[round(b, 3) for _, b in tf],
                   compact_ms_event=[round(a, 3) for a, _ in tc], compact_ms_wall=[round(b, 3) for _, b in tc])
        assert sum(live) == row["needed_message_attempts"] and len(live) == attempts
        print(json.dumps(row), flush=True)

g = torch.Generator(device=dev).manual_seed(5)
for logn in (12, 16, 20):
    nb = 1 << logn
    flag = torch.randint(0, 2, (nb,), generator=g, dtype=torch.int32, device=dev)
    idx = torch.empty(nb, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    bump = torch.zeros(nb, dtype=torch.int32, device=dev)
    for with_bump in (False, True):
        reps = 50
        for _ in range(5):
            ntt_amd.select(idx, count, flag, True, bump=bump if with_bump else None)
        _, ev, wall = timed(lambda: [ntt_amd.select(idx, count, flag, True, bump=bump if with_bump else None) for _ in range(reps)])
        row = dict(flags=nb, bump=with_bump, us_per_call_event=round(ev * 1e3 / reps, 2), selected=int(count))
        print(json.dumps(row), flush=True)
