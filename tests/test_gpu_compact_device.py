"""The restart loops with compaction (device_compact_keygen_sign_round_trip)
against the full-batch loops of device_keygen_round_trip, from the same seeds:
byte-identical signature rows and secrets, equal nonces, and live counts that
are exactly the messages not yet accepted, so that the message-attempts
processed are the sum of (nonce + 1).  And device_verdict, the verifier's
last line on the device, against the torch verdict."""
import pytest
import torch

import __graft_entry__ as E

pytestmark = pytest.mark.gpu

SHAPES = {"p-I": (3, 4), "p-III": (2, 3)}   # nkeys, per_key: the shapes of test_gpu_keygen_device.py


@pytest.fixture(scope="module", params=("p-I", "p-III"))
def cr(request, ntt, dev):
    ps = request.param
    return ps, E.device_compact_keygen_sign_round_trip(ps, *SHAPES[ps], dev)


def live_counts(nonces):
    """#{b : nonce_b >= t} for t = 0 .. max nonce"""
    return [sum(1 for v in nonces if v >= t) for t in range(max(nonces) + 1)]


def test_signatures_and_nonces_are_the_full_batch_loops(cr):
    ps, r = cr
    ref = r["ref"]
    assert r["sig"].shape == ref["sig"].shape and r["sig"].dtype == torch.uint8
    assert torch.equal(r["sig"], ref["sig"])                      # bytes: packed z and c' of every message
    assert torch.equal(r["nonces"], ref["nonces"])
    assert bool(ref["accepted"].all())


def test_secrets_and_their_nonces_are_the_full_batch_loops(cr):
    ps, r = cr
    ref = r["ref"]
    assert torch.equal(r["poly_nonces"], ref["poly_nonces"])
    assert torch.equal(r["se"][:, 0, :], ref["s"]) and torch.equal(r["se"][:, 1:, :], ref["e"])
    assert torch.equal(r["sums"], ref["sums"])


def test_an_attempt_runs_only_the_messages_still_rejected(cr):
    ps, r = cr
    ref = r["ref"]
    for live, nonces, attempts in ((r["sign_live"], ref["nonces"].cpu().tolist(), ref["attempts"]),
                                   (r["keygen_live"], ref["poly_nonces"].reshape(-1).cpu().tolist(), ref["keygen_attempts"])):
        assert live == live_counts(nonces)
        assert len(live) == attempts and live[0] == len(nonces)
        assert sum(live) == sum(v + 1 for v in nonces)           # the message-attempts processed
        assert any(b < a for a, b in zip(live, live[1:]))         # the list shrinks
        assert sum(live) < attempts * len(nonces)                 # ... below the full-batch loop's work
        print(f"{ps}: live per attempt {live}: {sum(live)} message-attempts, the full-batch loop runs {attempts * len(nonces)}")


def torch_verdict(ref, key_of, **kw):
    return (~ref["verify"](key_of, **kw)).to(torch.int32)


def test_verdict_is_torchs(cr):
    ps, r = cr
    ref = r["ref"]
    keys, zlen, batch = ref["keys"], ref["zlen"], ref["batch"]
    good = E.device_verdict(ref, keys)
    assert good.dtype == torch.int32 and tuple(good.shape) == (batch,)
    assert not bool(good.any()) and torch.equal(good, torch_verdict(ref, keys))
    assert not bool(E.device_verdict(ref, keys, sig_rows=r["sig"]).any())    # the compacted loop's rows verify
    for m, byte in ((1, 200), (batch - 1, zlen + 5), (0, zlen), (2, zlen + 31)):   # a bit of z; bits of c', its ends among them
        sig = ref["sig"].clone()
        sig[m, byte] ^= 16
        got = E.device_verdict(ref, keys, sig_rows=sig)
        assert got.tolist() == [int(b == m) for b in range(batch)], (m, byte)
        assert torch.equal(got, torch_verdict(ref, keys, sig_rows=sig))
    rotated = ((keys + 1) % ref["nkeys"]).contiguous()
    got = E.device_verdict(ref, rotated)
    assert bool(got.all()) and torch.equal(got, torch_verdict(ref, rotated))
    pk = ref["pk"].clone()
    pk[1, 100] ^= 4
    got = E.device_verdict(ref, keys, rows=ref["rows_from_pk"](pk))
    assert torch.equal(got, (keys == 1).to(torch.int32))
    assert not bool(E.device_verdict(ref, keys).any())            # again: no state is kept


def test_verdict_rejects_a_z_over_the_bound(cr, ntt, dev):
    """a row whose max |z| is over B - L_S: coefficient 0 of message 2 set to B, the largest value the field holds"""
    ps, r = cr
    ref = r["ref"]
    n, bits, batch, zlen = ref["n"], ref["bits"], ref["batch"], ref["zlen"]
    z = torch.empty((batch, n), dtype=torch.int32, device=dev)
    maxima = torch.empty(batch, dtype=torch.int32, device=dev)
    ntt.poly_unpack(z, ref["sig"], ps, bits, maxima=maxima)
    bound_z = (1 << (bits - 1)) - 1 - ref["bound"]
    assert int(maxima.max()) <= bound_z
    z[2, 0] = (1 << (bits - 1)) - 1
    sig = ref["sig"].clone()
    ntt.poly_pack(sig, z, ps, bits)
    assert torch.equal(sig[:, zlen:], ref["sig"][:, zlen:])       # c' is in the stride gap: not written
    ntt.poly_unpack(z, sig, ps, bits, maxima=maxima)
    assert int(maxima[2]) == (1 << (bits - 1)) - 1 > bound_z
    got = E.device_verdict(ref, ref["keys"], sig_rows=sig)
    assert got.tolist() == [int(b == 2) for b in range(batch)]
    assert torch.equal(got, torch_verdict(ref, ref["keys"], sig_rows=sig))
    # the bound alone decides it: with the same maxima against the field's own maximum nothing is over
    flag = torch.empty(batch, dtype=torch.int32, device=dev)
    ntt.rows_over(flag, maxima, [bound_z])
    assert flag.tolist() == [int(b == 2) for b in range(batch)]
    ntt.rows_over(flag, maxima, [(1 << (bits - 1)) - 1])
    assert not bool(flag.any())
