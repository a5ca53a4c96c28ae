"""A qTESLA signature made and verified with device calls only
(__graft_entry__.device_verify_round_trip): c' = H([a y]_M || G) on the
signer's side, Enc(c') by poly_challenge + poly_scatter, z = y + s c, and the
verifier's poly_challenge, poly_scatter, poly_mul_ntt_kl_round, ntt_xof must
give c' back bit for bit -- and equal hashlib over the downloaded hi bytes.
One coefficient of z changed by 2^d changes the hash."""
import hashlib

import pytest
import torch

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

HASHLIB = {"shake128": hashlib.shake_128, "shake256": hashlib.shake_256}


@pytest.mark.parametrize("ps", ("p-I", "p-III"))
def test_sign_verify_on_device(ntt, dev, ps):
    batch = 3
    r = entry.device_verify_round_trip(ps, batch, dev)
    n, q, k, d = r["n"], r["q"], r["k"], r["d"]
    assert (k, d, r["algo"]) == {"p-I": (4, 22, "shake128"), "p-III": (5, 24, "shake256")}[ps]
    c1, c2 = r["c1"].cpu().numpy(), r["c2"].cpu().numpy()
    assert c1.shape == (batch, 32)
    assert (c1 == c2).all(), f"{ps}: the verifier's hash differs from the signer's"
    assert torch.equal(r["hi1"], r["hi2"])
    hi, G = r["hi2"].cpu().numpy(), r["G"].cpu().numpy()
    assert hi.shape == (batch, k, n) and len({c1[b].tobytes() for b in range(batch)}) == batch
    for b in range(batch):
        want = HASHLIB[r["algo"]](hi[b].tobytes() + G[b].tobytes()).digest(32)
        assert c2[b].tobytes() == want, f"{ps}: message {b} against hashlib"
    # the challenge the verifier rebuilt: h entries of +-1
    c = ntt.to_numpy_u32(r["c"]).reshape(batch, n)
    assert ((c != 0).sum(axis=1) == r["h"]).all() and (((c == 0) | (c == 1) | (c == q - 1))).all()
    # a forged z: one coefficient of message 1 moved by 2^d
    z = r["z"].clone()
    z.view(batch, n)[1, 5] = (z.view(batch, n)[1, 5] + (1 << d)) % q
    forged = r["verify"](z).cpu().numpy()
    assert forged[0].tobytes() == c1[0].tobytes() and forged[2].tobytes() == c1[2].tobytes()
    assert forged[1].tobytes() != c1[1].tobytes(), f"{ps}: a forged z verified"
