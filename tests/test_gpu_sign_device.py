"""qTESLA signing with restarts, made and verified with device calls only
(__graft_entry__.device_sign_round_trip): y from poly_sample_y at per-message
nonces, the chain to z, the signer's rejection test on poly_round's norms, a
rerun with the rejected messages' nonces raised, and the verifier's hash.  The
final nonces are those the CPU model predicts from max |y| alone, y is the
model's at the final nonce, and a forged z fails for its message only."""
import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import keccak_model as K   # noqa: F401  (sample_model's import)
import sample_model as M

pytestmark = pytest.mark.gpu

NONCES = {"p-I": [0, 4, 0, 0, 0, 0, 0, 3, 0, 2, 5, 1, 0, 2, 0, 2], "p-III": [3, 7, 0, 4, 2, 0, 0, 1, 1, 0, 4, 0, 3, 0, 0, 2]}


@pytest.mark.parametrize("ps", ("p-I", "p-III"))
def test_sign_with_restarts_on_device(ntt, dev, ps):
    batch = 16
    r = entry.device_sign_round_trip(ps, batch, dev)
    n, q, k, d, bits = r["n"], r["q"], r["k"], r["d"], r["bits"]
    assert (k, d, r["h"], r["algo"], bits) == entry.SIGN_SHAPES[ps] and r["margin"] == entry.SIGN_MARGIN[ps] > 0
    B = (1 << (bits - 1)) - 1
    assert r["bound"] == B - r["margin"]
    # the verifier's hash equals the signer's for every message
    c1, c2 = r["c1"].cpu().numpy(), r["c2"].cpu().numpy()
    assert c1.shape == (batch, 32) and (c1 == c2).all(), f"{ps}: the verifier's hash differs from the signer's"
    assert torch.equal(r["hi1"], r["hi2"]) and len({c1[b].tobytes() for b in range(batch)}) == batch
    # restarts happened, for some messages only, and as many as max |y| of the model demands
    nonces = r["nonces"].cpu().tolist()
    assert 0 in nonces and max(nonces) > 0
    assert nonces == NONCES[ps] and r["attempts"] == max(nonces) + 1
    # the accepted z is inside the bound, by the kernel's norms and by the downloaded z
    z = ntt.to_numpy_u32(r["z"]).reshape(batch, n).astype(np.int64)
    zmax = np.abs(np.where(z > q // 2, z - q, z)).max(axis=1)
    assert (zmax <= r["bound"]).all() and ntt.to_numpy_u32(r["norms"]).reshape(batch, 2)[:, 0].tolist() == zmax.tolist()
    # y of message b is the model's at its final nonce, and at that nonce only
    y = ntt.to_numpy_u32(r["y"]).reshape(batch, n)
    seeds = entry.sign_seeds(batch)
    assert r["seeds"].cpu().numpy().tobytes() == b"".join(seeds)
    for b in range(batch):
        assert y[b].tolist() == M.sample_y(seeds[b], n, q, bits, r["algo"], nonces[b]), f"{ps}: y of message {b}"
    b = nonces.index(max(nonces))
    assert y[b].tolist() != M.sample_y(seeds[b], n, q, bits, r["algo"], nonces[b] - 1)
    # z = y + s c with |s c| <= 2 h
    diff = (z - y.astype(np.int64)) % q
    assert np.abs(np.where(diff > q // 2, diff - q, diff)).max() <= 2 * r["h"]
    # a forged z: one coefficient of message 1 moved by 2^d
    forged_z = r["z"].clone()
    forged_z.view(batch, n)[1, 5] = (forged_z.view(batch, n)[1, 5] + (1 << d)) % q
    forged = r["verify"](forged_z).cpu().numpy()
    assert all(forged[b].tobytes() == c1[b].tobytes() for b in range(batch) if b != 1)
    assert forged[1].tobytes() != c1[1].tobytes(), f"{ps}: a forged z verified"
