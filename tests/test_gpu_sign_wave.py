"""The device-only chain at a small batch (__graft_entry__.device_message_round_trip,
p-I, three short messages): G(m) and c' come from xof_ragged / xof with
path="auto", which is the wave path whenever xof_small_batch_max is at least
3.  G is hashlib's, the verifier's hash equals the signer's, the final nonces
are those of the seeds alone -- what tests/test_gpu_message_device.py asserts
at batch 16 -- and both hashes equal the two explicit paths'."""
import hashlib

import pytest
import torch

import __graft_entry__ as entry
from test_gpu_sign_device import NONCES

pytestmark = pytest.mark.gpu


def test_three_short_messages_sign_and_verify(ntt, dev):
    ps, algo = "p-I", entry.SIGN_SHAPES["p-I"][3]
    messages = [b"", b"qtesla", hashlib.shake_256(b"qtesla-ntt short message").digest(171)]
    batch = len(messages)
    # batch 3 is below both switches: path="auto" inside the round trip is the wave path
    assert ntt.xof_small_batch_max(algo, ragged=True) >= 3 and ntt.xof_small_batch_max(algo) >= 3
    r = entry.device_message_round_trip(ps, messages, dev)
    G = r["G"].cpu().numpy()
    assert G.shape == (batch, 64) and r["algo"] == algo == "shake128"
    for b, m in enumerate(messages):
        assert G[b].tobytes() == hashlib.shake_128(m).digest(64), f"G of message {b}"
    assert torch.equal(r["c1"], r["c2"]) and torch.equal(r["hi1"], r["hi2"]), "the verifier's hash differs from the signer's"
    assert r["nonces"].cpu().tolist() == NONCES[ps][:batch]          # the seeds alone decide them, not G
    for path in ("lane", "wave"):
        g = torch.empty_like(r["G"])
        ntt.xof_ragged(g, r["msg"], r["off"], algo=algo, path=path)
        assert torch.equal(g, r["G"]), f"G by path {path}"
        c = torch.empty_like(r["c1"])
        ntt.xof(c, r["hi1"], r["G"], algo=algo, path=path)
        assert torch.equal(c, r["c1"]), f"c' by path {path}"
    hi = r["hi1"].cpu().numpy()
    for b in range(batch):
        assert r["c1"][b].cpu().numpy().tobytes() == hashlib.shake_128(hi[b].tobytes() + G[b].tobytes()).digest(32)
