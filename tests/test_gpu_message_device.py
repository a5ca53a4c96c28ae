"""qTESLA signing and verification of real messages with device calls only
(__graft_entry__.device_message_round_trip): G(m) by xof_ragged over messages
of different byte lengths, then device_sign_round_trip under that G.  G is
hashlib's, the verifier's hash equals the signer's, the final nonces are those
of the seeds alone, and a changed byte of one message changes that message's G
and c' and no other's."""
import hashlib

import pytest
import torch

import __graft_entry__ as entry
from test_gpu_sign_device import NONCES

pytestmark = pytest.mark.gpu

HASHLIB = {"shake128": hashlib.shake_128, "shake256": hashlib.shake_256}


@pytest.mark.parametrize("ps", ("p-I", "p-III"))
def test_messages_sign_and_verify_on_device(ntt, dev, ps):
    batch = 16
    messages = [hashlib.shake_256(b"qtesla-ntt message %d" % b).digest(13 * b) for b in range(batch)]
    assert [len(m) for m in messages] == [13 * b for b in range(batch)]
    algo = entry.SIGN_SHAPES[ps][3]
    r = entry.device_message_round_trip(ps, messages, dev)
    G = r["G"].cpu().numpy()
    assert G.shape == (batch, 64) and r["algo"] == algo
    for b, m in enumerate(messages):
        assert G[b].tobytes() == HASHLIB[algo](m).digest(64), f"{ps}: G of message {b}"
    assert r["msg"].cpu().numpy().tobytes() == b"".join(messages) + bytes(-sum(map(len, messages)) % 8)
    assert r["off"].cpu().tolist() == [13 * b * (b - 1) // 2 for b in range(batch + 1)]
    assert torch.equal(r["c1"], r["c2"]) and torch.equal(r["hi1"], r["hi2"]), f"{ps}: the verifier's hash differs from the signer's"
    assert r["nonces"].cpu().tolist() == NONCES[ps]          # the seeds alone decide them, not G
    # one byte of one message
    changed = list(messages)
    changed[5] = changed[5][:17] + bytes([changed[5][17] ^ 0x20]) + changed[5][18:]
    r2 = entry.device_message_round_trip(ps, changed, dev)
    assert torch.equal(r2["c1"], r2["c2"]) and r2["nonces"].cpu().tolist() == NONCES[ps]
    same_G = (r2["G"] == r["G"]).all(dim=1).cpu().tolist()
    same_c = (r2["c1"] == r["c1"]).all(dim=1).cpu().tolist()
    assert same_G == same_c == [b != 5 for b in range(batch)]
