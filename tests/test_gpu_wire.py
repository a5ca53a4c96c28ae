"""Signatures and the public key as wire bytes (device_wire_round_trip):
poly_pack after the signer, poly_unpack with maxima in front of the verifier,
and rejection of a signature with one bit flipped."""
import pytest
import torch

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

BATCH = 16
SIG_BYTES = {"p-I": 2592, "p-III": 5664}
KEY_BYTES = {"p-I": 14880, "p-III": 38432}


@pytest.fixture(scope="module", params=("p-I", "p-III"))
def wire(request, ntt, dev):
    ps = request.param
    return ps, G.device_wire_round_trip(ps, BATCH, dev)


def test_signature_rows(wire):
    ps, r = wire
    assert tuple(r["sig"].shape) == (BATCH, SIG_BYTES[ps]) and r["zlen"] + 32 == SIG_BYTES[ps]
    assert torch.equal(r["sig"][:, r["zlen"]:], r["c1"])
    assert bool(r["accepted"].all()), "a signature does not verify from its bytes"
    assert torch.equal(r["z_unpacked"].view(-1), r["z"].view(-1))
    assert torch.equal(r["maxima"], r["norms"][:, 0])
    assert bool((r["maxima"] <= r["bound"]).all())


def test_key_row(wire):
    ps, r = wire
    k, n, q = r["k"], r["n"], r["q"]
    assert tuple(r["pk"].shape) == (1, KEY_BYTES[ps]) and r["tlen"] + 32 == KEY_BYTES[ps]
    assert torch.equal(r["pk"][0, r["tlen"]:].cpu(), torch.arange(32, dtype=torch.uint8))
    assert torch.equal(r["t_unpacked"], r["t"])
    assert tuple(r["t"].shape) == (1, k, n)
    assert bool((r["t_max"] < q).all()) and torch.equal(r["t_max"], r["t"].view(k, n).max(dim=1).values)


def test_flipped_z_bit_is_rejected(wire):
    """bit `bits - 2` of coefficient 5's field of message 1: by the norm test or by the hash"""
    ps, r = wire
    bits = r["bits"]
    sig = r["sig"].clone()
    j = 5 * bits + bits - 2
    sig[1, j // 8] ^= 1 << (j % 8)
    ok = r["verify_bytes"](sig)
    want = torch.ones(BATCH, dtype=torch.bool, device=ok.device)
    want[1] = False
    assert torch.equal(ok, want)


def test_flipped_challenge_bit_is_rejected(wire):
    ps, r = wire
    sig = r["sig"].clone()
    sig[2, r["zlen"] + 7] ^= 0x10
    ok = r["verify_bytes"](sig)
    want = torch.ones(BATCH, dtype=torch.bool, device=ok.device)
    want[2] = False
    assert torch.equal(ok, want)
    assert bool(r["verify_bytes"](r["sig"]).all())
