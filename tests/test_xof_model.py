"""The plain-Python Keccak model (keccak_model.py) without a GPU: against
hashlib's SHAKE, NIST's cSHAKE128 sample, its own general cSHAKE for
cshake*_simple, and the properties of enc the GPU cases rely on."""
import hashlib

import pytest

import keccak_model as K

LENGTHS = (0, 1, 135, 136, 137, 167, 168, 169, 500)
Q = {1024: 343576577, 2048: 856145921}


def _msg(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


@pytest.mark.parametrize("n", LENGTHS)
def test_model_equals_hashlib(n):
    m = _msg(n)
    for outlen in (32, 200):
        assert K.shake("shake128", m, outlen) == hashlib.shake_128(m).digest(outlen)
        assert K.shake("shake256", m, outlen) == hashlib.shake_256(m).digest(outlen)


def test_nist_cshake128_sample():
    # SP 800-185 cSHAKE sample #1: data 00 01 02 03, N empty, S = "Email Signature", 256 bits
    want = bytes.fromhex("c1c36925b6409a04f1b504fcbca9d82b4017277cb5ed2b2065fc1d3814d5aaf5")
    assert K.cshake("shake128", bytes(range(4)), 32, b"", b"Email Signature") == want


@pytest.mark.parametrize("algo", ("shake128", "shake256"))
def test_cshake_simple_is_cshake_with_two_byte_s(algo):
    rate = K.RATE[algo]
    for cstm in (0, 1, 0x1234, 65535):
        S = bytes([cstm & 0xFF, cstm >> 8])
        assert K.bytepad(K.encode_string(b"") + K.encode_string(S), rate) == K.cshake_simple_prefix(algo, cstm)
        for n in (0, 8, 40):
            assert K.cshake_simple(algo, _msg(n), 48, cstm) == K.cshake(algo, _msg(n), 48, b"", S)
    assert K.cshake_simple_prefix("shake128", 0x1234)[:8] == bytes.fromhex("01a8010001103412")
    assert K.cshake_simple_prefix("shake256", 0)[:8] == bytes.fromhex("0188010001100000")
    assert K.xof(algo, _msg(16), 32) == K.shake(algo, _msg(16), 32)


@pytest.mark.parametrize("n,h", ((1024, 25), (2048, 40), (2048, 57), (1024, 128)))
def test_enc_properties(n, h):
    q = Q[n]
    blocks, rejected = [], []
    for seed in K.seeds(12):
        st = {}
        pos, val = K.enc(seed, n, q, h, st)
        assert len(pos) == len(val) == h
        assert len(set(pos)) == h and all(0 <= p < n for p in pos)
        assert all(v in (1, q - 1) for v in val)
        assert K.enc(seed, n, q, h) == (pos, val)   # deterministic
        assert st["blocks"] == -(-(h + st["rejected"]) // K.BLOCK_DRAWS)
        blocks.append(st["blocks"])
        rejected.append(st["rejected"])
    if h > K.BLOCK_DRAWS:
        assert min(blocks) >= 2        # every seed takes a second block
    if h == 128:
        assert max(blocks) >= 3        # ... and some seed a third
    if (n, h) in ((2048, 40), (1024, 128)):
        assert max(rejected) >= 1      # some seed has a collision rejected


def test_enc_prefix_property():
    """a shorter h is a prefix of a longer one: the GPU cases may share one model run"""
    seed = K.seeds(1)[0]
    p128, v128 = K.enc(seed, 2048, Q[2048], 128)
    p40, v40 = K.enc(seed, 2048, Q[2048], 40)
    assert p128[:40] == p40 and v128[:40] == v40
