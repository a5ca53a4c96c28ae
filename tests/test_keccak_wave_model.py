"""The gather-form Keccak round of the wave kernels (tests/keccak_wave_model.py,
the text of csrc/ntt_xof_wave.hpp) against the plain permutation of
tests/keccak_model.py, and the shape of its index tables.  No GPU."""
import hashlib
import random

import keccak_model as K
import keccak_wave_model as W


def test_equals_the_permutation_on_random_states():
    rng = random.Random(0x5EED0031)
    for _ in range(64):
        a = [rng.getrandbits(64) for _ in range(25)]
        assert W.keccak_f1600(a) == K.keccak_f1600(a)


def test_zero_state_and_single_bits():
    assert W.keccak_f1600([0] * 25) == K.keccak_f1600([0] * 25)
    rng = random.Random(0x5EED0032)
    for i in range(25):
        for bit in (0, 31, 32, 63, rng.randrange(64)):
            a = [0] * 25
            a[i] = 1 << bit
            assert W.keccak_f1600(a) == K.keccak_f1600(a), (i, bit)


def test_one_round_at_a_time():
    """a single round with each constant, so that a failure names the round"""
    rng = random.Random(0x5EED0033)
    a = [rng.getrandbits(64) for _ in range(25)]
    for r, rc in enumerate(K.RC):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ K.rotl(c[(x + 1) % 5], 1) for x in range(5)]
        t = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = K.rotl(t[x + 5 * y], K.RHO[x + 5 * y])
        want = [b[i] ^ (~b[W.row(i, 1)] & K.M64 & b[W.row(i, 2)]) for i in range(25)]
        want[0] ^= rc
        a = W.keccak_round(a, rc)
        assert a == want, r


def test_variable_rotate():
    rng = random.Random(0x5EED0034)
    for n in range(64):
        for v in (0, 1, 1 << 63, K.M64, 0x0123456789ABCDEF, rng.getrandbits(64)):
            assert W.rotr_var(v, (64 - n) & 63) == K.rotl(v, n), (n, hex(v))


def test_index_tables_are_permutations():
    full = list(range(25))
    for name, t in W.TABLES.items():
        assert len(t) == 25 and sorted(t) == full, name
    # the column gathers stay in the column and visit each of its other rows once
    for i in range(25):
        col = {W.UP5[i], W.UP10[i], W.UP20[i], W.UP5[W.UP10[i]], i}
        assert col == {i % 5 + 5 * y for y in range(5)}, i
    # the row gathers are permutations of each row of five
    for name in ("XM1", "XP1", "XP2"):
        for y in range(5):
            assert sorted(W.TABLES[name][5 * y:5 * y + 5]) == list(range(5 * y, 5 * y + 5)), (name, y)
    # src is pi inverted: word x + 5 y moves to y + 5 (2 x + 3 y)
    for x in range(5):
        for y in range(5):
            assert W.src(y + 5 * ((2 * x + 3 * y) % 5)) == x + 5 * y


def test_placement_keeps_every_row_inside_a_16_lane_row():
    lanes = [W.lane_of(i) for i in range(25)]
    assert sorted(lanes) == list(range(15)) + list(range(16, 26))
    assert [W.word_of(l) for l in lanes] == list(range(25))
    assert [l for l in range(32) if W.word_of(l) is None] == [15, 26, 27, 28, 29, 30, 31]
    for i in range(25):
        for k in (1, 2, 4):
            want = W.lane_of(W.row(i, k))
            got = lanes[i] + k - 5 if i % 5 + k >= 5 else lanes[i] + k
            assert got == want and got // 16 == lanes[i] // 16, (i, k)


def test_placed_round_equals_the_round():
    """the round as the kernel runs it -- words placed in 32 lanes, passengers holding garbage, row gathers as shifts
    that read 0 outside a 16-lane row -- equals the gather form on the 25 words"""
    rng = random.Random(0x5EED0035)
    for _ in range(8):
        a = [rng.getrandbits(64) for _ in range(25)]
        v32 = [rng.getrandbits(64) for _ in range(32)]
        for i in range(25):
            v32[W.lane_of(i)] = a[i]
        for rc in K.RC:
            a = W.keccak_round(a, rc)
            v32 = W.keccak_round_placed(v32, rc)
            assert [v32[W.lane_of(i)] for i in range(25)] == a


def test_sponge_with_the_wave_permutation_is_shake():
    saved = K.keccak_f1600
    K.keccak_f1600 = W.keccak_f1600
    try:
        for n in (0, 8, 135, 136, 300):
            m = bytes(range(256)) * 2
            assert K.shake("shake256", m[:n], 200) == hashlib.shake_256(m[:n]).digest(200)
            assert K.shake("shake128", m[:n], 200) == hashlib.shake_128(m[:n]).digest(200)
    finally:
        K.keccak_f1600 = saved
