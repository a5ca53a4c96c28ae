"""A verifier that holds only the public-key row's bytes
(device_pk_round_trip): the rows [a_i-hat, q - t_i-hat] made on the device from
t's fields and seed_a, poly_gen_a with pstride = 2 n beside q - t-hat, and
rejection of every signature once one bit of the key row is flipped."""
import functools

import numpy as np
import pytest
import torch

import __graft_entry__ as G
import gen_a_model as M
import keccak_model as K

pytestmark = pytest.mark.gpu

BATCH = 16
NONCES = {"p-I": [0, 4, 0, 0, 0, 0, 0, 3, 0, 2, 5, 1, 0, 2, 0, 2],      # device_sign_round_trip's docstring
          "p-III": [3, 7, 0, 4, 2, 0, 0, 1, 1, 0, 4, 0, 3, 0, 0, 2]}

K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


@pytest.fixture(scope="module", params=("p-I", "p-III"))
def pk(request, ntt, dev):
    ps = request.param
    return ps, G.device_pk_round_trip(ps, BATCH, dev)


def test_every_signature_is_accepted(pk):
    ps, r = pk
    assert r["accepted"].dtype == torch.bool and tuple(r["accepted"].shape) == (BATCH,)
    assert bool(r["accepted"].all()), "a signature does not verify under rows made from the key row's bytes"
    assert torch.equal(r["pk"][0, r["tlen"]:].cpu(), torch.tensor(list(G.pk_seed_a()), dtype=torch.uint8))
    assert bool(r["verify_with_pk"](r["pk"]).all())


def test_rows_slot_0_is_the_models_a(ntt, pk):
    ps, r = pk
    k, n, q = r["k"], r["n"], r["q"]
    want = np.array(M.gen_a(G.pk_seed_a(), k, n, q, G.GEN_A_BLOCKS[ps]), dtype=np.uint32)
    rows = ntt.to_numpy_u32(r["rows"]).reshape(k, 2, n)
    assert np.array_equal(rows[:, 0, :], want)
    assert np.array_equal(rows[:, 0, :], ntt.to_numpy_u32(r["ahat"]).reshape(k, n))      # the signer's rows
    assert np.array_equal(rows[:, 1, :], q - ntt.to_numpy_u32(r["that"]).reshape(k, n))  # beside them, untouched


def test_flipped_seed_a_bit_rejects_every_signature(pk):
    ps, r = pk
    row = r["pk"].clone()
    row[0, r["tlen"] + 17] ^= 0x08
    assert not bool(r["verify_with_pk"](row).any())
    assert bool(r["verify_with_pk"](r["pk"]).all())     # the closure keeps no state of the rejected key


def test_flipped_t_bit_rejects_every_signature(pk):
    """the top bit of t_0's coefficient 0 (bit qbits - 1 of the row): t changes by 2^(qbits-1) mod q, so every
    coefficient of t_0 c that c touches moves by more than 2^d and [w_0]_M, hence the hash, changes"""
    ps, r = pk
    row = r["pk"].clone()
    j = r["qbits"] - 1
    row[0, j // 8] ^= 1 << (j % 8)
    assert not bool(r["verify_with_pk"](row).any())


def test_sign_with_seed_a_ends_at_the_same_nonces(dev, pk):
    ps, r = pk
    assert r["nonces"].cpu().tolist() == NONCES[ps]
    plain = G.device_sign_round_trip(ps, BATCH, dev)
    assert plain["nonces"].cpu().tolist() == NONCES[ps]
    assert not torch.equal(plain["ahat"], r["ahat"])
    assert torch.equal(plain["y"], r["y"])
