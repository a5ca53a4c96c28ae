"""Signatures under several keys verified in one launch
(device_multikey_round_trip): the verifier builds all keys' rows from the key
rows' bytes in batch calls and checks every signature, message m under key
keys[m], with one poly_mul_ntt_kl_round_keyed.  The true assignment accepts
everything, a wrong key rejects, and the answers are those of one unkeyed
verification per key."""
import functools

import numpy as np
import pytest
import torch

import __graft_entry__ as G
import gen_a_model as M
import keccak_model as K

pytestmark = pytest.mark.gpu

NKEYS, PER_KEY = 3, 4
BATCH = NKEYS * PER_KEY
NONCES = {"p-I": [0, 4, 0, 0], "p-III": [3, 7, 0, 4]}   # device_sign_round_trip's docstring, the first PER_KEY seeds

K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


@pytest.fixture(scope="module", params=("p-I", "p-III"))
def mk(request, ntt, dev):
    ps = request.param
    return ps, G.device_multikey_round_trip(ps, NKEYS, PER_KEY, dev)


def _unkeyed(r, key_of):
    """The answers of NKEYS separate unkeyed verifications: key j's signatures
    (messages j, j + NKEYS, ...) by its own verify_bytes under the rows of the
    key that key_of names for them; None unless one key serves them all."""
    want = torch.empty(BATCH, dtype=torch.bool, device=r["sig"].device)
    for j, rj in enumerate(r["per_key_results"]):
        used = set(key_of[j::NKEYS])
        if len(used) != 1:
            return None
        want[j::NKEYS] = rj["verify_bytes"](rj["sig"], r["rows"][used.pop()].contiguous())
    return want


def test_every_signature_is_accepted_under_its_key(mk, dev):
    ps, r = mk
    assert r["keys"].cpu().tolist() == [m % NKEYS for m in range(BATCH)]
    assert r["accepted"].dtype == torch.bool and tuple(r["accepted"].shape) == (BATCH,)
    assert bool(r["accepted"].all())
    assert torch.equal(r["verify"](r["keys"]), _unkeyed(r, r["keys"].cpu().tolist()))
    for j, rj in enumerate(r["per_key_results"]):
        assert rj["nonces"].cpu().tolist() == NONCES[ps]            # the restarts already listed, whatever the key
        assert torch.equal(r["sig"][j::NKEYS], rj["sig"])           # message m is message m // NKEYS of key m % NKEYS
    seeds = {bytes(r["pk"][j, r["tlen"]:].cpu().tolist()) for j in range(NKEYS)}
    assert seeds == set(r["seed_a"]) and len(seeds) == NKEYS
    assert len({bytes(r["pk"][j, :64].cpu().tolist()) for j in range(NKEYS)}) == NKEYS   # distinct secrets: distinct t


def test_slot_0_of_every_key_is_the_models_a(ntt, mk):
    ps, r = mk
    k, n, q = r["k"], r["n"], r["q"]
    rows = ntt.to_numpy_u32(r["rows"]).reshape(NKEYS, k, 2, n)
    for j in range(NKEYS):
        want = np.array(M.gen_a(r["seed_a"][j], k, n, q, G.GEN_A_BLOCKS[ps]), dtype=np.uint32)
        assert np.array_equal(rows[j, :, 0, :], want), j
        rj = r["per_key_results"][j]
        assert np.array_equal(rows[j, :, 0, :], ntt.to_numpy_u32(rj["ahat"]).reshape(k, n))      # the signer's rows
        assert np.array_equal(rows[j, :, 1, :], q - ntt.to_numpy_u32(rj["that"]).reshape(k, n))  # beside them


def test_rotated_keys_reject_every_signature(mk, dev):
    ps, r = mk
    rotated = [(m + 1) % NKEYS for m in range(BATCH)]
    got = r["verify"](torch.tensor(rotated, dtype=torch.int32, device=dev))
    assert not bool(got.any())
    assert torch.equal(got, _unkeyed(r, rotated))
    assert bool(r["verify"](r["keys"]).all())   # the closure keeps no state of the rejected assignment


def test_two_swapped_indices_reject_exactly_those_two(mk, dev):
    ps, r = mk
    a, b = 4, 8   # under keys 1 and 2
    swapped = r["keys"].clone()
    swapped[a], swapped[b] = r["keys"][b], r["keys"][a]
    assert int(swapped[a]) != int(r["keys"][a])
    got = r["verify"](swapped)
    want = torch.ones(BATCH, dtype=torch.bool, device=dev)
    want[a] = want[b] = False
    assert torch.equal(got, want)


def test_keys_none_is_message_b_under_key_b(mk, dev):
    """d_key = NULL: messages 0 .. NKEYS - 1 under their own keys, every later one
    under the last key -- accepted where that is its key."""
    ps, r = mk
    got = r["verify"](None)
    want = torch.tensor([min(m, NKEYS - 1) == m % NKEYS for m in range(BATCH)], device=dev)
    assert torch.equal(got, want)
