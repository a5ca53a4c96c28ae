"""The verifier's rows from the key rows' bytes in two calls
(device_fused_rows_round_trip): poly_gen_a into slot 0 and poly_unpack_ntt,
negated, into slot 1 of [nkeys][k][2][n].  Every signature is accepted under
its own key and rejected under a neighbour's, the rows are the three-step rows
modulo q, the maxima are poly_unpack's, and one flipped bit of t in a key row
rejects that key's signatures and no others."""
import pytest
import torch

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

NKEYS, PER_KEY = 3, 2
BATCH = NKEYS * PER_KEY


@pytest.fixture(scope="module", params=("p-I", "p-III"))
def fr(request, ntt, dev):
    ps = request.param
    return ps, G.device_fused_rows_round_trip(ps, NKEYS, PER_KEY, dev)


def test_accepted_under_its_key_rejected_under_a_neighbours(fr, dev):
    ps, r = fr
    assert r["keys"].cpu().tolist() == [m % NKEYS for m in range(BATCH)]
    assert r["accepted"].dtype == torch.bool and tuple(r["accepted"].shape) == (BATCH,)
    assert bool(r["accepted"].all())
    rotated = torch.tensor([(m + 1) % NKEYS for m in range(BATCH)], dtype=torch.int32, device=dev)
    assert not bool(r["verify"](rotated, r["rows"]).any())
    assert bool(r["verify"](r["keys"], r["rows"]).all())   # the closure keeps no state of the rejected assignment
    assert torch.equal(r["verify"](r["keys"], r["rows"]), r["multikey"]["accepted"])


def test_rows_are_the_three_step_rows_mod_q(fr):
    ps, r = fr
    k, n, q = r["k"], r["n"], r["q"]
    assert r["rows_equal"] is True
    rows, three = r["rows"], r["multikey"]["rows"]
    assert tuple(rows.shape) == (NKEYS, k, 2, n) and rows.dtype == torch.int32
    assert torch.equal(rows[:, :, 0, :], three[:, :, 0, :])                      # poly_gen_a's, word for word
    assert int(rows.min()) >= 0 and int(rows.max()) < q                         # canonical: 0 where the three steps give q
    assert torch.equal(rows[:, :, 1, :], three[:, :, 1, :].remainder(q))
    assert torch.equal(rows[:, :, 1, :] == 0, three[:, :, 1, :] == q)


def test_maxima_are_poly_unpacks(ntt, fr, dev):
    ps, r = fr
    k, n, q = r["k"], r["n"], r["q"]
    t = torch.empty((NKEYS, k, n), dtype=torch.int32, device=dev)
    want = torch.empty((NKEYS, k), dtype=torch.int32, device=dev)
    ntt.poly_unpack(t, r["pk"], ps, r["qbits"], signed=False, maxima=want)
    assert tuple(r["maxima"].shape) == (NKEYS, k)
    assert torch.equal(r["maxima"], want)
    assert int(want.max()) < q and int(want.min()) > 0                          # well-formed keys


def test_one_flipped_bit_of_t_rejects_that_keys_signatures_only(fr, dev):
    """the top bit of one field of t (bit qbits - 1 of coefficient c of t_i): t_i changes by 2^(qbits-1) mod q, so
    every coefficient of t_i c that c touches moves by more than 2^d and [w_i]_M, hence the hash, changes"""
    ps, r = fr
    k, n, qbits = r["k"], r["n"], r["qbits"]
    for key, i, coeff in ((1, 0, 0), (0, k - 1, n - 1), (2, 1, n // 2 + 5)):
        j = (i * n + coeff) * qbits + qbits - 1
        byte, bit = j // 8, j % 8
        assert byte < r["tlen"]
        pk = r["pk"].clone()
        pk[key, byte] ^= 1 << bit
        rows, maxima = r["rows_from_pk"](pk)
        changed = (rows != r["rows"]).flatten(1).any(dim=1).cpu().tolist()
        assert changed == [j == key for j in range(NKEYS)]
        assert torch.equal(rows[:, :, 0, :], r["rows"][:, :, 0, :])             # seed_a untouched: slot 0 as before
        got = r["verify"](r["keys"], rows)
        want = torch.tensor([m % NKEYS != key for m in range(BATCH)], device=dev)
        assert torch.equal(got, want), (ps, key, byte, bit)
    assert bool(r["verify"](r["keys"], r["rows"]).all())
