"""Key generation, signing with e != 0 and verification on the device
(device_keygen_round_trip): the secret polynomials come from
poly_sample_gauss and pass check_ES by poly_hsum after exactly the restarts
the CPU model predicts, t = a s + e equals the oracle's, every signature is
accepted by a verifier that holds bytes alone, and a flipped bit or a wrong
key rejects."""
import functools

import numpy as np
import pytest
import torch

import __graft_entry__ as E
import gauss_model as G
import gen_a_model as A
import keccak_model as K

pytestmark = pytest.mark.gpu

SHAPES = {"p-I": (3, 4), "p-III": (2, 3)}   # nkeys, per_key

K.cshake_simple = functools.lru_cache(maxsize=None)(K.cshake_simple)


def predicted_nonces(ps, nkeys, n, q):
    """The final nonce of every polynomial by the CPU model: the first nonce at
    which gauss_model.hsum of gauss_model.sample_gauss is within KEYGEN_BOUND.
    With the labels of keygen_seed the restarts are
      p-I,   3 keys  [[0, 0, 1, 0, 0], [0, 0, 3, 2, 0], [1, 0, 0, 1, 0]]
      p-III, 2 keys  [[2, 0, 1, 0, 1, 1], [0, 2, 0, 0, 1, 0]]
    (NONCES below; rows: keys; columns: s, e_1 .. e_k), computed on the CPU
    before they were written down: polynomials of each set restart, key 0's
    among them, and none needs more than 4 attempts.  The label was chosen for
    that: "qtesla-ntt keygen seed %d.%d" gave a polynomial of p-III ten."""
    k, d, h, algo, bits = E.SIGN_SHAPES[ps]
    rows, cols = E.KEYGEN_TABLE[ps]
    table = E.keygen_table(ps)
    out = []
    for j in range(nkeys):
        out.append([])
        for i in range(k + 1):
            for nonce in range(256):
                if G.hsum(G.sample_gauss(E.keygen_seed(j, i), n, q, table, cols, algo, nonce), q, h) <= E.KEYGEN_BOUND[ps]:
                    break
            out[-1].append(nonce)
    return out


NONCES = {"p-I": [[0, 0, 1, 0, 0], [0, 0, 3, 2, 0], [1, 0, 0, 1, 0]], "p-III": [[2, 0, 1, 0, 1, 1], [0, 2, 0, 0, 1, 0]]}


@pytest.fixture(scope="module", params=("p-I", "p-III"))
def kg(request, ntt, dev):
    ps = request.param
    return ps, E.device_keygen_round_trip(ps, *SHAPES[ps], dev)


def test_secrets_pass_check_es_at_the_predicted_nonces(ntt, kg):
    ps, r = kg
    nkeys, k, n, q, h = r["nkeys"], r["k"], r["n"], r["q"], r["h"]
    want = predicted_nonces(ps, nkeys, n, q)
    assert want == NONCES[ps]
    assert any(v for row in want for v in row) and max(v for row in want for v in row) < 8
    assert r["poly_nonces"].cpu().tolist() == want
    assert r["keygen_attempts"] == 1 + max(v for row in want for v in row)
    assert int(r["sums"].max()) <= E.KEYGEN_BOUND[ps]
    se = np.concatenate([ntt.to_numpy_u32(r["s"]).reshape(nkeys, 1, n), ntt.to_numpy_u32(r["e"]).reshape(nkeys, k, n)], axis=1)
    table, cols = E.keygen_table(ps), E.KEYGEN_TABLE[ps][1]
    for j in range(nkeys):
        for i in range(k + 1):
            assert G.hsum(se[j, i], q, h) == int(r["sums"][j, i]) <= E.KEYGEN_BOUND[ps], (j, i)
    # key 0's polynomials are the model's at those nonces
    for i in range(k + 1):
        m = G.sample_gauss(E.keygen_seed(0, i), n, q, table, cols, r["algo"], want[0][i])
        assert np.array_equal(se[0, i], np.array(m, dtype=np.uint32)), i
    assert np.any(se[:, 1:] != 0)   # e is not zero


def test_t_is_the_oracles_a_s_plus_e(ntt, oracle, kg):
    ps, r = kg
    k, n, q = r["k"], r["n"], r["q"]
    s = ntt.to_numpy_u32(r["s"]).reshape(-1, n)[0]
    e = ntt.to_numpy_u32(r["e"]).reshape(-1, k, n)[0]
    ahat = ntt.to_numpy_u32(r["ahat"]).reshape(-1, k, n)[0]
    assert np.array_equal(ahat, np.array(A.gen_a(r["seed_a"][0], k, n, q, E.GEN_A_BLOCKS[ps]), dtype=np.uint32))
    a = oracle.poly_invntt(ahat, ps)
    want = (oracle.poly_mul(a, np.broadcast_to(s, a.shape), ps).astype(np.uint64) + e) % q
    assert np.array_equal(ntt.to_numpy_u32(r["t"]).reshape(-1, k, n)[0], want.astype(np.uint32))
    # the key row carries it: unpacked again it is t, and the row ends in seed_a
    t2 = torch.empty_like(r["t"])
    ntt.poly_unpack(t2, r["pk"], ps, r["qbits"], signed=False)
    assert torch.equal(t2, r["t"])
    assert [bytes(row[r["tlen"]:].cpu().tolist()) for row in r["pk"]] == r["seed_a"]


def test_every_signature_is_accepted_from_bytes(kg):
    ps, r = kg
    assert r["attempts"] <= 256 and int(r["nonces"].max()) == r["attempts"] - 1
    print(f"{ps}: {r['attempts']} signing attempts, final nonces {r['nonces'].cpu().tolist()}")
    assert r["accepted"].dtype == torch.bool and tuple(r["accepted"].shape) == (r["batch"],)
    assert bool(r["accepted"].all())
    assert r["keys"].cpu().tolist() == [m % r["nkeys"] for m in range(r["batch"])]
    # the signer's bounds held at the final attempt
    L, q, d, bits = r["bound"], r["q"], r["d"], r["bits"]
    assert int(r["znorms"][:, 0].max()) <= (1 << (bits - 1)) - 1 - L
    assert int(r["wnorms"][:, :, 0].max()) <= (q - 1) // 2 - L and int(r["wnorms"][:, :, 1].max()) <= (1 << (d - 1)) - L
    assert bool(r["verify"](r["keys"]).all())   # again: the closure keeps no state


@pytest.mark.parametrize("where", ("z", "c", "t"))
def test_one_flipped_bit_rejects(kg, where):
    ps, r = kg
    m = 1   # a message of key 1
    if where == "t":
        pk = r["pk"].clone()
        pk[1, 100] ^= 4
        got = r["verify"](r["keys"], rows=r["rows_from_pk"](pk))
        want = r["keys"] != 1            # every signature of key 1, and no other
    else:
        sig = r["sig"].clone()
        sig[m, 200 if where == "z" else r["zlen"] + 5] ^= 16
        got = r["verify"](r["keys"], sig_rows=sig)
        want = torch.ones_like(got)
        want[m] = False
    assert torch.equal(got, want)
    assert bool(r["verify"](r["keys"]).all())


def test_the_wrong_key_rejects(kg, dev):
    ps, r = kg
    rotated = ((r["keys"] + 1) % r["nkeys"]).contiguous()
    assert not bool(r["verify"](rotated).any())
    assert bool(r["verify"](r["keys"]).all())
