"""The device arithmetic primitives themselves, on the GPU, against exact
integers.

lib/libqtesla_ntt_arith.so (tools/arith_probe.hip) includes the product
headers unchanged and applies one inlined device function per launch to
independent operand tuples: csub, canon4, shoup_mul, sshoup_mul, the seven
ct_bfly_t forms the kernels instantiate, gs_bfly, mont_mul, BaseMul's canon /
half / redc / run, the WIDE0 first stage of inv_pass2, inv_last_stage
(ntt_device.hpp), mont_dot (ntt_mulkl.hpp) and round_coeff (ntt_round.hpp),
for the three primes.  The operands are arith_model.grid's: every word within
+-2 of 0, q, 2q, 3q, 4q, 2^31 and 2^32 that the primitive's domain admits (the
S-form negatives too) in full product with each other and with the twiddles
(the named ones, the library's Phi / invPhi tables, 64 random ones), the
coincidences a random polynomial cannot aim at (a zero low word in the
Montgomery carry, d = 0 in the signed quotient, the rounding's ties, operands
built so that a lazy Shoup product lands at the ends of its interval), and
2^18 seeded random tuples.  Each case asserts

  * arith_model.check: congruence mod q and the output interval the callers
    rely on, in exact integer arithmetic;
  * equality with arith_model.model word for word, which binds the Python
    model that tests/test_device_arith.py examines to the header;
  * intact guard words around the output array and unchanged inputs.

Everything is bit-exact: there are no tolerances.

Out of scope: the Nussbaumer ring arithmetic, which lives inside
csrc/nussbaumer.hip and not in a header (tests/test_gpu_nussbaumer.py and
tests/nussbaumer_model.py cover that kernel as a whole).
"""
import numpy as np
import pytest
import torch

import arith_model as AM
import arith_probe as AP
from conftest import PARAM_SETS

pytestmark = pytest.mark.gpu

GUARD = 64                  # words before and after the output array
SENTINEL = 0xA5C3F00D
CASE_IDS = [f"{p}-v{v}" for p, v in AM.CASES]


@pytest.fixture(scope="module")
def probe(ntt):
    return AP.load(ntt)


@pytest.fixture(scope="module")
def twiddles(ntt):
    return {name: AM.twiddle_set(AM.PRIMES[name], *(ntt.tables(name)[k] for k in ("Phi", "invPhi"))) for name in PARAM_SETS}


def run_case(ntt, probe, dev, name, prim, variant, inputs, stream=None):
    """upload, one launch, download; asserts the guards and the inputs, returns the output columns"""
    _, nin, nout, _ = AM.PRIMS[prim]
    count = len(inputs[0])
    flat = np.concatenate([np.asarray(c).astype(np.uint32) for c in inputs])
    assert flat.size == nin * count
    d_in = ntt.from_numpy_u32(flat, dev)
    d_out = ntt.from_numpy_u32(np.full(nout * count + 2 * GUARD, SENTINEL, dtype=np.uint32), dev)
    torch.cuda.synchronize(dev)
    raw = None if stream is None else stream.cuda_stream
    rc = AP.run(probe, prim, variant, name, d_in.data_ptr(), flat.size, d_out.data_ptr() + 4 * GUARD, nout * count, count, raw)
    assert rc == 0, f"arith_probe({prim}, {variant}, {name}) returned {rc}"
    (stream or torch.cuda.current_stream(dev)).synchronize()
    got = ntt.to_numpy_u32(d_out)
    assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), "guard words around the output were written"
    assert np.array_equal(ntt.to_numpy_u32(d_in), flat), "the probe changed its inputs"
    body = got[GUARD:-GUARD]
    return [body[c * count:(c + 1) * count] for c in range(nout)]


def assert_case(ntt, probe, dev, twiddles, name, prim, variant, stream=None):
    q = AM.PRIMES[name]
    inputs = AM.grid(prim, q, variant, twiddles[name])
    outputs = run_case(ntt, probe, dev, name, prim, variant, inputs, stream)
    AM.check(prim, q, inputs, outputs, variant)
    want = AM.model(prim, q, inputs, variant)
    for c, (g, w) in enumerate(zip(outputs, want)):
        diff = np.flatnonzero(g != w.astype(np.uint32))
        assert diff.size == 0, (f"{prim} v{variant} {name}: output {c} differs from arith_model at {diff.size} tuples (the claim "
                                f"holds: the model is stale); first at {diff[0]}: in = {[hex(int(col[diff[0]])) for col in inputs]}, "
                                f"device {hex(int(g[diff[0]]))}, model {hex(int(w[diff[0]]))}")


@pytest.mark.parametrize("name", PARAM_SETS)
@pytest.mark.parametrize("prim,variant", AM.CASES, ids=CASE_IDS)
def test_device_primitive(ntt, probe, dev, twiddles, name, prim, variant):
    assert_case(ntt, probe, dev, twiddles, name, prim, variant)


def test_device_primitive_on_a_side_stream(ntt, probe, dev, twiddles):
    """the probe launches on the stream it is given: the typed butterfly that
    takes every kind of operand (S x, S y), and a register-set form"""
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        assert_case(ntt, probe, dev, twiddles, "p-III", "ct_bfly_t", 1, stream=s)
        assert_case(ntt, probe, dev, twiddles, "p-I", "bm_run", 1, stream=s)


def test_probe_rejects_mismatched_sizes(ntt, probe, dev):
    """a size that does not fit the primitive's operand count never reaches a launch"""
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    o = torch.zeros(64, dtype=torch.int32, device=dev)
    assert AP.run(probe, "ct_bfly_t", 0, "ref", t.data_ptr(), 64, o.data_ptr(), 64, 16) != 0     # needs 32 output words
    assert AP.run(probe, "ct_bfly_t", 7, "ref", t.data_ptr(), 64, o.data_ptr(), 32, 16) != 0     # no such form
    assert AP.run(probe, "csub_q", 0, "ref", t.data_ptr(), 64, o.data_ptr(), 64, 0) != 0
    assert probe.arith_probe(99, 0, 0, t.data_ptr(), 64, o.data_ptr(), 64, 64, None) != 0
    assert probe.arith_probe(0, 0, 3, t.data_ptr(), 64, o.data_ptr(), 64, 64, None) != 0         # p-III's prime is set 2
    torch.cuda.synchronize(dev)
    assert not bool(o.any())
