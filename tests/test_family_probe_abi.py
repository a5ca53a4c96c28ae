"""The test-only family probe (tools/family_probe.hip) without a GPU: its
argument checks on fake pointers (every call here fails a check or is an empty
batch, so nothing is launched), its launch shapes against a Python restatement
of launch_shape(), and the enumerations tests/test_gpu_family_probe.py walks.
"""
import pytest

import family_probe as fp

FAKE = 0x100000      # never dereferenced
FAR = 0x1000000000   # 64 GiB apart: no two fake buffers overlap
A, B, C = FAKE, FAKE + FAR, FAKE + 2 * FAR
FAMILIES = (0, 2, 3, 4)


@pytest.fixture(scope="module")
def probe(ntt):
    return fp.load(ntt)


def test_symbols_are_exported(probe):
    for name in ("family_probe_xform", "family_probe_mul", "family_probe_shape", "family_probe_sync_expiries",
                 "family_probe_set_cus", "family_probe_consts"):
        assert hasattr(probe, name), name
    assert fp.consts(probe) == dict(min_wg_per_cu=4, ppw_max=fp.CHUNK_MAX)


def test_instantiations(ntt, probe):
    """The enumeration has one entry per compiled kernel -- 5 parameter sets x
    4 transform kinds x 3 radices = 60 one-polynomial transforms, the 20 batch
    transforms, 5 bit-reversal copies, 10 batch products and the 8 radix-4
    products (k_poly_mul_lat exists for n <= 4096) -- and the probe accepts
    exactly those combinations."""
    inst = fp.instantiations()
    assert len(inst) == len(set(inst)) == 103
    assert sum(1 for ps, op, f in inst if op in fp.TRANSFORMS and f) == 60
    assert sum(1 for ps, op, f in inst if op in fp.TRANSFORMS and not f) == 20
    assert [(ps, f) for ps, op, f in inst if op == "bitrev"] == [(ps, 0) for ps in fp.ALL_SETS]
    assert sum(1 for ps, op, f in inst if op in fp.PRODUCTS and not f) == 10
    assert sorted((ps, op) for ps, op, f in inst if op in fp.PRODUCTS and f) == sorted(
        (ps, op) for ps in fp.ALL_SETS[:4] for op in fp.PRODUCTS)
    assert all(f == 2 for ps, op, f in inst if op in fp.PRODUCTS and f)
    for ps in fp.ALL_SETS:
        for op in fp.OPS:
            for family in FAMILIES:
                # a named chunk: family 0's shape then needs no device
                rc, _ = fp.shape(probe, family, op, ntt.PARAM_SETS[ps], 5, chunk=0 if family else 1)
                assert rc == (ntt.NTT_OK if (ps, op, family) in inst else ntt.NTT_ERR_PARAM), (ps, op, family)


def test_routed_instantiations(ntt):
    """How many of the 60 one-polynomial transform kernels any batch reaches
    through the entry points, derived from ntt_small_batch_radix: 29 at the
    table this was written against (ref / p-I 8 each, p-III 4, n = 4096 5,
    n = 8192 4).  The number moves with every measured table, so only its
    range is asserted; the other kernels are run by the probe alone."""
    import family_cells as fc
    compiled = {i for i in fp.instantiations() if i[2] and i[1] in fp.TRANSFORMS}
    routed = set()
    for ps in fp.ALL_SETS:
        for op in ntt.SWITCH_OPS:
            if op in fp.PRODUCTS:
                continue
            for radix, _, _ in fc.families(ntt, ps, op)[:-1]:
                routed.add((ps, op.replace("_oop", ""), radix.bit_length() - 1))
    print(f"{len(routed)} of {len(compiled)} one-polynomial transform kernels are routed to")
    assert routed <= compiled and len(compiled) == 60 and 0 < len(routed) <= 60


def _xf(probe, family=0, kind=0, ps=0, out=B, inp=A, batch=3, chunk=1):
    return probe.family_probe_xform(family, kind, ps, out, inp, batch, chunk, None)


def _ml(probe, family=0, bhat=0, ps=0, c=C, a=A, b=B, batch=3, chunk=1):
    return probe.family_probe_mul(family, bhat, ps, c, a, b, batch, chunk, None)


def test_param(ntt, probe):
    E = ntt
    for kw in (dict(family=1), dict(family=5), dict(family=-1), dict(kind=-1), dict(kind=5), dict(kind=6), dict(ps=-1),
               dict(ps=5), dict(chunk=-1), dict(chunk=17),
               dict(family=2, chunk=1), dict(family=3, chunk=16), dict(family=4, chunk=2),     # no chunk to name
               dict(family=2, kind=4, chunk=0), dict(family=4, kind=4, chunk=0)):              # BITREV: family 0 only
        assert _xf(probe, **kw) == E.NTT_ERR_PARAM, kw
        assert _xf(probe, **dict(kw, batch=0, out=None, inp=None)) == E.NTT_ERR_PARAM, kw      # before the empty batch
    for kw in (dict(family=1), dict(family=3, chunk=0), dict(family=4, chunk=0), dict(family=2, ps=4, chunk=0),
               dict(family=2, chunk=1), dict(bhat=2), dict(bhat=-1), dict(ps=5), dict(chunk=17), dict(chunk=-1)):
        assert _ml(probe, **kw) == E.NTT_ERR_PARAM, kw
        assert _ml(probe, **dict(kw, batch=0, c=None)) == E.NTT_ERR_PARAM, kw
    # family 2 products exist up to n = 4096: the next check speaks
    assert _ml(probe, family=2, ps=3, chunk=0, c=None) == E.NTT_ERR_NULL


def test_checks_in_order(ntt, probe):
    """PARAM, empty batch, NULL, ALIGN, SIZE, ALIAS: the ABI's codes in the ABI's order"""
    E = ntt
    for family, chunk in ((0, 1), (0, 16), (0, 0), (2, 0), (3, 0), (4, 0)):
        for ps in range(5):
            n = ntt.param_info(fp.ALL_SETS[ps])["n"]
            kw = dict(family=family, chunk=chunk, ps=ps)
            # an empty batch looks at nothing else
            assert _xf(probe, **kw, batch=0, out=None, inp=None) == E.NTT_OK
            assert _xf(probe, **kw, batch=0, out=A + 1, inp=A + 2) == E.NTT_OK
            assert _xf(probe, **kw, out=None) == E.NTT_ERR_NULL
            assert _xf(probe, **kw, inp=None, out=B + 1) == E.NTT_ERR_NULL
            assert _xf(probe, **kw, inp=None, batch=1 << 31) == E.NTT_ERR_NULL
            for off in (1, 2):
                assert _xf(probe, **kw, out=B + off) == E.NTT_ERR_ALIGN
                assert _xf(probe, **kw, inp=A + off, batch=1 << 31) == E.NTT_ERR_ALIGN
                assert _xf(probe, **kw, inp=A + off, out=A + off + 4 * n) == E.NTT_ERR_ALIGN
            for batch in (1 << 31, 1 << 40):
                assert _xf(probe, **kw, batch=batch) == E.NTT_ERR_SIZE
                assert _xf(probe, **kw, batch=batch, out=A + 4) == E.NTT_ERR_SIZE            # before the overlap
            for out in (A + 4, A + 4 * n, A + 4 * (3 * n - 1), A - 4 * (3 * n - 1)):          # batch 3: 3 n words each
                assert _xf(probe, **kw, out=out) == E.NTT_ERR_ALIAS, hex(out)
            if family in (0, 2) and not (family == 2 and ps == 4):
                for bhat in (0, 1):
                    mk = dict(kw, bhat=bhat)
                    assert _ml(probe, **mk, batch=0, a=None, b=None, c=None) == E.NTT_OK
                    for nul in ("a", "b", "c"):
                        assert _ml(probe, **mk, **{nul: None}) == E.NTT_ERR_NULL
                        assert _ml(probe, **mk, **{nul: FAKE + 9 * FAR + 2}) == E.NTT_ERR_ALIGN
                    assert _ml(probe, **mk, a=None, b=B + 1) == E.NTT_ERR_NULL
                    assert _ml(probe, **mk, c=C + 2, batch=1 << 31) == E.NTT_ERR_ALIGN
                    assert _ml(probe, **mk, batch=1 << 31, c=A + 4) == E.NTT_ERR_SIZE
                    assert _ml(probe, **mk, c=A + 4) == E.NTT_ERR_ALIAS
                    assert _ml(probe, **mk, c=B + 4 * n) == E.NTT_ERR_ALIAS
                    assert _ml(probe, **mk, c=B - 4 * (3 * n - 1)) == E.NTT_ERR_ALIAS


def test_launch_size(ntt, probe):
    """grid x block must fit 32 bits: a one-polynomial family's grid is the
    batch; a named chunk fixes the grid whatever the device"""
    E = ntt
    for family, ps, threads in ((4, 0, 64), (3, 1, 128), (2, 0, 256), (2, 4, 1024), (4, 4, 512), (3, 3, 512)):
        first_bad = (1 << 32) // threads
        assert _xf(probe, family=family, ps=ps, chunk=0, batch=first_bad) == E.NTT_ERR_SIZE
        rc, sh = fp.shape(probe, family, "fwd", ps, first_bad)
        assert rc == E.NTT_ERR_SIZE
        rc, sh = fp.shape(probe, family, "fwd", ps, first_bad - 1)
        assert rc == E.NTT_OK and sh == dict(grid=first_bad - 1, block=threads, chunk=1, per=1)
    # n = 1024 batch kernels, chunk 1: 8 units = 16 polynomials per 512-thread workgroup,
    # so 2^27 - 16 polynomials are the last batch with fewer than 2^23 workgroups
    assert _xf(probe, family=0, ps=0, chunk=1, batch=(1 << 27) - 15) == E.NTT_ERR_SIZE
    assert _ml(probe, family=0, ps=1, chunk=1, batch=(1 << 27) - 15) == E.NTT_ERR_SIZE
    rc, sh = fp.shape(probe, 0, "fwd", 0, (1 << 27) - 16, chunk=1)
    assert rc == E.NTT_OK and sh["grid"] * sh["block"] == (1 << 32) - 512
    rc, _ = fp.shape(probe, 0, "fwd", 0, 1 << 31, chunk=16)
    assert rc == E.NTT_ERR_SIZE
    for out in ("grid", "block", "chunk", "per"):
        import ctypes
        args = {k: ctypes.c_uint32() for k in ("grid", "block", "chunk", "per")}
        args[out] = None
        assert probe.family_probe_shape(0, 0, 0, 5, 1, args["grid"], args["block"], args["chunk"], args["per"]) == E.NTT_ERR_NULL
    for cus in (-1, 65537):
        assert probe.family_probe_set_cus(cus) == E.NTT_ERR_PARAM


def test_shape_is_the_products_rule(ntt, probe):
    """chunk 0: launch_shape() over the product's constants, at the CU counts
    of a partitioned and a whole card"""
    seen = set()
    try:
        for cus in (32, 256):
            assert probe.family_probe_set_cus(cus) == ntt.NTT_OK
            for ps in fp.ALL_SETS:
                for op in fp.OPS:
                    for batch in (1, 7, 2817, 131073, 1 << 20):
                        rc, sh = fp.shape(probe, 0, op, ntt.PARAM_SETS[ps], batch)
                        assert rc == ntt.NTT_OK and sh == fp.expected_shape(ps, op, batch, cus), (cus, ps, op, batch, sh)
                        seen.add(sh["chunk"])
    finally:
        assert probe.family_probe_set_cus(0) == ntt.NTT_OK
    assert {1, 16} <= seen and len(seen) > 4   # the rule's whole range is walked


def test_walk_batches(ntt, probe):
    """The batches test_batch_kernel_chunks uses give the grids their
    definition promises (two full workgroups and one that stops mid-chunk; two
    full ones; one unit), a named chunk is the chunk launched, and a work unit
    is two polynomials exactly at n = 1024."""
    largest = 0
    for ps in fp.ALL_SETS:
        psi = ntt.PARAM_SETS[ps]
        for op in fp.OPS:
            for c in fp.CHUNKS:
                rc, one = fp.shape(probe, 0, op, psi, 1, chunk=c)
                assert rc == ntt.NTT_OK and one["grid"] == 1
                per = one["per"]
                rc, two = fp.shape(probe, 0, op, psi, 2 * per, chunk=1)
                assert rc == ntt.NTT_OK and two["grid"] == 2 // fp.upw(ps), (ps, op)
                walk = fp.walk_batches(per, fp.upw(ps), c)
                assert [g for _, g in walk] == [3, 2, 1]
                for batch, grid in walk:
                    rc, sh = fp.shape(probe, 0, op, psi, batch, chunk=c)
                    assert rc == ntt.NTT_OK and sh["grid"] == grid and sh["per"] == per, (ps, op, c, batch, sh)
                    if not (ps in fp.LARGE_SETS and op == "bitrev"):
                        assert sh["chunk"] == c
                    assert sh["block"] == one["block"]
                    largest = max(largest, batch)
                # the tail workgroup walks c // 2 full passes, then one that holds per // 2 + 1 units
                units = -(-walk[0][0] // fp.upw(ps))
                left = units - 2 * per * c
                assert left == per * (c // 2) + per // 2 + 1 and 0 < left <= per * c
                if per > 2:
                    # ... a partial pass, and from c = 3 on not the chunk's last: the loop's break ends it
                    assert 0 < left % per < per and (c <= 2 or -(-left // per) < c)
        if fp.upw(ps) == 2:
            assert all(fp.walk_batches(8, 2, c)[0][0] % 2 == 1 for c in fp.CHUNKS)
    assert largest == 1297   # W = 16, c = 16, n = 1024 (poly_mul_ntt)
