"""qTESLA's GenA (poly_uniform) as include/qtesla_ntt.h states it for
poly_gen_a, written on keccak_model.cshake_simple -- the definition poly_gen_a
is tested against, in its two forms: the literal loop of the header and the
flat draw stream the kernel walks.  Not a test.  About 1 ms per permutation:
0.05 s per n = 1024 polynomial."""
import keccak_model as K

RATE = 168
BLOCKS_MAX = 256   # NTT_GEN_A_BLOCKS_MAX


def qbits(q: int) -> int:
    return q.bit_length()


def nbytes(q: int) -> int:
    return (qbits(q) + 7) // 8


def draws_per_call(nblocks: int, nb: int = 4) -> int:
    """draws a call of `nblocks` rate blocks gives, in groups of four draws of nb bytes"""
    return 4 * (RATE * nblocks // (4 * nb))


def refills_max(k: int, n: int) -> int:
    """the bound on single-block refills: a function of the arguments alone"""
    return min(65535, 4 * -(-(k * n) // 40))


def _le32(buf: bytes, pos: int) -> int:
    return int.from_bytes(buf[pos:pos + 4].ljust(4, b"\0"), "little")


def gen_a(seed: bytes, k: int, n: int, q: int, nblocks: int, stats=None):
    """The literal loop.  k lists of n values in [0, q); stats, if a dict, gets
    the number of refills and of draws rejected."""
    assert 1 <= nblocks <= BLOCKS_MAX
    nby, mask = nbytes(q), (1 << qbits(q)) - 1
    buf = K.cshake_simple("shake128", seed, RATE * nblocks, 0)
    nb, pos, dmsp, rejected = nblocks, 0, 1, 0
    a = []
    while len(a) < k * n:
        if pos > RATE * nb - 4 * nby:
            if dmsp - 1 == refills_max(k, n):   # not reachable by hash outputs: the rest is 0
                a += [0] * (k * n - len(a))
                break
            nb, buf, pos = 1, K.cshake_simple("shake128", seed, RATE, dmsp), 0
            dmsp += 1
        for _ in range(4):
            v = _le32(buf, pos) & mask
            pos += nby
            if v < q and len(a) < k * n:
                a.append(v)
            elif v >= q:
                rejected += 1
    if stats is not None:
        stats["refills"] = dmsp - 1
        stats["rejected"] = rejected
    return [a[i * n:(i + 1) * n] for i in range(k)]


def gen_a_flat(seed: bytes, k: int, n: int, q: int, nblocks: int):
    """The flat draw stream: the first call's draws_per_call(nblocks) draws,
    then draws_per_call(1) per refill, each draw accepted when < q."""
    nby, mask = nbytes(q), (1 << qbits(q)) - 1
    a, call = [], 0
    while len(a) < k * n and call <= refills_max(k, n):
        blocks = nblocks if call == 0 else 1
        buf = K.cshake_simple("shake128", seed, RATE * blocks, call)
        for d in range(draws_per_call(blocks, nby)):
            v = _le32(buf, d * nby) & mask
            if v < q and len(a) < k * n:
                a.append(v)
        call += 1
    a += [0] * (k * n - len(a))
    return [a[i * n:(i + 1) * n] for i in range(k)]
