"""Plain-Python Keccak-f[1600], the sponge, NIST cSHAKE (SP 800-185) with
general N and S, qTESLA's cshake*_simple and its challenge expansion
enc(seed, n, q, h) -- the definitions ntt_xof and poly_challenge are tested
against.  Not a test.  About 1 ms per permutation: for short inputs only
(hashlib serves the long SHAKE cases)."""

RATE = {"shake128": 168, "shake256": 136}
BLOCK_DRAWS = 56   # three-byte draws in one 168-byte block
M64 = (1 << 64) - 1

RC = []
RHO = [0] * 25   # rotation of lane x + 5 y


def _init():
    r = 1
    for _ in range(24):
        c = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) & 0xFF
            if r & 2:
                c ^= 1 << ((1 << j) - 1)
        RC.append(c)
    x, y = 1, 0
    for t in range(24):
        RHO[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5


_init()


def rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f1600(a):
    """25 lanes (lane x + 5 y) -> 25 lanes"""
    a = list(a)
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], RHO[x + 5 * y])
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & M64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        a[0] ^= rc
    return a


def sponge(rate: int, data: bytes, domain: int, outlen: int) -> bytes:
    """pad10*1 with the domain bits in `domain` (0x1F SHAKE, 0x04 cSHAKE)"""
    p = bytearray(data) + bytes([domain])
    p += bytes(-len(p) % rate)
    p[-1] ^= 0x80
    a = [0] * 25
    for o in range(0, len(p), rate):
        for i in range(rate // 8):
            a[i] ^= int.from_bytes(p[o + 8 * i:o + 8 * i + 8], "little")
        a = keccak_f1600(a)
    out = b""
    while True:
        out += b"".join(v.to_bytes(8, "little") for v in a[:rate // 8])
        if len(out) >= outlen:
            return out[:outlen]
        a = keccak_f1600(a)


def shake(algo: str, data: bytes, outlen: int) -> bytes:
    return sponge(RATE[algo], data, 0x1F, outlen)


def left_encode(v: int) -> bytes:
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return bytes([len(b)]) + b


def encode_string(s: bytes) -> bytes:
    return left_encode(8 * len(s)) + s


def bytepad(x: bytes, w: int) -> bytes:
    z = left_encode(w) + x
    return z + bytes(-len(z) % w)


def cshake(algo: str, data: bytes, outlen: int, N: bytes = b"", S: bytes = b"") -> bytes:
    if not N and not S:
        return shake(algo, data, outlen)
    rate = RATE[algo]
    return sponge(rate, bytepad(encode_string(N) + encode_string(S), rate) + data, 0x04, outlen)


def cshake_simple_prefix(algo: str, cstm: int) -> bytes:
    """the block qTESLA's cshake*_simple absorbs first, written out"""
    rate = RATE[algo]
    return bytes([0x01, rate, 0x01, 0x00, 0x01, 0x10, cstm & 0xFF, cstm >> 8]) + bytes(rate - 8)


def cshake_simple(algo: str, data: bytes, outlen: int, cstm: int) -> bytes:
    assert 0 <= cstm <= 0xFFFF
    return sponge(RATE[algo], cshake_simple_prefix(algo, cstm) + data, 0x04, outlen)


def xof(algo: str, data: bytes, outlen: int, cstm: int = -1) -> bytes:
    """ntt_xof's definition"""
    return shake(algo, data, outlen) if cstm < 0 else cshake_simple(algo, data, outlen, cstm)


def seeds(count: int, length: int = 32):
    """the fixed seeds of the CPU and GPU tests (SHAKE256 of a label, by hashlib)"""
    import hashlib
    return [hashlib.shake_256(b"qtesla-ntt challenge seed %d" % i).digest(length) for i in range(count)]


def enc(seed: bytes, n: int, q: int, h: int, stats=None):
    """qTESLA's encode_c: (pos, val), h entries each.  stats, if a dict, gets
    the number of blocks squeezed and of draws rejected as collisions."""
    dmsp = 0
    r = cshake_simple("shake128", seed, 168, dmsp)
    dmsp += 1
    cnt = rejected = 0
    pos, val, taken = [], [], set()
    while len(pos) < h:
        if cnt > 168 - 3:
            r = cshake_simple("shake128", seed, 168, dmsp)
            dmsp += 1
            cnt = 0
        p = ((r[cnt] << 8) | r[cnt + 1]) & (n - 1)
        if p not in taken:
            taken.add(p)
            pos.append(p)
            val.append(q - 1 if r[cnt + 2] & 1 else 1)
        else:
            rejected += 1
        cnt += 3
    if stats is not None:
        stats["blocks"] = dmsp
        stats["rejected"] = rejected
    return pos, val
