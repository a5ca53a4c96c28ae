"""qTESLA's masking-polynomial sampler sample_y as include/qtesla_ntt.h states
it for poly_sample_y, written on keccak_model.cshake_simple -- the definition
poly_sample_y is tested against.  Not a test.  About 30 ms per n = 2048
polynomial."""
import keccak_model as K

REFILLS_MAX = 255   # NTT_SAMPLE_Y_REFILLS_MAX


def sample_y(seed: bytes, n: int, q: int, bits: int, algo: str, nonce: int, stats=None):
    """n coefficients in [0, q), centred in [-B, B] with B = 2^(bits-1) - 1.
    stats, if a dict, gets the number of draws rejected and of refills."""
    assert 2 <= bits <= 24 and 0 <= nonce <= 255
    rate = K.RATE[algo]
    mask = (1 << bits) - 1
    B = (1 << (bits - 1)) - 1
    cstm = (nonce << 8) & 0xFFFF
    buf = K.cshake_simple(algo, seed, 3 * n, cstm)
    limit, pos, r, rejected = 3 * n, 0, 0, 0
    y = []
    while len(y) < n:
        if pos >= limit:
            if r == REFILLS_MAX:        # not reachable by hash outputs: the rest is 0
                y += [0] * (n - len(y))
                break
            r += 1
            buf = K.cshake_simple(algo, seed, rate, (cstm + r) & 0xFFFF)
            limit, pos = 3 * (rate // 3), 0
        v = (buf[pos] | buf[pos + 1] << 8 | buf[pos + 2] << 16) & mask
        pos += 3
        if v != mask:
            y.append((v - B) % q)
        else:
            rejected += 1
    if stats is not None:
        stats["rejected"] = rejected
        stats["refills"] = r
    return y
