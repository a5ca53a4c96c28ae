"""qTESLA's CDT Gaussian sampler and check_ES's sum as include/qtesla_ntt.h
states them for poly_sample_gauss and poly_hsum, written on
keccak_model.cshake_simple -- the definitions the two entry points are tested
against -- and the cumulative table the tests and the key-generation chain use.
Not a test.  About 50 ms per p-I polynomial, 250 ms per p-III polynomial."""
import functools
from decimal import Decimal, getcontext

import keccak_model as K

CHUNK = 512        # NTT_GAUSS_CHUNK
ROWS_MAX = 128     # NTT_GAUSS_ROWS_MAX
COLS_MAX = 4       # NTT_GAUSS_COLS_MAX
LIMB = 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def cdt_integers(sigma: str, rows: int, cols: int):
    """T_j = floor(2^(31 cols) * sum_{i <= j} D(i)) for j < rows, with D the
    half-Gaussian D(0) = 1/S, D(i) = 2 exp(-i^2 / 2 sigma^2) / S and
    S = 1 + 2 sum_{i >= 1} exp(-i^2 / 2 sigma^2), computed with `decimal` at 80
    digits (31 * 4 bits are 38 digits).  sigma is a decimal string."""
    getcontext().prec = 80
    sg = Decimal(sigma)
    two_s2 = 2 * sg * sg
    rho = lambda i: (-(Decimal(i) * i) / two_s2).exp()
    # the tail beyond 40 sigma is below 10^-340: nothing at 80 digits
    S = 1 + 2 * sum(rho(i) for i in range(1, int(40 * sg) + 2))
    scale = Decimal(1 << (31 * cols))
    acc, out = Decimal(0), []
    for j in range(rows):
        acc += (rho(j) if j == 0 else 2 * rho(j)) / S
        out.append(int((scale * acc).to_integral_value(rounding="ROUND_FLOOR")))
    return tuple(out)


def limbs(T: int, cols: int):
    """an integer below 2^(31 cols) as cols 31-bit limbs, most significant first"""
    return [(T >> (31 * (cols - 1 - k))) & LIMB for k in range(cols)]


def cdt_table(sigma, rows: int, cols: int):
    """[rows][cols] limbs of cdt_integers: with this table m = #{R >= T_j} of a
    uniform R below 2^(31 cols) has the half-Gaussian with P(m = 0) = D(0) (and
    P(m = rows) the tail beyond the table), and the free sign bit makes
    +-m the discrete Gaussian of parameter sigma.  This is this project's own
    table: upstream's constants are not reproduced here."""
    return [limbs(T, cols) for T in cdt_integers(str(sigma), rows, cols)]


def row_integers(table, cols: int):
    """the integers T_j a [rows][cols] table stands for (bit 31 of a word is ignored)"""
    return [sum((int(w) & LIMB) << (31 * (cols - 1 - k)) for k, w in enumerate(row)) for row in table]


def sample_words(seed: bytes, n: int, cols: int, algo: str, nonce: int):
    """the n samples' source words W_0 .. W_{cols-1}, chunk by chunk"""
    assert n % CHUNK == 0 and 1 <= cols <= COLS_MAX and 0 <= nonce <= 255
    out = []
    for ch in range(n // CHUNK):
        buf = K.cshake_simple(algo, seed, CHUNK * cols * 4, ((nonce << 8) + ch) & 0xFFFF)
        for i in range(CHUNK):
            out.append([int.from_bytes(buf[4 * (i * cols + k):4 * (i * cols + k) + 4], "little") for k in range(cols)])
    return out


def sample_value(words, cols: int):
    """R of one sample's words"""
    return sum((w & LIMB) << (31 * (cols - 1 - k)) for k, w in enumerate(words))


def sample_gauss(seed: bytes, n: int, q: int, table, cols: int, algo: str, nonce: int):
    """n coefficients in [0, q): (sign && m) ? q - m : m with m = #{j : R >= T_j}"""
    assert 1 <= len(table) <= ROWS_MAX and all(len(row) == cols for row in table)
    T = sorted(row_integers(table, cols))   # the count does not depend on the order
    import bisect
    out = []
    for words in sample_words(seed, n, cols, algo, nonce):
        m = bisect.bisect_right(T, sample_value(words, cols))
        out.append(q - m if (words[0] >> 31) and m else m)
    return out


def centred_abs(w, q: int):
    """|c| of poly_round's centred value, for entries < 2q"""
    return [min(x % q, q - x % q) for x in (int(v) for v in w)]


def hsum(w, q: int, h: int) -> int:
    """the sum of the h largest |c|, by a threshold: everything above the h-th
    largest value t, and t as often as is left (test_gauss_model compares it
    with sort-and-sum)"""
    a = centred_abs(w, q)
    assert 1 <= h <= len(a)
    t = sorted(a)[len(a) - h]
    above = [x for x in a if x > t]
    return sum(above) + (h - len(above)) * t
