"""Keccak-f[1600] in gather form: the round of csrc/ntt_xof_wave.hpp restated
in plain Python.  State word i = x + 5 y; g(v, idx) means "the holder of word
i reads v[idx[i]]"; every index table is a per-lane constant.  Also the
kernel's placement of the words in the lanes of a 32-lane half and the row
gathers as lane shifts.  Not a test (tests/test_keccak_wave_model.py compares
it with keccak_model)."""
import keccak_model as K

M64 = K.M64
WORDS = range(25)


def src(j):
    """pi inverted: b[j] = r[src(j)]"""
    return (j % 5 + 3 * (j // 5)) % 5 + 5 * (j % 5)


def row(i, dx):
    """word (x + dx) mod 5 of word i's row"""
    return (i % 5 + dx) % 5 + 5 * (i // 5)


UP5 = [(i + 5) % 25 for i in WORDS]
UP10 = [(i + 10) % 25 for i in WORDS]
UP20 = [(i + 20) % 25 for i in WORDS]
XM1 = [row(i, 4) for i in WORDS]
XP1 = [row(i, 1) for i in WORDS]
XP2 = [row(i, 2) for i in WORDS]
PI = [src(i) for i in WORDS]
TABLES = {"UP5": UP5, "UP10": UP10, "UP20": UP20, "XM1": XM1, "XP1": XP1, "XP2": XP2, "PI": PI}


def g(v, idx):
    return [v[idx[i]] for i in WORDS]


def rotr_var(v, n):
    """the kernel's variable rotate: right by n = 32 s + k as a swap of the dwords if s, then two 32-bit funnel shifts
    by k (k = 0 is the funnel shift's count 0)"""
    lo, hi = v & 0xFFFFFFFF, v >> 32
    if n & 32:
        lo, hi = hi, lo
    k = n & 31
    nlo = (((hi << 32) | lo) >> k) & 0xFFFFFFFF
    nhi = (((lo << 32) | hi) >> k) & 0xFFFFFFFF
    return (nhi << 32) | nlo


def keccak_round(a, rc):
    s1 = [a[i] ^ t for i, t in zip(WORDS, g(a, UP5))]
    c = [s1[i] ^ t ^ u for i, t, u in zip(WORDS, g(s1, UP10), g(a, UP20))]
    d = [t ^ K.rotl(u, 1) for t, u in zip(g(c, XM1), g(c, XP1))]
    r = [rotr_var(a[i] ^ d[i], (64 - K.RHO[i]) & 63) for i in WORDS]
    b = g(r, PI)
    a = [b[i] ^ (~t & M64 & u) for i, t, u in zip(WORDS, g(b, XP1), g(b, XP2))]
    a[0] ^= rc
    return a


def keccak_f1600(a):
    """25 words (word x + 5 y) -> 25 words"""
    a = list(a)
    for rc in K.RC:
        a = keccak_round(a, rc)
    return a


# -- placement: which lane of a 32-lane half holds word i, and the row gathers as shifts within a 16-lane row ----------

def lane_of(i):
    """rows 0 .. 2 in lanes 0 .. 14, rows 3 and 4 in lanes 16 .. 25"""
    return i + (i >= 15)


def word_of(lane):
    """the word a lane of a half holds, None for a passenger (lanes 15 and 26 .. 31)"""
    if lane == 15 or lane >= 26:
        return None
    return lane - (lane > 15)


def row_shift(v32, k, x_of):
    """the kernel's row gather over the 32 lanes of a half: every lane reads lane + k of its 16-lane row where
    x + k < 5, lane + k - 5 otherwise; a lane outside the 16-lane row reads 0"""
    def read(lane, src):
        return v32[src] if 0 <= src < 32 and src // 16 == lane // 16 else 0
    return [read(lane, lane + k - 5) if x_of(lane) + k >= 5 else read(lane, lane + k) for lane in range(32)]


def keccak_round_placed(v32, rc):
    """the round on the 32 lanes of a half, passengers holding whatever they hold: the column gathers and pi through
    lane_of, the row gathers by row_shift"""
    def x_of(lane):
        i = word_of(lane)
        return 0 if i is None else i % 5

    def gather(v, table):
        return [v[lane] if word_of(lane) is None else v[lane_of(table[word_of(lane)])] for lane in range(32)]

    lanes = range(32)
    s1 = [v32[l] ^ t for l, t in zip(lanes, gather(v32, UP5))]
    c = [s1[l] ^ t ^ u for l, t, u in zip(lanes, gather(s1, UP10), gather(v32, UP20))]
    d = [t ^ K.rotl(u, 1) for t, u in zip(row_shift(c, 4, x_of), row_shift(c, 1, x_of))]
    rho = [0 if word_of(l) is None else K.RHO[word_of(l)] for l in lanes]
    r = [rotr_var(v32[l] ^ d[l], (64 - rho[l]) & 63) for l in lanes]
    b = gather(r, PI)
    out = [b[l] ^ (~t & M64 & u) for l, t, u in zip(lanes, row_shift(b, 1, x_of), row_shift(b, 2, x_of))]
    out[lane_of(0)] ^= rc
    return out
