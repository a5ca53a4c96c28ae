"""numpy model of poly_round (include/qtesla_ntt.h): qTESLA's rounding [.]_M
and the two norm maxima, restated.  For x < 2q and a bit count d:

    x' = x mod q
    c  = x' > (q-1)/2 ? x' - q : x'
    lo = c mod+- 2^d  in (-2^(d-1), 2^(d-1)]
    hi = (c - lo) >> d

The two forms in which qTESLA's C code writes it are here too, for the tests
that tie the model to them.
"""
import numpy as np

# qTESLA's own d per parameter set (ref / p-I / p-III; the n = 4096 / 8192 sets share p-III's prime)
OWN_D = {"ref": 22, "p-I": 22, "p-III": 24, "p-III-4096": 24, "p-III-8192": 24}


def centre(x, q):
    """c as int64, |c| <= (q-1)/2."""
    xp = np.asarray(x).astype(np.int64) % q
    return np.where(xp > (q - 1) // 2, xp - q, xp)


def split(x, q, d):
    """(c, lo, hi) as int64 arrays."""
    c = centre(x, q)
    t = c & ((1 << d) - 1)
    lo = np.where(t > (1 << (d - 1)), t - (1 << d), t)
    hi = (c - lo) >> d
    return c, lo, hi


def hi_shift_form(x, q, d):
    """test_correctness's form: (c + 2^(d-1) - 1) >> d, arithmetic shift."""
    return (centre(x, q) + (1 << (d - 1)) - 1) >> d


def hi_mask_form(x, q, d):
    """The hash input's form: lo from the mask, corrected where it exceeds
    2^(d-1) by a sign-bit trick, then (c - lo) >> d."""
    c = centre(x, q)
    t = c & ((1 << d) - 1)
    t = t - ((((1 << (d - 1)) - t) >> 63) & (1 << d))   # minus 2^d where t > 2^(d-1)
    return (c - t) >> d


def hmax(q, d):
    """The largest hi; hi fits a signed byte iff this is <= 127."""
    return ((q - 1) // 2 + (1 << (d - 1)) - 1) >> d


def min_d(q):
    """The smallest d at which hi fits a signed byte."""
    return next(d for d in range(1, 31) if hmax(q, d) <= 127)


def edge_values(q, d):
    """The inputs at which a branch of the definition flips, all < 2q."""
    h, m = 1 << (d - 1), (q - 1) // 2
    vals = [0, 1, m, m - 1, m + 1, q - 1, h, h - 1, h + 1, q - h, q - h - 1, q - h + 1, q, 2 * q - 1]
    return np.array([v for v in vals if 0 <= v < 2 * q], dtype=np.uint32)


def poly_round(w, q, d):
    """w [..., n] uint32 < 2q -> (hi int8 [..., n], norms uint32 [..., 2])."""
    c, lo, hi = split(w, q, d)
    assert hi.min() >= -128 and hi.max() <= 127, "d too small for a byte"
    norms = np.stack([np.abs(c).max(axis=-1), np.abs(lo).max(axis=-1)], axis=-1).astype(np.uint32)
    return hi.astype(np.int8), norms
