"""poly_unpack_ntt in numpy: the statement of include/qtesla_ntt.h.

pack_model.unpack_rows (the canonical polynomials poly_unpack gives and their
maxima), then the oracle's poly_ntt (natural order, the library's psi), then
the entrywise negation mod q with 0 staying 0.  Not a test."""
import numpy as np

import pack_model


def unpack_ntt_rows(oracle, rows, ps: str, k: int, bits: int, signed: bool, neg: bool):
    """rows uint8 [batch, stride] -> (X uint32 [batch, k, n] canonical, maxima uint32 [batch, k])"""
    p = oracle.params(ps)
    n, q = p["n"], p["q"]
    x, mx = pack_model.unpack_rows(rows, k, n, q, bits, signed)
    X = oracle.poly_ntt(np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, n), ps).reshape(x.shape)
    if neg:
        X = ((q - X.astype(np.int64)) % q).astype(np.uint32)
    return X, mx


def place(X, pstride: int, fill, total=None) -> np.ndarray:
    """X [batch, k, n] at pstride words per polynomial in a flat array of
    `total` words (default: ending with the last polynomial) otherwise `fill`"""
    X = np.asarray(X)
    npoly, n = X.shape[0] * X.shape[1], X.shape[-1]
    total = (npoly - 1) * pstride + n if total is None else total
    out = np.full(total, fill, dtype=np.uint32)
    idx = (np.arange(npoly)[:, None] * pstride + np.arange(n)[None, :]).reshape(-1)
    out[idx] = X.reshape(-1)
    return out
