"""poly_pack / poly_unpack in numpy: the statement of include/qtesla_ntt.h.

A polynomial's packed form is n b / 8 bytes; field i occupies stream bits
[i b, (i+1) b), and stream bit j is bit j mod 8 of byte j / 8 (np.packbits /
np.unpackbits with bitorder="little").  Not a test."""
import numpy as np

PRIMES = {"ref": 8404993, "p-I": 343576577, "p-III": 856145921, "p-III-4096": 856145921, "p-III-8192": 856145921}


def qbits(q: int) -> int:
    return int(q).bit_length()


def bits_range(q: int, signed: bool):
    """the legal field widths: 8 .. qbits - 1 signed, 8 .. qbits unsigned"""
    return range(8, qbits(q) - (1 if signed else 0) + 1)


def fields(w, q: int, bits: int, signed: bool) -> np.ndarray:
    """poly_pack's field of every word of w (entries < 2q): uint32 < 2^bits"""
    x = np.asarray(w).astype(np.int64) % q
    c = np.where(x > (q - 1) // 2, x - q, x) if signed else x
    return (c & ((1 << bits) - 1)).astype("<u4")


def pack_fields(f, bits: int) -> np.ndarray:
    """fields [..., n] (uint32 < 2^bits) to bytes [..., n * bits / 8]"""
    f = np.ascontiguousarray(f, dtype="<u4")
    bit = np.unpackbits(f[..., None].view(np.uint8), axis=-1, bitorder="little")[..., :bits]   # [..., n, bits]
    return np.packbits(bit.reshape(*f.shape[:-1], f.shape[-1] * bits), axis=-1, bitorder="little")


def unpack_fields(b, n: int, bits: int) -> np.ndarray:
    """bytes [..., n * bits / 8] to fields [..., n] (uint32 < 2^bits)"""
    b = np.asarray(b, dtype=np.uint8)
    assert b.shape[-1] * 8 == n * bits
    bit = np.unpackbits(b, axis=-1, bitorder="little").reshape(*b.shape[:-1], n, bits)
    full = np.zeros((*b.shape[:-1], n, 32), dtype=np.uint8)
    full[..., :bits] = bit
    return np.packbits(full, axis=-1, bitorder="little").view("<u4")[..., 0]


def poly_pack(w, q: int, bits: int, signed: bool) -> np.ndarray:
    """w [..., n] uint32 entries < 2q -> uint8 [..., n * bits / 8]"""
    return pack_fields(fields(w, q, bits, signed), bits)


def poly_unpack(b, n: int, q: int, bits: int, signed: bool):
    """uint8 [..., n * bits / 8] -> (canonical uint32 [..., n], maxima uint32 [...]):
    signed, the maximum of |sign-extended field|; unsigned, the largest raw field"""
    f = unpack_fields(b, n, bits).astype(np.int64)
    if signed:
        s = np.where(f >= 1 << (bits - 1), f - (1 << bits), f)
        return np.where(s < 0, s + q, s).astype(np.uint32), np.abs(s).max(axis=-1).astype(np.uint32)
    return np.where(f < q, f, f - q).astype(np.uint32), f.max(axis=-1).astype(np.uint32)


def pack_rows(w, q: int, bits: int, signed: bool, stride: int, gap=None) -> np.ndarray:
    """w [batch, k, n] -> rows uint8 [batch, stride]: the k polynomials back to
    back, then `gap` (uint8 [batch, stride - k n bits / 8], zeros if None)"""
    w = np.asarray(w)
    batch, k, n = w.shape
    packed = k * n * bits // 8
    rows = np.zeros((batch, stride), dtype=np.uint8)
    rows[:, :packed] = poly_pack(w, q, bits, signed).reshape(batch, packed)
    if gap is not None:
        rows[:, packed:] = gap
    return rows


def unpack_rows(rows, k: int, n: int, q: int, bits: int, signed: bool):
    """rows uint8 [batch, stride] -> (w [batch, k, n], maxima [batch, k])"""
    rows = np.asarray(rows, dtype=np.uint8)
    packed = k * n * bits // 8
    return poly_unpack(rows[:, :packed].reshape(rows.shape[0], k, packed // k), n, q, bits, signed)
