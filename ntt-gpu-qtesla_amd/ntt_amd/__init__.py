"""ntt_amd -- Python host binding of the MI355X batched negacyclic NTT engine.

Thin ctypes layer over the C ABI in include/qtesla_ntt.h (libqtesla_ntt.so,
built in-tree for gfx950).  PyTorch is used only as plumbing: device memory
(int32 tensors carry the uint32 coefficient bit patterns), the current HIP
stream and torch.distributed.  There is no CPU fallback: if the HIP library
is missing every call raises.

Names and argument meaning follow the reference's GPU pipeline
(benlwk/ntt-gpu-qTESLA NTT.cu):
  poly_ntt      -- bit_reverse_copy_tbl_Phi_gpu + radix2NTT_gpu0/1 (NTT.cu:2388-2400)
  poly_invntt   -- GS_radix2INTT_gpu0/2 + bit_reverse_copy_tbl_invPhi_gpu (:2415-2425)
  poly_mul      -- the whole CT-GS poly-mul driver (test_NTT_CT_GS_nega_gpu, :2358)
  poly_pointwise -- pointwise_mult (:1155-1160)
  poly_mul_nussbaumer -- nussbaumer_fft (:167-277), batched, n = 1024 / 2048
  poly_ntt_bitrev / poly_invntt_bitrev -- the CT-CT ordering: bit-reversed
                   NTT domain (radix2INTT_gpu0/1/2 on bit-reversed input, :2240-2249)

Every torch wrapper runs on its tensors' device (all operands must share
one) and, by default, on that device's current stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._abi import *  # noqa: F401,F403 -- paths, constants, SIGNATURES, lib, NTTError: this package's names too
from ._abi import _FN, _sz, _u32p, _vp


def _ps(param_set) -> int:
    return PARAM_SETS[param_set] if isinstance(param_set, str) else int(param_set)


def _check(rc: int, where: str):
    if rc != NTT_OK:
        raise NTTError(rc, where)


_PARAM_CACHE: dict = {}
_N_CACHE: dict = {}


def _n(param_set) -> int:
    """n of a parameter set, cached (the per-call wrappers' fast path)."""
    n = _N_CACHE.get(param_set)
    if n is None:
        n = _N_CACHE[param_set] = param_info(param_set)["n"]
    return n


def param_info(param_set) -> dict:
    """n, q, psi, omega, omega^-1, n^-1 of a parameter set (immutable: cached,
    so that the per-call wrappers cost no extra library call)."""
    ps = _ps(param_set)
    info = _PARAM_CACHE.get(ps)
    if info is None:
        vals = [ctypes.c_uint32() for _ in range(6)]
        _check(lib().ntt_param_info(ps, *[ctypes.byref(v) for v in vals]), "ntt_param_info")
        info = _PARAM_CACHE[ps] = dict(zip(("n", "q", "psi", "omega", "omega_inv", "n_inv"), (v.value for v in vals)))
    return dict(info)


def tables(param_set) -> dict:
    n = _n(param_set)
    names = ("bitrev_tbl", "Phi", "invPhi", "tf0", "ti0")
    out = {k: np.zeros(n, np.uint32) for k in names}
    _check(lib().ntt_get_tables(_ps(param_set), *(out[k].ctypes.data_as(_u32p) for k in names)), "ntt_get_tables")
    return out


def sync_expiries() -> int:
    """Expired bounded waits of the n = 4096 / 8192 kernels on the current
    device (0 unless a per-polynomial barrier broke; see qtesla_ntt.h)."""
    v = ctypes.c_uint32()
    _check(lib().ntt_sync_expiries(ctypes.byref(v)), "ntt_sync_expiries")
    return v.value


def small_batch_max(param_set, op: str) -> int:
    """Largest batch for which entry point `op` (a SWITCH_OPS key) runs the
    small-batch kernels, one polynomial per workgroup (0: never)."""
    v = _sz()
    _check(lib().ntt_small_batch_max(_ps(param_set), SWITCH_OPS[op], ctypes.byref(v)), "ntt_small_batch_max")
    return v.value


def small_batch_radix(param_set, op: str, batch: int) -> int:
    """Radix of the one-polynomial-per-workgroup kernel entry point `op`
    runs at `batch` polynomials (4 / 8 / 16), 0 for the batch kernels."""
    v = ctypes.c_int()
    _check(lib().ntt_small_batch_radix(_ps(param_set), SWITCH_OPS[op], batch, ctypes.byref(v)), "ntt_small_batch_radix")
    return v.value


def build_info() -> str:
    buf = ctypes.create_string_buffer(1024)
    lib().ntt_build_info(buf, 1024)
    return buf.value.decode()


def build_hash() -> str:
    """Hash of the library sources the loaded .so was built from ("src=" field)."""
    info = build_info()
    return info.rsplit("src=", 1)[1].strip() if "src=" in info else "unknown"


# ------------------------------------------------------------- torch API

_TORCH = None
_INT_DTYPES = ()
_BYTE_DTYPES = ()
_RAW_STREAM = None


def _torch():
    """torch, imported on first use (this module also serves torch-free
    ctypes callers) and then cached: the per-call wrappers below run once per
    polynomial in the signing loop's small calls."""
    global _TORCH, _INT_DTYPES, _BYTE_DTYPES, _RAW_STREAM
    if _TORCH is None:
        import torch
        _INT_DTYPES = (torch.int32, getattr(torch, "uint32", torch.int32))
        _BYTE_DTYPES = (torch.int8, torch.uint8)
        # torch's raw accessor where this torch build has it (no Stream
        # object: ~1.4 us less per call, tools/call_overhead.py)
        _RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        _TORCH = torch
    return _TORCH


def _same_device(tensors):
    """All operands (None: an optional one not given) live on one device
    (ValueError otherwise)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not getattr(t, "is_cuda", False):
            raise ValueError("ntt_amd operates on device tensors only (no CPU fallback)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"operands on different devices: {dev} and {t.device}")


def _stream(stream, device=None):
    """The stream's handle (hipStream_t) as an int: of a torch Stream or an
    int as given, of None `device`'s current stream (a torch.device, an
    index, or None for the current device)."""
    if stream is not None:
        return getattr(stream, "cuda_stream", stream)
    if type(device) is not int:
        torch = _torch()
        if isinstance(device, torch.device) and device.index is not None:
            return _stream(None, device.index)
        return torch.cuda.current_stream(device).cuda_stream
    return _RAW_STREAM(device) if _RAW_STREAM is not None else _torch().cuda.current_stream(device).cuda_stream


def _batch(t, n: int, dtypes=None, storage="int32/uint32") -> int:
    _torch()
    if not t.is_cuda:
        raise ValueError("ntt_amd operates on device tensors only (no CPU fallback)")
    if t.dtype not in (dtypes or _INT_DTYPES):
        raise TypeError(f"expected {storage} storage, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous (poly-major [batch][n])")
    numel = t.numel()
    if numel % n:
        raise ValueError(f"numel {numel} is not a multiple of n={n}")
    return numel // n


def _byte_batch(t) -> int:
    """_batch of an int8/uint8 tensor in bytes."""
    _torch()
    return _batch(t, 1, _BYTE_DTYPES, "int8/uint8")


def _run(name: str, tensors, stream, *args):
    """The call path of the device entry points (_inplace runs the same steps
    in line for the in-place transforms): check that the operands
    (None: an optional one not given) share a device, make it current unless
    it is, and call the ABI's `name` as fn(*args, stream) -- each of them takes
    the stream last.  An error names the entry point less its "_path" suffix
    (ntt_xof_path is how ntt_xof is called)."""
    t = tensors[0]
    if len(tensors) > 1 or not getattr(t, "is_cuda", False):
        _same_device(tensors)
    torch = _TORCH or _torch()
    dev = t.get_device()   # an int: no torch.device object
    fn = _FN.get(name)
    if fn is None:
        lib()
        fn = _FN[name]
    s = _stream(stream, dev)
    if torch.cuda.current_device() == dev:   # already current: no device switch
        rc = fn(*args, s)
    else:
        with torch.cuda.device(dev):
            rc = fn(*args, s)
    if rc != NTT_OK:
        raise NTTError(rc, name.removesuffix("_path"))


def _ptr(t):
    """The device pointer of an optional operand (None: NULL)."""
    return None if t is None else t.data_ptr()


def _same_batch(n: int, first, *others) -> int:
    b = _batch(first, n)
    for o in others:
        if _batch(o, n) != b:
            raise ValueError("batch mismatch")
    return b


def _inplace(name: str, t, param_set, stream):
    """The in-place transforms, the signing loop's one-polynomial calls
    (config 1): _batch's checks in one test, _batch itself only for its error
    text, and _run's steps for its one tensor in line, with _run's _stream --
    through _run itself bench config 1 lost ~0.3 of its ~4.2 us per call
    (profiles/binding_call_path/)."""
    n = _N_CACHE.get(param_set) or _n(param_set)
    numel = t.numel()
    if not t.is_cuda or t.dtype not in _INT_DTYPES or not t.is_contiguous() or numel % n:
        _batch(t, n)   # raises the specific error; passes once, before torch is cached
    torch = _TORCH or _torch()
    fn = _FN.get(name)
    if fn is None:
        lib()
        fn = _FN[name]
    ps = PARAM_SETS[param_set] if isinstance(param_set, str) else int(param_set)
    dev = t.get_device()
    s = _stream(stream, dev)
    if torch.cuda.current_device() == dev:
        rc = fn(t.data_ptr(), None, numel // n, ps, s)
    else:
        with torch.cuda.device(dev):
            rc = fn(t.data_ptr(), None, numel // n, ps, s)
    if rc != NTT_OK:
        raise NTTError(rc, name)
    return t


def poly_ntt(t, param_set, stream=None):
    """In-place forward negacyclic NTT of a [batch, n] device tensor."""
    return _inplace("poly_ntt", t, param_set, stream)


def poly_invntt(t, param_set, stream=None):
    """In-place inverse negacyclic NTT (includes n^-1 and psi^-i)."""
    return _inplace("poly_invntt", t, param_set, stream)


def _oop(name, out, inp, param_set, stream):
    n = _n(param_set)
    b = _same_batch(n, inp, out)
    _run(name, (out, inp), stream, out.data_ptr(), inp.data_ptr(), b, _ps(param_set))
    return out


def poly_ntt_oop(out, inp, param_set, stream=None):
    return _oop("poly_ntt_oop", out, inp, param_set, stream)


def poly_invntt_oop(out, inp, param_set, stream=None):
    return _oop("poly_invntt_oop", out, inp, param_set, stream)


def poly_ntt_bitrev(out, inp, param_set, stream=None):
    """Forward NTT with bit-reversed output order: out[b, t] = X[b, brv(t)]."""
    return _oop("poly_ntt_bitrev", out, inp, param_set, stream)


def poly_invntt_bitrev(out, inp, param_set, stream=None):
    """Inverse NTT of a bit-reversed-order input (inp[b, t] = X[b, brv(t)])."""
    return _oop("poly_invntt_bitrev", out, inp, param_set, stream)


def poly_bitrev_copy(out, inp, param_set, stream=None):
    """out[b, t] = inp[b, brv(t)] (bit_reverse_copy_tbl_gpu); out may be inp."""
    return _oop("poly_bitrev_copy", out, inp, param_set, stream)


def _mul(name, c, a, b, param_set, stream, *extra):
    n = _n(param_set)
    nb = _same_batch(n, a, b, c)
    _run(name, (c, a, b), stream, c.data_ptr(), a.data_ptr(), b.data_ptr(), nb, _ps(param_set), *extra)
    return c


def poly_mul(c, a, b, param_set, stream=None):
    """c = a*b mod (x^n + 1, q), fused single launch."""
    return _mul("poly_mul", c, a, b, param_set, stream)


def poly_mul_ntt(c, a, bhat, param_set, stream=None):
    """c = a*b mod (x^n + 1, q) with bhat = poly_ntt(b) given (NTT domain)."""
    return _mul("poly_mul_ntt", c, a, bhat, param_set, stream)


def poly_mul_ntt_k(out, y, ahat, param_set, add=None, stream=None):
    """out[b, i] = a_i * y[b] (+ add[b, i]) mod (x^n + 1, q) for the k rows
    ahat[i] = poly_ntt(a_i), shared by the whole batch: one launch, y read and
    transformed once (qTESLA's t_i = a_i y + e_i).

    y is [batch, n], ahat [k, n] with k = ahat.numel() // n, out and add
    [batch, k, n]; add may be out (accumulate in place)."""
    n = _n(param_set)
    k, nb = ahat.numel() // n, y.numel() // n
    if ahat.numel() != k * n or not 1 <= k <= MUL_K_MAX:
        raise ValueError(f"ahat: numel {ahat.numel()} is not k*n with 1 <= k <= {MUL_K_MAX} (n={n})")
    if y.numel() != nb * n:
        raise ValueError(f"y: numel {y.numel()} is not a multiple of n={n}")
    if out.numel() != nb * k * n:
        raise ValueError(f"out: numel {out.numel()} is not batch*k*n = {nb}*{k}*{n}")
    if add is not None and add.numel() != nb * k * n:
        raise ValueError(f"add: numel {add.numel()} is not batch*k*n = {nb}*{k}*{n}")
    for t in (out, y, ahat) if add is None else (out, y, ahat, add):
        _batch(t, n)   # device, dtype, contiguity
    _run("poly_mul_ntt_k", (out, y, ahat, add), stream,
         out.data_ptr(), y.data_ptr(), ahat.data_ptr(), _ptr(add), nb, k, _ps(param_set))
    return out


def mul_k_shape(param_set) -> dict:
    """Launch shape of poly_mul_ntt_k (ntt_mul_k_shape): "split_max", the
    largest batch whose k rows are spread over k workgroups (0: never), and
    "waves", the work units (one n = 2048 polynomial or two n = 1024
    polynomials each) of a workgroup."""
    v, w = _sz(), ctypes.c_int()
    _check(lib().ntt_mul_k_shape(_ps(param_set), ctypes.byref(v), ctypes.byref(w)), "ntt_mul_k_shape")
    return {"split_max": v.value, "waves": w.value}


def poly_mul_ntt_kl(out, ys, ahat, param_set, add=None, stream=None):
    """out[b, i] = sum_j a_ij * ys[j][b] (+ add[b, i]) mod (x^n + 1, q) for the
    k x l matrix ahat[i, j] = poly_ntt(a_ij), shared by the whole batch: one
    launch, the l products of a row summed in the NTT domain (qTESLA's
    verification w_i = a_i z - t_i c with ys = (z, c), ahat[i] = (a_i-hat,
    q - t_i-hat)).

    ys is a sequence of l tensors [batch, n] (separate allocations or views,
    used where they lie), ahat [k, l, n] with k = ahat.numel() // (l * n), out
    and add [batch, k, n]; add may be out (accumulate in place)."""
    py, pa, nb, k, l, tensors = _rows_operands(_n(param_set), ys, ahat, add, out)
    _run("poly_mul_ntt_kl", tensors, stream, out.data_ptr(), py, ahat.data_ptr(), pa, nb, k, l, _ps(param_set))
    return out


def _rows_operands(n: int, ys, ahat, add, out=None):
    """The operands of poly_mul_ntt_kl / poly_mul_ntt_kl_round, checked: the
    host array of the ys' pointers (read during the call only), add's pointer
    or None, batch, k, l and the tensors given, for _run."""
    ys = tuple(ys)
    l = len(ys)
    if not 1 <= l <= MUL_L_MAX:
        raise ValueError(f"ys: {l} tensors, expected 1 .. {MUL_L_MAX}")
    nb = ys[0].numel() // n
    for j, y in enumerate(ys):
        if y.numel() != nb * n:
            raise ValueError(f"ys: numel of ys[{j}] = {y.numel()} is not batch*n = {nb}*{n}, one batch for all")
    k = ahat.numel() // (l * n)
    if ahat.numel() != k * l * n or not 1 <= k <= MUL_K_MAX:
        raise ValueError(f"ahat: numel {ahat.numel()} is not k*l*n with 1 <= k <= {MUL_K_MAX} (l={l}, n={n})")
    if out is not None and out.numel() != nb * k * n:
        raise ValueError(f"out: numel {out.numel()} is not batch*k*n = {nb}*{k}*{n}")
    if add is not None and add.numel() != nb * k * n:
        raise ValueError(f"add: numel {add.numel()} is not batch*k*n = {nb}*{k}*{n}")
    tensors = tuple(t for t in (out, *ys, ahat, add) if t is not None)
    for t in tensors:
        _batch(t, n)   # device, dtype, contiguity
    py = (_vp * l)(*[y.data_ptr() for y in ys])
    return py, _ptr(add), nb, k, l, tensors


def mul_kl_shape(param_set, l: int) -> dict:
    """Launch shape of poly_mul_ntt_kl with l inputs (ntt_mul_kl_shape), as
    mul_k_shape."""
    v, w = _sz(), ctypes.c_int()
    _check(lib().ntt_mul_kl_shape(_ps(param_set), l, ctypes.byref(v), ctypes.byref(w)), "ntt_mul_kl_shape")
    return {"split_max": v.value, "waves": w.value}


def poly_scatter(out, pos, val, param_set, stream=None):
    """out[b, pos[b, j]] = val[b, j] mod q for j < h, every other coefficient 0
    (qTESLA's challenge c from its h positions and signs).  pos and val are
    [batch, h] with 1 <= h <= n, val < 2q; out is [batch, n], fully written.
    Entries with pos >= n are ignored; positions of one polynomial are
    distinct."""
    n = _n(param_set)
    nb = out.numel() // n
    if out.numel() != nb * n:
        raise ValueError(f"out: numel {out.numel()} is not a multiple of n={n}")
    h = pos.numel() // nb if nb else 1
    if pos.numel() != nb * h or (nb and not 1 <= h <= n):
        raise ValueError(f"pos: numel {pos.numel()} is not batch*h = {nb}*h with 1 <= h <= {n}")
    if val.numel() != pos.numel():
        raise ValueError(f"val: numel {val.numel()} is not pos.numel() = {pos.numel()}")
    for t in (out, pos, val):
        _batch(t, 1)   # device, dtype, contiguity
    _run("poly_scatter", (out, pos, val), stream, out.data_ptr(), pos.data_ptr(), val.data_ptr(), nb, h, _ps(param_set))
    return out


def _round_outputs(where: str, hi, norms, npoly: int, n: int, d: int):
    """poly_round's outputs, checked: hi int8/uint8 [npoly, n] or None, norms
    int32 [npoly, 2] or None, not both None.  Returns their two pointers."""
    if hi is None and norms is None:
        raise ValueError(f"{where}: neither hi nor norms given")
    if not 1 <= int(d) <= 30:
        raise ValueError(f"{where}: d = {d}, expected 1 .. 30")
    if hi is not None and _byte_batch(hi) != npoly * n:   # device, dtype, contiguity
        raise ValueError(f"hi: numel {hi.numel()} is not polynomials*n = {npoly}*{n}")
    if norms is not None and _batch(norms, 1) != npoly * 2:   # device, dtype, contiguity
        raise ValueError(f"norms: numel {norms.numel()} is not polynomials*2 = {npoly}*2")
    return _ptr(hi), _ptr(norms)


def poly_round(w, param_set, d: int, hi=None, norms=None, stream=None):
    """qTESLA's rounding and norm maxima of the polynomials w [batch, n]
    (entries < 2q; pass a [B, k, n] tensor as it is): with c the centred
    coefficient and c = hi * 2^d + lo, lo in (-2^(d-1), 2^(d-1)],

    hi     int8/uint8 [batch, n], the high parts (two's-complement bytes);
    norms  int32 [batch, 2], (max |c|, max |lo|) of each polynomial.

    Either may be None (not computed), not both.  d is the caller's constant
    (qTESLA: 22 / 22 / 24 for ref / p-I / p-III); with hi it must leave hi
    within a signed byte (NTTError otherwise).  Returns (hi, norms)."""
    n = _n(param_set)
    nb = _batch(w, n)
    ph, pn = _round_outputs("poly_round", hi, norms, nb, n, d)
    _run("poly_round", (w, hi, norms), stream, ph, pn, w.data_ptr(), nb, int(d), _ps(param_set))
    return hi, norms


def poly_mul_ntt_kl_round(ys, ahat, param_set, d: int, hi=None, norms=None, add=None, stream=None):
    """poly_round of poly_mul_ntt_kl(ys, ahat, add) in one launch, the product
    never stored (qTESLA's verification: the hash's input [w_i]_M straight
    from z and c; with one y and add = v, the signer's norms of
    w_i = v_i - e_i c).  ys, ahat and add as poly_mul_ntt_kl; hi is int8/uint8
    [batch, k, n], norms int32 [batch, k, 2], either may be None.  No output
    may overlap an input.  Returns (hi, norms)."""
    n = _n(param_set)
    py, pa, nb, k, l, ins = _rows_operands(n, ys, ahat, add)
    ph, pn = _round_outputs("poly_mul_ntt_kl_round", hi, norms, nb * k, n, d)
    _run("poly_mul_ntt_kl_round", (*ins, hi, norms), stream,
         ph, pn, py, ahat.data_ptr(), pa, nb, k, l, int(d), _ps(param_set))
    return hi, norms


def _keyed_operands(n: int, ys, ahat, keys, add, out=None):
    """The operands of the keyed products, checked: _rows_operands on key 0's
    block, then ahat's (nkeys, k, l, n) shape and keys, None or int32 [batch] on
    the same device.  Returns _rows_operands' tuple with keys' pointer or None
    and nkeys appended, keys among the tensors."""
    torch = _torch()
    ys = tuple(ys)
    if getattr(ahat, "dim", lambda: 0)() != 4:
        raise ValueError(f"ahat: shape {tuple(getattr(ahat, 'shape', ()))}, expected (nkeys, k, l, n)")
    nkeys = ahat.shape[0]
    if not 1 <= nkeys <= MUL_KEYS_MAX or tuple(ahat.shape[2:]) != (len(ys), n):
        raise ValueError(f"ahat: shape {tuple(ahat.shape)}, expected (nkeys >= 1, k, l = {len(ys)}, n = {n})")
    if not ahat.is_contiguous():
        raise ValueError("ahat: tensor must be contiguous ([nkeys][k][l][n])")
    if keys is not None:   # shapes before devices, as _rows_operands
        if keys.dtype != torch.int32:
            raise ValueError(f"keys: dtype {keys.dtype}, expected int32")
        if keys.dim() != 1 or not ys or keys.shape[0] != ys[0].numel() // n:
            raise ValueError(f"keys: shape {tuple(keys.shape)}, expected [batch]")
    py, pa, nb, k, l, tensors = _rows_operands(n, ys, ahat[0], add, out)
    if keys is not None:
        _batch(keys, 1)   # device, contiguity
    return py, pa, nb, k, l, (*tensors, keys), _ptr(keys), nkeys


def poly_mul_ntt_kl_keyed(out, ys, ahat, keys, param_set, add=None, stream=None):
    """poly_mul_ntt_kl over many keys in one launch: message b is multiplied
    by the rows of key min(keys[b], nkeys - 1), or of key min(b, nkeys - 1) with
    keys None (a key-generation batch's t_b = a_b s_b + e_b with one ys, one a
    per key).  ahat is a contiguous int32 (nkeys, k, l, n) tensor, key j's
    block what poly_mul_ntt_kl takes -- poly_gen_a over nkeys seeds writes all
    of it (l = 1), or slot 0 of every key with pstride = 2 n (l = 2); keys is an
    int32 [batch] tensor on the same device (read as unsigned: an index beyond
    the last key, a caller's bug, gives the last key's result) or None.  ys,
    add and out as poly_mul_ntt_kl.  Returns out."""
    py, pa, nb, k, l, tensors, pk, nkeys = _keyed_operands(_n(param_set), ys, ahat, keys, add, out)
    _run("poly_mul_ntt_kl_keyed", tensors, stream,
         out.data_ptr(), py, ahat.data_ptr(), pk, nkeys, pa, nb, k, l, _ps(param_set))
    return out


def poly_mul_ntt_kl_round_keyed(ys, ahat, keys, param_set, d: int, hi=None, norms=None, add=None, stream=None):
    """poly_mul_ntt_kl_round over many keys in one launch (a batch of
    signatures made under different public keys, verified together): ahat and
    keys as poly_mul_ntt_kl_keyed, everything else as poly_mul_ntt_kl_round.
    Returns (hi, norms)."""
    n = _n(param_set)
    py, pa, nb, k, l, ins, pk, nkeys = _keyed_operands(n, ys, ahat, keys, add)
    ph, pn = _round_outputs("poly_mul_ntt_kl_round_keyed", hi, norms, nb * k, n, d)
    _run("poly_mul_ntt_kl_round_keyed", (*ins, hi, norms), stream,
         ph, pn, py, ahat.data_ptr(), pk, nkeys, pa, nb, k, l, int(d), _ps(param_set))
    return hi, norms


def _byte_rows(name: str, t, batch: int) -> int:
    """Row length of a uint8/int8 device tensor [batch, ...]: a multiple of 8."""
    _byte_batch(t)   # device, dtype, contiguity
    if t.dim() < 2 or t.shape[0] != batch:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected [{batch}, bytes]")
    row = int(np.prod(t.shape[1:]))
    if row % 8:
        raise ValueError(f"{name}: {row} bytes per message, expected a multiple of 8")
    return row


def _xof_path(path) -> int:
    if path not in XOF_PATHS:
        raise ValueError(f"path {path!r}, expected one of {sorted(XOF_PATHS)}")
    return XOF_PATHS[path]


def _xof_algo(algo) -> int:
    if isinstance(algo, str) and algo not in XOF_ALGOS:
        raise ValueError(f"algo {algo!r}, expected one of {sorted(XOF_ALGOS)}")
    return XOF_ALGOS[algo] if isinstance(algo, str) else int(algo)


def _xof_cstm(cstm) -> int:
    c = -1 if cstm is None else int(cstm)
    if cstm is not None and not 0 <= c <= 0xFFFF:
        raise ValueError(f"cstm = {cstm}, expected None or 0 .. 65535")
    return c


def _seed_rows(seed, batch: int, shake256: bool = False) -> int:
    """Bytes per seed of seed [batch, seedlen]: a multiple of 8 within 8 .. 160,
    8 .. 128 for the samplers under SHAKE256."""
    seedlen = _byte_rows("seed", seed, batch)
    smax = 128 if shake256 else 160
    if seed.dim() != 2 or not 8 <= seedlen <= smax:
        raise ValueError(f"seed: shape {tuple(seed.shape)}, expected [{batch}, 8 .. {smax}]")
    return seedlen


def _nonce(nonce) -> int:
    if not 0 <= int(nonce) <= 255:
        raise ValueError(f"nonce = {nonce}, expected 0 .. 255")
    return int(nonce)


def _nonces(nonces, batch: int):
    """The per-message nonces, None or int32 [batch]: their pointer."""
    if nonces is not None and (_batch(nonces, 1) != batch or nonces.dim() != 1):
        raise ValueError(f"nonces: shape {tuple(nonces.shape)}, expected [{batch}]")
    return _ptr(nonces)


def _pstride(pstride, n: int) -> int:
    pstride = n if pstride is None else int(pstride)
    if pstride < n or pstride % 4:
        raise ValueError(f"pstride = {pstride}, expected a multiple of 4 and >= n = {n}")
    return pstride


def xof_small_batch_max(algo="shake256", ragged: bool = False) -> int:
    """Largest batch at which xof (ragged False) or xof_ragged (ragged True)
    with path="auto" runs the wave kernels, two messages per wave (0: never)."""
    v = _sz()
    _check(lib().ntt_xof_small_batch_max(_xof_algo(algo), int(bool(ragged)), ctypes.byref(v)), "ntt_xof_small_batch_max")
    return v.value


def xof(out, in0, in1=None, algo="shake256", cstm=None, stream=None, path="auto"):
    """out[b] = XOF(in0[b] || in1[b]) for every b, one launch: SHAKE128 /
    SHAKE256 (cstm None) or qTESLA's cshake128_simple / cshake256_simple with
    the 16-bit customization cstm (qTESLA's H, G and the expansions).

    out, in0 and in1 are int8/uint8 device tensors whose first dimension is
    the batch ([batch, k, n] hi bytes are taken as they are); in1 may be None
    (one segment).  Bytes per message: multiples of 8, out's within
    8 .. 512.  The two segments are read where they lie; out overlaps
    neither.  path: "auto" (two messages per wave up to xof_small_batch_max,
    one message per lane above), "lane" or "wave" -- the same bytes on each.
    Returns out."""
    pth = _xof_path(path)
    if out.dim() < 2:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected [batch, bytes]")
    nb = out.shape[0]
    outlen = _byte_rows("out", out, nb)
    if not 8 <= outlen <= XOF_OUT_MAX:
        raise ValueError(f"out: {outlen} bytes per message, expected 8 .. {XOF_OUT_MAX}")
    len0 = _byte_rows("in0", in0, nb)
    len1 = 0 if in1 is None else _byte_rows("in1", in1, nb)
    if len0 + len1 >= 1 << 32:
        raise ValueError("message of 2^32 bytes or more")
    a, c = _xof_algo(algo), _xof_cstm(cstm)
    p0 = in0.data_ptr() if len0 else None
    p1 = in1.data_ptr() if len1 else None
    _run("ntt_xof_path", (out, in0, in1), stream, out.data_ptr(), outlen, p0, len0, p1, len1, nb, a, c, pth)
    return out


def xof_ragged(out, msg, off, algo="shake256", cstm=None, stream=None, path="auto"):
    """out[b] = XOF(msg[off[b] : off[b + 1]]) for every b, one launch: xof's
    hash over messages of any byte length, back to back in msg (qTESLA's
    G(m) from the messages as they arrive).

    out is [batch, outlen] int8/uint8 (outlen a multiple of 8 within 8 .. 512);
    msg a contiguous 1-D int8/uint8 device tensor whose numel is a multiple of
    8 (the caller pads the buffer: the kernel reads aligned 8-byte words); off a
    contiguous int64 device tensor of batch + 1 byte offsets, its bits taken as
    uint64.  Offsets are clamped to the buffer and to each other as
    ntt_xof_ragged defines (qtesla_ntt.h); a well-formed table is non-decreasing
    and ends at or below msg.numel().  path as xof's, with
    xof_small_batch_max(algo, ragged=True).  Dtypes and shapes are checked
    before the devices.  Returns out."""
    torch = _torch()
    for name, t in (("out", out), ("msg", msg)):
        if t.dtype not in _BYTE_DTYPES:
            raise TypeError(f"{name}: expected int8/uint8 storage, got {t.dtype}")
    if off.dtype != torch.int64:
        raise TypeError(f"off: expected int64 storage (the offsets' uint64 bits), got {off.dtype}")
    if out.dim() != 2:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected [batch, bytes]")
    nb, outlen = out.shape
    if outlen % 8 or not 8 <= outlen <= XOF_OUT_MAX:
        raise ValueError(f"out: {outlen} bytes per message, expected a multiple of 8 within 8 .. {XOF_OUT_MAX}")
    if msg.dim() != 1:
        raise ValueError(f"msg: shape {tuple(msg.shape)}, expected one dimension (all messages back to back)")
    msg_bytes = msg.numel()
    if msg_bytes % 8:
        raise ValueError(f"msg: {msg_bytes} bytes, expected a multiple of 8: pad the buffer to whole 8-byte words "
                         "(the pad bytes belong to no message)")
    if off.dim() != 1 or off.numel() != nb + 1:
        raise ValueError(f"off: shape {tuple(off.shape)}, expected [{nb + 1}] (batch + 1 offsets)")
    for name, t in (("out", out), ("msg", msg), ("off", off)):
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
    a, c = _xof_algo(algo), _xof_cstm(cstm)
    pm = msg.data_ptr() if msg_bytes else None
    _run("ntt_xof_ragged_path", (out, msg, off), stream,
         out.data_ptr(), outlen, pm, msg_bytes, off.data_ptr(), nb, a, c, _xof_path(path))
    return out


def ragged_pack(messages, device):
    """A list of bytes to xof_ragged's (msg, off) on `device`: the messages back
    to back, zero-padded to a multiple of 8 bytes, and their batch + 1 offsets.
    A host helper for tests and small callers (one copy per call)."""
    torch = _torch()
    off = np.zeros(len(messages) + 1, dtype=np.int64)
    np.cumsum(np.array([len(m) for m in messages], dtype=np.int64), out=off[1:])
    data = b"".join(messages)
    buf = np.frombuffer(data + bytes(-len(data) % 8), dtype=np.uint8).copy()
    return torch.from_numpy(buf).to(device), torch.from_numpy(off).to(device)


def poly_challenge(pos, val, seed, param_set, stream=None):
    """qTESLA's Enc(c'): seed [batch, seedlen] int8/uint8 (seedlen a multiple
    of 8 within 8 .. 160) to the challenge's h positions and signs, pos and
    val int32 [batch, h] with 1 <= h <= 128 -- the lists poly_scatter takes
    (val is 1 or q - 1).  Returns (pos, val)."""
    _n(param_set)   # the parameter set exists
    if pos.dim() != 2 or tuple(val.shape) != tuple(pos.shape):
        raise ValueError(f"pos / val: shapes {tuple(pos.shape)} / {tuple(val.shape)}, expected two equal [batch, h]")
    nb, h = pos.shape
    for t in (pos, val):
        _batch(t, 1)   # device, dtype, contiguity
    if not 1 <= h <= CHALLENGE_H_MAX:
        raise ValueError(f"h = {h}, expected 1 .. {CHALLENGE_H_MAX}")
    seedlen = _seed_rows(seed, nb)
    _run("poly_challenge", (pos, val, seed), stream,
         pos.data_ptr(), val.data_ptr(), seed.data_ptr(), seedlen, nb, h, _ps(param_set))
    return pos, val


def poly_sample_y(y, seed, param_set, bits: int, algo="shake256", nonce: int = 0, nonces=None, stream=None):
    """qTESLA's sample_y: seed [batch, seedlen] int8/uint8 (seedlen a multiple
    of 8 within 8 .. 160 for SHAKE128, 8 .. 128 for SHAKE256) to the masking
    polynomials y, int32 [batch, n] (or flat), canonical in [0, q) and centred
    in [-B, B], B = 2^(bits-1) - 1 with 2 <= bits <= 24 (qTESLA: 20 for p-I,
    22 for p-III).  Message b is drawn at nonce (nonces[b] + nonce) & 0xFF:
    nonce a scalar 0 .. 255, nonces None or an int32 [batch] device tensor of
    per-message attempt counters.  Returns y."""
    nb = _batch(y, _n(param_set))
    if y.dim() > 1 and y.shape[0] != nb:
        raise ValueError(f"y: shape {tuple(y.shape)}, expected [{nb}, n] or flat")
    if not 2 <= int(bits) <= 24:
        raise ValueError(f"bits = {bits}, expected 2 .. 24")
    nonce, a = _nonce(nonce), _xof_algo(algo)
    seedlen = _seed_rows(seed, nb, a == XOF_ALGOS["shake256"])
    _run("poly_sample_y", (y, seed, nonces), stream,
         y.data_ptr(), seed.data_ptr(), seedlen, _nonces(nonces, nb), nonce, nb, int(bits), a, _ps(param_set))
    return y


def poly_gen_a(a, seed, param_set, nblocks: int, k: int, pstride=None, stream=None):
    """qTESLA's GenA: seed [batch, seedlen] int8/uint8 (seedlen a multiple of 8
    within 8 .. 160; qTESLA: seed_a's 32 bytes) to the k public polynomials of
    each key, canonical in [0, q) and already in the NTT domain: what
    poly_mul_ntt_k / _kl / _kl_round take as ahat.  a is an int32 contiguous
    device tensor of batch*k*pstride elements; polynomial i of key b starts at
    element (b*k + i)*pstride and the pstride - n elements after it are not
    written.  pstride defaults to n (dense [batch, k, n]); pstride = 2n fills
    slot 0 of [k, 2, n] verification rows in place.  nblocks is qTESLA's
    PARAM_GEN_A (108 for p-I, 180 for p-III), 1 .. 256.  Every parameter set
    but "ref".  Returns a."""
    n = _n(param_set)
    _batch(a, 1)   # device, dtype, contiguity
    if not 1 <= int(k) <= MUL_K_MAX:
        raise ValueError(f"k = {k}, expected 1 .. {MUL_K_MAX}")
    if not 1 <= int(nblocks) <= GEN_A_BLOCKS_MAX:
        raise ValueError(f"nblocks = {nblocks}, expected 1 .. {GEN_A_BLOCKS_MAX}")
    pstride = _pstride(pstride, n)
    if seed.dim() != 2:   # the batch is the seeds': their shape first, worded without it
        raise ValueError(f"seed: shape {tuple(seed.shape)}, expected [batch, 8 .. 160]")
    nb = seed.shape[0]
    seedlen = _seed_rows(seed, nb)
    if a.numel() != nb * int(k) * pstride:
        raise ValueError(f"a: numel {a.numel()} is not batch*k*pstride = {nb}*{k}*{pstride}")
    _run("poly_gen_a", (a, seed), stream,
         a.data_ptr(), pstride, seed.data_ptr(), seedlen, nb, int(k), int(nblocks), _ps(param_set))
    return a


def poly_sample_gauss(out, seed, cdt, param_set, algo="shake256", nonce: int = 0, nonces=None, stream=None):
    """qTESLA's CDT Gaussian sampler: seed [batch, seedlen] int8/uint8 (seedlen a
    multiple of 8 within 8 .. 160 for SHAKE128, 8 .. 128 for SHAKE256), one
    seed per polynomial, to the secret polynomials out, int32 [batch, n] (or
    flat), canonical in [0, q).  cdt is the caller's cumulative table, an int32
    device tensor [rows, cols] with 1 <= rows <= 128 and 1 <= cols <= 4, most
    significant 31-bit limb first; a coefficient is +-#{rows <= the sample}.
    Polynomial b is drawn at nonce (nonces[b] + nonce) & 0xFF: nonce a scalar
    0 .. 255, nonces None or an int32 [batch] device tensor of per-polynomial
    restart counters.  Returns out."""
    nb = _batch(out, _n(param_set))
    if out.dim() > 1 and out.shape[0] != nb:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected [{nb}, n] or flat")
    _batch(cdt, 1)   # device, dtype, contiguity
    if cdt.dim() != 2 or not 1 <= cdt.shape[0] <= GAUSS_ROWS_MAX or not 1 <= cdt.shape[1] <= GAUSS_COLS_MAX:
        raise ValueError(f"cdt: shape {tuple(cdt.shape)}, expected [1 .. {GAUSS_ROWS_MAX}, 1 .. {GAUSS_COLS_MAX}]")
    rows, cols = cdt.shape
    nonce, a = _nonce(nonce), _xof_algo(algo)
    seedlen = _seed_rows(seed, nb, a == XOF_ALGOS["shake256"])
    _run("poly_sample_gauss", (out, seed, cdt, nonces), stream, out.data_ptr(), seed.data_ptr(), seedlen,
         _nonces(nonces, nb), nonce, cdt.data_ptr(), rows, cols, nb, a, _ps(param_set))
    return out


def poly_hsum(sums, w, param_set, h: int, stream=None):
    """qTESLA's check_ES: sums[b] = the sum of the h largest |c| of polynomial
    b of w, int32 [batch, n] (or flat; entries < 2q, c the centred value as in
    poly_round), equal values counted as often as they occur.  sums is an
    int64 device tensor of batch elements; 1 <= h <= n.  Returns sums."""
    torch = _torch()
    n = _n(param_set)
    nb = _batch(w, n)
    if _batch(sums, 1, (torch.int64,), "int64") != nb:
        raise ValueError(f"sums: numel {sums.numel()} is not the batch {nb}")
    if not 1 <= int(h) <= n:
        raise ValueError(f"h = {h}, expected 1 .. {n}")
    _run("poly_hsum", (sums, w), stream, sums.data_ptr(), w.data_ptr(), nb, int(h), _ps(param_set))
    return sums


def _pack_operands(rows, w, param_set, bits, signed, maxima=None):
    """The operands of poly_pack / poly_unpack, checked: batch, stride, k, sgn
    and the tensors given, for _run.  rows is int8/uint8 [batch, stride], w
    int32 [batch, k, n] or [batch, n], maxima None or int32 with batch*k
    elements."""
    n, nb, stride = _packed_rows("rows", rows, param_set)
    _batch(w, n)
    if w.dim() < 2 or w.shape[0] != nb:
        raise ValueError(f"w: shape {tuple(w.shape)}, expected [{nb}, k, {n}] or [{nb}, {n}]")
    k = w.numel() // (nb * n) if nb else 1
    if w.numel() != nb * k * n or not 1 <= k <= MUL_K_MAX:
        raise ValueError(f"w: numel {w.numel()} is not batch*k*n = {nb}*k*{n} with 1 <= k <= {MUL_K_MAX}")
    sgn = _packed_fields("rows", stride, k, bits, signed, param_set)
    _maxima(maxima, nb, k)
    return nb, stride, k, sgn, (rows, w, maxima)


def _packed_rows(name: str, rows, param_set):
    """The packed side of poly_pack / poly_unpack / poly_unpack_ntt, int8/uint8
    [batch, stride]: n, batch and stride."""
    n = _n(param_set)
    _byte_batch(rows)   # device, dtype, contiguity
    if rows.dim() != 2:
        raise ValueError(f"{name}: shape {tuple(rows.shape)}, expected [batch, stride]")
    return (n, *rows.shape)


def _packed_fields(name: str, stride: int, k: int, bits, signed, param_set) -> int:
    """The field geometry of the packed rows `name`, checked: bits against q's
    bit length, stride against the k*n*bits/8 bytes of a row.  Returns sgn."""
    info = param_info(param_set)
    n, qbits = info["n"], info["q"].bit_length()
    sgn = 1 if signed else 0
    if not 8 <= int(bits) <= qbits - sgn:
        raise ValueError(f"bits = {bits}, expected 8 .. {qbits - sgn} ({'signed' if sgn else 'unsigned'})")
    packed = k * n * int(bits) // 8
    if stride % 16 or stride < packed:
        raise ValueError(f"{name}: stride {stride}, expected a multiple of 16 and >= k*n*bits/8 = {packed}")
    return sgn


def _maxima(maxima, nb: int, k: int):
    """poly_unpack's maxima: None or int32 with one element per polynomial."""
    if maxima is not None and _batch(maxima, 1) != nb * k:
        raise ValueError(f"maxima: numel {maxima.numel()} is not batch*k = {nb}*{k}")


def poly_pack(out, w, param_set, bits: int, signed=True, stream=None):
    """qTESLA's wire format: the coefficients w, int32 [batch, k, n] (or
    [batch, n] for k = 1; entries < 2q), as fields of `bits` bits in the rows
    out, int8/uint8 [batch, stride] with stride a multiple of 16 and
    >= k*n*bits/8.  signed: the centred value's two's-complement low bits (a
    signature's z: bits = 20 for p-I, 22 for p-III); unsigned: the canonical
    value's low bits (a public key's t: bits = 29 / 30).  A value outside the
    field's range is truncated.  Bytes of a row beyond k*n*bits/8 are not
    written.  8 <= bits <= bit length of q, less one when signed.  Returns out."""
    nb, stride, k, sgn, tensors = _pack_operands(out, w, param_set, bits, signed)
    _run("poly_pack", tensors, stream, out.data_ptr(), stride, w.data_ptr(), nb, k, int(bits), sgn, _ps(param_set))
    return out


def poly_unpack(w, inp, param_set, bits: int, signed=True, maxima=None, stream=None):
    """poly_pack's inverse: the rows inp, int8/uint8 [batch, stride], to
    canonical coefficients w, int32 [batch, k, n] (or [batch, n]).  maxima,
    None or int32 with batch*k elements, receives per polynomial max |s| of
    the sign-extended fields (signed) or the largest raw field (unsigned: a
    maximum >= q is a malformed key).  Bytes of a row beyond k*n*bits/8 are not
    read.  Returns (w, maxima)."""
    nb, stride, k, sgn, tensors = _pack_operands(inp, w, param_set, bits, signed, maxima)
    _run("poly_unpack", tensors, stream,
         w.data_ptr(), _ptr(maxima), inp.data_ptr(), stride, nb, k, int(bits), sgn, _ps(param_set))
    return w, maxima


def poly_unpack_ntt(out, inp, param_set, bits: int, k: int, signed=False, negate=False, pstride=None, maxima=None,
                    stream=None):
    """poly_unpack, poly_ntt and (negate) the entrywise negation mod q in one
    launch: the rows inp, int8/uint8 [batch, stride] with k polynomials of
    n*bits/8 bytes each, to canonical NTT-domain polynomials in natural order.
    out is a flat (or any contiguous) int32 device tensor; polynomial i of row
    b starts at element (b*k + i)*pstride and the pstride - n elements after it
    are not written.  out has batch*k*pstride elements, or ends with its last
    polynomial: (batch*k - 1)*pstride + n elements, which is what a view from
    an offset into a larger buffer has.  pstride defaults to n (dense
    [batch, k, n]); pstride = 2n with out = rows.view(-1)[n:] fills slot 1 of
    [batch, k, 2, n] verification rows in place, beside poly_gen_a's slot 0
    (negate=True: q - t-hat).  maxima is poly_unpack's: None or int32 with
    batch*k elements.  Parameter sets "ref", "p-I", "p-III".  Returns
    (out, maxima)."""
    n, nb, stride = _packed_rows("inp", inp, param_set)
    _batch(out, 1)
    if not 1 <= int(k) <= MUL_K_MAX:
        raise ValueError(f"k = {k}, expected 1 .. {MUL_K_MAX}")
    k = int(k)
    sgn = _packed_fields("inp", stride, k, bits, signed, param_set)
    pstride = _pstride(pstride, n)
    if nb and out.numel() not in (nb * k * pstride, (nb * k - 1) * pstride + n):
        raise ValueError(f"out: numel {out.numel()} is neither batch*k*pstride = {nb}*{k}*{pstride} "
                         f"nor (batch*k - 1)*pstride + n")
    _maxima(maxima, nb, k)
    _run("poly_unpack_ntt", (out, inp, maxima), stream, out.data_ptr(), pstride, _ptr(maxima), inp.data_ptr(), stride,
         nb, k, int(bits), sgn, 1 if negate else 0, _ps(param_set))
    return out, maxima


def _words(name: str, t, numel=None):
    """A contiguous 1-D int32/uint32 tensor (of `numel` elements): flags, index lists, counts."""
    _torch()
    if t.dtype not in _INT_DTYPES:
        raise TypeError(f"{name}: expected int32/uint32 storage, got {t.dtype}")
    if t.dim() != 1 or (numel is not None and t.numel() != numel):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected [{'.' if numel is None else numel}]")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def _strided_rows(name: str, t):
    """(rows, row bytes, stride in bytes) of a tensor [rows, ...] whose rows are
    contiguous in themselves and lie a fixed, non-negative distance apart: a
    contiguous tensor, or a view of some columns of one (sig[:, zlen:])."""
    if t.dim() < 1:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected [rows, ...]")
    inner = 1   # elements per row
    for size, st in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and st != inner:
            raise ValueError(f"{name}: strides {t.stride()}: a row must be contiguous in itself")
        inner *= size
    item = t.element_size()
    row_bytes = inner * item
    if row_bytes % 4 or row_bytes < 4:
        raise ValueError(f"{name}: {row_bytes} bytes per row, expected a multiple of 4, at least 4")
    stride = t.stride(0) * item if t.shape[0] > 1 else row_bytes
    if stride % 4 or stride < row_bytes:
        raise ValueError(f"{name}: rows {stride} bytes apart, expected a multiple of 4, at least the row's {row_bytes}")
    return t.shape[0], row_bytes, stride


def rows_over(flag, vals, bounds, accumulate=False, stream=None):
    """flag[b] = any(vals[b][j] > bounds[j]), or flag[b] | that with accumulate
    (ntt_rows_over).  vals is a contiguous [batch, ...] device tensor of int32 /
    uint32 (poly_round's norms, poly_unpack's maxima) or int64 (poly_hsum's
    sums), its bits taken as unsigned, with m = 1 .. 16 values per row; bounds a
    sequence of m Python ints in 0 .. 2^64 - 1 -- one at or above the type's
    maximum never flags, which skips its column; flag int32 [batch].  Returns
    flag."""
    torch = _torch()
    if vals.dtype in _INT_DTYPES:
        width = 32
    elif vals.dtype in (torch.int64, getattr(torch, "uint64", torch.int64)):
        width = 64
    else:
        raise TypeError(f"vals: expected int32/uint32 or int64 storage, got {vals.dtype}")
    if vals.dim() < 1 or not vals.is_contiguous():
        raise ValueError(f"vals: shape {tuple(vals.shape)}, expected a contiguous [batch, ...]")
    nb = vals.shape[0]
    _words("flag", flag, nb)
    bounds = [int(x) for x in bounds]
    m = len(bounds)
    if not 1 <= m <= ROWS_M_MAX:
        raise ValueError(f"{m} bounds, expected 1 .. {ROWS_M_MAX}")
    if vals.numel() != nb * m:
        raise ValueError(f"vals: shape {tuple(vals.shape)} with {m} bounds, expected {m} values per row")
    if any(not 0 <= x < 1 << 64 for x in bounds):
        raise ValueError("bounds: expected 0 .. 2^64 - 1")
    arr = (ctypes.c_uint64 * m)(*bounds)
    _run("ntt_rows_over", (flag, vals), stream,
         flag.data_ptr(), vals.data_ptr(), width, m, arr, 1 if accumulate else 0, nb)
    return flag


def rows_differ(flag, a, b, accumulate=False, stream=None):
    """flag[r] = 1 iff rows a[r] and b[r] differ in any byte, or flag[r] | that
    with accumulate (ntt_rows_differ).  a and b are [batch, ...] device tensors
    of equal bytes per row (a multiple of 4), each contiguous or a view of some
    columns of a contiguous tensor, read where it lies (c' as sig[:, zlen:]);
    flag int32 [batch].  Returns flag."""
    na, row_bytes, sa = _strided_rows("a", a)
    nb, row_b, sb = _strided_rows("b", b)
    if na != nb or row_bytes != row_b:
        raise ValueError(f"a / b: {na} rows of {row_bytes} bytes and {nb} rows of {row_b} bytes")
    _words("flag", flag, nb)
    _run("ntt_rows_differ", (flag, a, b), stream,
         flag.data_ptr(), a.data_ptr(), sa, b.data_ptr(), sb, row_bytes, 1 if accumulate else 0, nb)
    return flag


def select(idx, count, flag, want, bump=None, stream=None):
    """idx[:c] = the b with (flag[b] != 0) == want, ascending, and count[0] = c
    (ntt_select); idx[c:] keeps what it held.  bump, int32 [batch] or None, is
    raised by one at exactly the selected b.  idx and flag are int32 [batch],
    count int32 [1]; want is False / True.  An empty batch writes nothing,
    count included.  Returns (idx, count)."""
    nb = _words("flag", flag).numel()
    _words("idx", idx, nb)
    _words("count", count, 1)
    if want not in (0, 1, False, True):
        raise ValueError(f"want = {want!r}, expected False / True")
    if bump is not None:
        _words("bump", bump, nb)
    _run("ntt_select", (idx, count, flag, bump), stream,
         idx.data_ptr(), count.data_ptr(), flag.data_ptr(), int(want), _ptr(bump), nb)
    return idx, count


def rows_move(dst, src, dst_idx=None, src_idx=None, count=None, n=None, stream=None):
    """dst[dst_idx[i]] = src[src_idx[i]] for i < min(n, count[0]), whole rows
    (ntt_rows_move).  dst and src are [rows, ...] device tensors of equal bytes
    per row (a multiple of 4; the dtypes need not match), each contiguous or a
    view of some columns of a contiguous tensor; a 1-D tensor has one element
    per row.  dst_idx / src_idx are int32 index lists or None (the identity);
    an index at or past its side's rows skips the row.  count is an int32 [1]
    device tensor or None; n, the host's count that sizes the launch, defaults
    to the index lists' length, or without lists to the smaller side's rows.
    Returns dst."""
    dr, row_bytes, ds = _strided_rows("dst", dst)
    sr, row_s, ss = _strided_rows("src", src)
    if row_bytes != row_s:
        raise ValueError(f"dst / src: rows of {row_bytes} and of {row_s} bytes")
    lists = [(nm, _words(nm, t)) for nm, t in (("dst_idx", dst_idx), ("src_idx", src_idx)) if t is not None]
    if n is None:
        n = min(t.numel() for _, t in lists) if lists else min(dr, sr)
    n = int(n)
    if n < 0 or any(t.numel() < n for _, t in lists):
        raise ValueError(f"n = {n} with index lists of {[t.numel() for _, t in lists]} entries")
    if count is not None:
        _words("count", count, 1)
    _run("ntt_rows_move", (dst, src, dst_idx, src_idx, count), stream, dst.data_ptr(), ds, _ptr(dst_idx), dr,
         src.data_ptr(), ss, _ptr(src_idx), sr, row_bytes, _ptr(count), n)
    return dst


def poly_mul_nussbaumer(c, a, b, param_set, ring="q", stream=None):
    """c = a*b mod x^n + 1 by the Nussbaumer algorithm (nussbaumer_fft, NTT.cu:167-277).

    ring "q": mod param_set's q (equals poly_mul); ring "m32": mod 2^32 - 1,
    the reference's ring.  Buffers must be 16-byte aligned."""
    r = RINGS[ring] if isinstance(ring, str) else int(ring)
    return _mul("poly_mul_nussbaumer", c, a, b, param_set, stream, r)


def poly_pointwise(c, a, b, param_set, stream=None):
    return _mul("poly_pointwise", c, a, b, param_set, stream)


def fill_uniform(t, param_set, seed: int, first_poly: int = 0, stream=None):
    """Device-side counter-based uniform coefficients in [0, q)."""
    n = _n(param_set)
    b = _batch(t, n)
    _run("ntt_fill_uniform", (t,), stream, t.data_ptr(), b, _ps(param_set), seed & (2**64 - 1), first_poly)
    return t


def to_numpy_u32(t) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint32)


def from_numpy_u32(a: np.ndarray, device="cuda"):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(device)


# ------------------------------------------------------- host-buffer API
# Host -> host operation pipelined over HIP streams (include/qtesla_ntt.h,
# "host-buffer (streamed) operation"; the reference's PCIe-inclusive driver
# body NTT.cu:2384-2428).  Arrays are numpy uint32, C-contiguous [batch, n].

class HostContext:
    """Owns the device / pinned staging buffers of ntt_host_ctx_create."""

    def __init__(self, param_set, chunk_polys: int = 0, nslots: int = 0):
        self.param_set = param_set
        self.n = _n(param_set)
        h = _vp()
        _check(lib().ntt_host_ctx_create(ctypes.byref(h), _ps(param_set), chunk_polys, nslots),
               "ntt_host_ctx_create")
        self._h = h

    def close(self):
        if self._h is not None and self._h.value:
            _check(lib().ntt_host_ctx_destroy(self._h), "ntt_host_ctx_destroy")
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _arr(self, x, name):
        if not isinstance(x, np.ndarray) or x.dtype != np.uint32 or not x.flags["C_CONTIGUOUS"]:
            raise TypeError(f"{name}: expected a C-contiguous numpy uint32 array")
        if x.size % self.n:
            raise ValueError(f"{name}: size {x.size} is not a multiple of n={self.n}")
        return x.size // self.n

    def _oop(self, name, out, inp):
        b = self._arr(inp, "inp")
        if self._arr(out, "out") != b:
            raise ValueError("out/in batch mismatch")
        _check(_FN[name](self._h, out.ctypes.data, inp.ctypes.data, b), name)
        return out

    def ntt(self, out, inp):
        return self._oop("poly_ntt_host", out, inp)

    def invntt(self, out, inp):
        return self._oop("poly_invntt_host", out, inp)

    def mul(self, c, a, b):
        nb = self._arr(a, "a")
        if self._arr(b, "b") != nb or self._arr(c, "c") != nb:
            raise ValueError("batch mismatch")
        _check(lib().poly_mul_host(self._h, c.ctypes.data, a.ctypes.data, b.ctypes.data, nb), "poly_mul_host")
        return c


def host_empty(count: int) -> np.ndarray:
    """A numpy uint32 array of `count` words in pinned host memory (ntt_host_alloc).

    The memory is freed when the last array viewing it is garbage-collected
    (the ctypes buffer below is the numpy base of every view)."""
    words = max(int(count), 1)
    ptr = lib().ntt_host_alloc(words * 4)
    if not ptr:
        raise MemoryError("ntt_host_alloc failed")

    def _free(self):
        if getattr(self, "_ptr", None):
            lib().ntt_host_free(self._ptr)
            self._ptr = None

    buf_t = type("PinnedU32", (ctypes.c_uint32 * words,), {"__del__": _free})
    buf = buf_t.from_address(ptr)
    buf._ptr = ptr
    return np.frombuffer(buf, dtype=np.uint32, count=int(count))
