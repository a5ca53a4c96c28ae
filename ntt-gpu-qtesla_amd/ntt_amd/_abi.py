"""The C ABI of include/qtesla_ntt.h as this package binds it: the library's
path, the header's constants, one ctypes signature per prototype and lib(),
which loads the library and applies them.

The header is the specification and this file the binding; nothing here reads
the header.  tests/test_binding_table.py compares the two, every prototype and
every integer #define.
"""
from __future__ import annotations

import ctypes
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("NTT_AMD_LIB") or os.path.join(ROOT_DIR, "lib", "libqtesla_ntt.so")
HEADER_PATH = os.path.join(os.path.dirname(ROOT_DIR), "include", "qtesla_ntt.h")

# ------------------------------------------------------------- constants
# NTT_<name> of the header, each under the same name less the prefix or as
# the value of a dictionary's key.

NTT_OK = 0
NTT_ERR_PARAM, NTT_ERR_NULL, NTT_ERR_ALIGN, NTT_ERR_HIP, NTT_ERR_SIZE, NTT_ERR_ALIAS = -1, -2, -3, -4, -5, -6

PARAM_SETS = {"ref": 0, "p-I": 1, "p-III": 2, "p-III-4096": 3, "p-III-8192": 4}   # NTT_PARAM_REF .. NTT_PARAM_N8192
RINGS = {"q": 0, "m32": 1}   # NTT_RING_*
# entry points of the small-batch switch (NTT_OP_*)
SWITCH_OPS = {"fwd": 0, "inv": 1, "fwd_br": 2, "inv_br": 3, "mul": 4, "mul_ntt": 5, "fwd_oop": 6, "inv_oop": 7}
XOF_ALGOS = {"shake128": 0, "shake256": 1}   # NTT_XOF_SHAKE*
XOF_PATHS = {"auto": 0, "lane": 1, "wave": 2}   # NTT_XOF_PATH_*
XOF_PATH_AUTO, XOF_PATH_LANE, XOF_PATH_WAVE = 0, 1, 2

MUL_K_MAX = 8
MUL_L_MAX = 2
MUL_KEYS_MAX = 2**31 - 1
XOF_OUT_MAX = 512
CHALLENGE_H_MAX = 128
SAMPLE_Y_REFILLS_MAX = 255
GEN_A_BLOCKS_MAX = 256
GAUSS_CHUNK = 512
GAUSS_ROWS_MAX = 128
GAUSS_COLS_MAX = 4
ROWS_M_MAX = 16

# ------------------------------------------------------------ signatures
# Device and host pointers are c_void_p (the callers pass data_ptr() ints or
# None); the pointers ctypes fills or reads on the host are typed.

_int, _sz, _vp = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
_u32, _u64 = ctypes.c_uint32, ctypes.c_uint64
_u32p, _u64p = ctypes.POINTER(_u32), ctypes.POINTER(_u64)
_intp, _szp, _vpp = ctypes.POINTER(_int), ctypes.POINTER(_sz), ctypes.POINTER(_vp)

SIGNATURES = {
    "ntt_param_info": (_int, (_int,) + (_u32p,) * 6),
    "ntt_get_tables": (_int, (_int,) + (_u32p,) * 5),
    # out, in (the in-place pair: NULL), batch, param_set, stream
    **dict.fromkeys(("poly_ntt", "poly_invntt", "poly_ntt_oop", "poly_invntt_oop", "poly_ntt_bitrev", "poly_invntt_bitrev",
                     "poly_bitrev_copy"), (_int, (_vp, _vp, _sz, _int, _vp))),
    # c, a, b, batch, param_set, stream
    **dict.fromkeys(("poly_mul", "poly_mul_ntt", "poly_pointwise"), (_int, (_vp, _vp, _vp, _sz, _int, _vp))),
    "poly_mul_nussbaumer": (_int, (_vp, _vp, _vp, _sz, _int, _int, _vp)),
    "poly_mul_ntt_k": (_int, (_vp, _vp, _vp, _vp, _sz, _int, _int, _vp)),
    "ntt_mul_k_shape": (_int, (_int, _szp, _intp)),
    "poly_mul_ntt_kl": (_int, (_vp, _vpp, _vp, _vp, _sz, _int, _int, _int, _vp)),
    "ntt_mul_kl_shape": (_int, (_int, _int, _szp, _intp)),
    "poly_scatter": (_int, (_vp, _vp, _vp, _sz, _int, _int, _vp)),
    "poly_round": (_int, (_vp, _vp, _vp, _sz, _int, _int, _vp)),
    "poly_mul_ntt_kl_round": (_int, (_vp, _vp, _vpp, _vp, _vp, _sz, _int, _int, _int, _int, _vp)),
    "poly_mul_ntt_kl_keyed": (_int, (_vp, _vpp, _vp, _vp, _sz, _vp, _sz, _int, _int, _int, _vp)),
    "poly_mul_ntt_kl_round_keyed": (_int, (_vp, _vp, _vpp, _vp, _vp, _sz, _vp, _sz, _int, _int, _int, _int, _vp)),
    "ntt_xof": (_int, (_vp, _sz, _vp, _sz, _vp, _sz, _sz, _int, _int, _vp)),
    "ntt_xof_path": (_int, (_vp, _sz, _vp, _sz, _vp, _sz, _sz, _int, _int, _int, _vp)),
    "ntt_xof_small_batch_max": (_int, (_int, _int, _szp)),
    "ntt_xof_ragged": (_int, (_vp, _sz, _vp, _sz, _vp, _sz, _int, _int, _vp)),
    "ntt_xof_ragged_path": (_int, (_vp, _sz, _vp, _sz, _vp, _sz, _int, _int, _int, _vp)),
    "poly_challenge": (_int, (_vp, _vp, _vp, _sz, _sz, _int, _int, _vp)),
    "poly_sample_y": (_int, (_vp, _vp, _sz, _vp, _u32, _sz, _int, _int, _int, _vp)),
    "poly_gen_a": (_int, (_vp, _sz, _vp, _sz, _sz, _int, _int, _int, _vp)),
    "poly_sample_gauss": (_int, (_vp, _vp, _sz, _vp, _u32, _vp, _int, _int, _sz, _int, _int, _vp)),
    "poly_hsum": (_int, (_vp, _vp, _sz, _int, _int, _vp)),
    "poly_pack": (_int, (_vp, _sz, _vp, _sz, _int, _int, _int, _int, _vp)),
    "poly_unpack": (_int, (_vp, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _vp)),
    "poly_unpack_ntt": (_int, (_vp, _sz, _vp, _vp, _sz, _sz, _int, _int, _int, _int, _int, _vp)),
    "ntt_rows_over": (_int, (_vp, _vp, _int, _int, _u64p, _int, _sz, _vp)),
    "ntt_rows_differ": (_int, (_vp, _vp, _sz, _vp, _sz, _sz, _int, _sz, _vp)),
    "ntt_select": (_int, (_vp, _vp, _vp, _int, _vp, _sz, _vp)),
    "ntt_rows_move": (_int, (_vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp)),
    "ntt_fill_uniform": (_int, (_vp, _sz, _int, _u64, _u64, _vp)),
    "ntt_host_ctx_create": (_int, (_vpp, _int, _sz, _int)),
    "ntt_host_ctx_destroy": (_int, (_vp,)),
    **dict.fromkeys(("poly_ntt_host", "poly_invntt_host"), (_int, (_vp, _vp, _vp, _sz))),
    "poly_mul_host": (_int, (_vp, _vp, _vp, _vp, _sz)),
    "ntt_host_alloc": (_vp, (_sz,)),
    "ntt_host_free": (None, (_vp,)),
    "ntt_last_hip_error": (_int, ()),
    "ntt_strerror": (ctypes.c_char_p, (_int,)),
    "ntt_sync_expiries": (_int, (_u32p,)),
    "ntt_small_batch_max": (_int, (_int, _int, _szp)),
    "ntt_small_batch_radix": (_int, (_int, _int, _sz, _intp)),
    "ntt_build_info": (_int, (ctypes.c_char_p, _sz)),
}

_lib = None
_FN: dict = {}   # name -> the library's function, signature applied (filled by lib())


def lib():
    """Load libqtesla_ntt.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"HIP library {LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # One HIP runtime per process: torch ships its own libamdhip64, loaded
        # into the global scope when torch is imported.  Importing it first
        # makes this library's hip* references bind to that same runtime; a
        # second runtime initialised after torch's finds no device
        # (hipErrorNoDevice from the host-buffer context, measured).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = _FN[name] = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


class NTTError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        msg = lib().ntt_strerror(code).decode()
        if code == NTT_ERR_HIP:
            msg += f" (hipError {lib().ntt_last_hip_error()})"
        super().__init__(f"{where}: {msg} [{code}]")
