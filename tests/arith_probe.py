"""Loader of the test-only probe library lib/libqtesla_ntt_arith.so
(ntt-gpu-qtesla_amd/tools/arith_probe.hip, `make testlibs`): the device
arithmetic primitives applied element-wise, and the library's constexpr
constant builders as host functions."""
import ctypes
import os

import arith_model as AM

PS_INDEX = {"ref": 0, "p-I": 1, "p-III": 2}
CONST_NAMES = ("Q", "N", "QNEG", "R", "NINV", "C1", "NINV_R", "C1_R", "NINV_R_SHORT", "C1_R_SHORT", "MUL_LOGR", "PSI",
               "AH", "WIDE", "OUT_CSUB_Z", "OUT_CSUB_H")
_lib = None


def path(ntt):
    return os.path.join(os.path.dirname(ntt.LIB_PATH), "libqtesla_ntt_arith.so")


def load(ntt):
    """The probe library, built through __graft_entry__.build() if it is missing."""
    global _lib
    if _lib is None:
        p = path(ntt)
        if not os.path.exists(p):
            import __graft_entry__
            __graft_entry__.build()
        ntt.lib()   # the HIP runtime torch loaded is bound first
        L = ctypes.CDLL(p)
        vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        L.arith_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, sz, vp, sz, sz, vp]
        L.arith_probe_consts.argtypes = [ctypes.c_int, ctypes.POINTER(u32)]
        L.arith_probe_cshoup.argtypes = [u32, u32]
        L.arith_probe_cshoup.restype = u32
        L.arith_probe_csigned_tw.argtypes = [u32, u32, ctypes.POINTER(u32)]
        L.arith_probe_csigned_tw.restype = None
        L.arith_probe_cqinv_neg.argtypes = [u32]
        L.arith_probe_cqinv_neg.restype = u32
        _lib = L
    return _lib


def consts(L, name):
    out = (ctypes.c_uint32 * 16)()
    assert L.arith_probe_consts(PS_INDEX[name], out) == 0
    return dict(zip(CONST_NAMES, (int(v) for v in out)))


def csigned_tw(L, w, q):
    out = (ctypes.c_uint32 * 2)()
    L.arith_probe_csigned_tw(w, q, out)
    return int(out[0]), int(out[1])


def run(L, prim, variant, name, d_in, in_words, d_out, out_words, count, stream=None):
    """arith_probe on raw device pointers; returns the library's status"""
    return L.arith_probe(AM.PRIMS[prim][0], variant, PS_INDEX[name], d_in, in_words, d_out, out_words, count, stream)
