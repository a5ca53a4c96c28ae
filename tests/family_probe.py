"""Loader of the test-only probe library lib/libqtesla_ntt_family.so
(ntt-gpu-qtesla_amd/tools/family_probe.hip, `make testlibs`): every transform
and product kernel the product compiles, launched by the family and the chunk
length the caller names -- and the enumerations the tests of it share."""
import ctypes
import os

from conftest import LARGE_SETS, PARAM_SETS

ALL_SETS = PARAM_SETS + LARGE_SETS
KINDS = ("fwd", "inv", "fwd_br", "inv_br", "bitrev")        # family_probe_xform's kind
OPS = KINDS + ("mul", "mul_ntt")                            # family_probe_shape's op
OP = {name: i for i, name in enumerate(OPS)}
TRANSFORMS = KINDS[:4]
PRODUCTS = OPS[5:]
RADIX_FAMILIES = (2, 3, 4)                                  # radix 4 / 8 / 16, one polynomial per workgroup
BATCH = 0                                                   # the batch kernels
CHUNK_MAX = 16                                              # NTT_PPW_MAX
CHUNKS = (1, 2, 3, 5, 16)                                   # the chunk lengths the GPU test walks
_N = {"ref": 1024, "p-I": 1024, "p-III": 2048, "p-III-4096": 4096, "p-III-8192": 8192}
_lib = None


def path(ntt):
    return os.path.join(os.path.dirname(ntt.LIB_PATH), "libqtesla_ntt_family.so")


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
        i, vp, sz, pu32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)
        L.family_probe_xform.argtypes = [i, i, i, vp, vp, sz, i, vp]
        L.family_probe_mul.argtypes = [i, i, i, vp, vp, vp, sz, i, vp]
        L.family_probe_shape.argtypes = [i, i, i, sz, i, pu32, pu32, pu32, pu32]
        L.family_probe_set_cus.argtypes = [i]
        L.family_probe_consts.argtypes = [pu32]
        L.family_probe_sync_expiries.argtypes = [pu32]
        _lib = L
    return _lib


def family_id(family):
    return f"radix{1 << family}" if family else "batch"


def upw(ps):
    """Polynomials per work unit of the n <= 2048 batch kernels: a wave takes
    two n = 1024 polynomials (test_family_probe_abi.py binds this to the probe)."""
    return 2 if _N[ps] == 1024 else 1


def instantiations():
    """Every (ps, op, family) csrc/ntt_kernels.hip compiles a kernel for:
    LXform<PS>::run's three one-polynomial families and its batch kernels for
    the four transforms, the bit-reversal copy (batch kernels only), and
    LMul<PS>::run's batch kernels and radix-4 kernels (k_poly_mul_lat: n <= 4096)."""
    out = []
    for ps in ALL_SETS:
        for op in TRANSFORMS:
            out += [(ps, op, f) for f in RADIX_FAMILIES + (BATCH,)]
        out.append((ps, "bitrev", BATCH))
        for op in PRODUCTS:
            if _N[ps] <= 4096:
                out.append((ps, op, 2))
            out.append((ps, op, BATCH))
    return out


def walk_batches(per, upw, chunk):
    """[(batch, grid)]: the batches at which a batch kernel whose workgroup
    takes W = `per` units per pass walks chunk `chunk` through every path of
    its loop, and the grid the probe must launch for each.
      units = 2 W c + W (c // 2) + W // 2 + 1, batch = units upw - (upw - 1):
        workgroups 0 and 1 walk a full chunk, workgroup 2 stops mid-chunk in a
        pass where only W // 2 + 1 waves have a unit; with upw = 2 the batch
        is odd and the last unit holds one polynomial
      units = 2 W c: two full workgroups, no tail
      batch = 1"""
    W, c = per, chunk
    units = 2 * W * c + W * (c // 2) + W // 2 + 1
    return [(units * upw - (upw - 1), 3), (2 * W * c * upw, 2), (1, 1)]


# launch_shape() of csrc/launch_shape.hpp and the constants batch_shape /
# large_shape of csrc/ntt_kernels.hip pass to it, restated: (waves per pass,
# threads, minimum workgroups per CU) per (kind of set, op).  A tuning round
# that moves one of them (NTT_WG, MUL_WG, BIG_WAVES_8192, BIG_MUL_WAVES,
# MUL_LARGE_INC_WAVES, NTT_MIN_WG_PER_CU) updates this table with it.
def _launch_shape(items, per, cus, per_cu, max_chunk):
    chunk = min(max(items // (per * cus * per_cu), 1), max_chunk)
    return -(-items // (per * chunk)), chunk


_RULE = {"small": {**{op: (8, 512, 4) for op in KINDS}, "mul": (8, 512, 4), "mul_ntt": (16, 1024, 4)},
         "p-III-4096": {**{op: (16, 1024, 2) for op in TRANSFORMS}, "mul": (4, 256, 2), "mul_ntt": (8, 512, 2)},
         "p-III-8192": {**{op: (8, 512, 2) for op in TRANSFORMS}, "mul": (2, 512, 2), "mul_ntt": (4, 1024, 2)}}


def expected_shape(ps, op, batch, cus):
    """dict(grid, block, chunk, per) of a family-0 launch under the product's rule on a device with `cus` CUs"""
    if ps in LARGE_SETS and op == "bitrev":   # capped_grid(batch, 1, cus, 64): one polynomial per workgroup step
        grid = min(batch, cus * 64)
        return dict(grid=grid, block=512, chunk=-(-batch // grid), per=1)
    per, block, per_cu = _RULE[ps if ps in LARGE_SETS else "small"][op]
    grid, chunk = _launch_shape(-(-batch // upw(ps)), per, cus, per_cu, CHUNK_MAX)
    return dict(grid=grid, block=block, chunk=chunk, per=per)


def shape(L, family, op, ps_index, batch, chunk=0):
    """(rc, dict(grid, block, chunk, per)) of family_probe_shape"""
    g, b, c, p = (ctypes.c_uint32() for _ in range(4))
    rc = L.family_probe_shape(family, OP[op], ps_index, batch, chunk, g, b, c, p)
    return rc, dict(grid=g.value, block=b.value, chunk=c.value, per=p.value)


def consts(L):
    out = (ctypes.c_uint32 * 2)()
    assert L.family_probe_consts(out) == 0
    return dict(min_wg_per_cu=int(out[0]), ppw_max=int(out[1]))


def sync_expiries(L):
    n = ctypes.c_uint32(0xFFFFFFFF)
    assert L.family_probe_sync_expiries(n) == 0
    return n.value


def _raw_stream(ntt, t, stream):
    return ntt._stream(stream, t.device)


def xform(L, ntt, family, kind, ps, out, inp, chunk=0, stream=None):
    """family_probe_xform on [batch * n] device tensors; returns the status"""
    n = _N[ps]
    assert out.numel() == inp.numel() and inp.numel() % n == 0 and out.is_contiguous() and inp.is_contiguous()
    return L.family_probe_xform(family, OP[kind], ntt.PARAM_SETS[ps], out.data_ptr(), inp.data_ptr(), inp.numel() // n, chunk,
                                _raw_stream(ntt, out, stream))


def mul(L, ntt, family, op, ps, c, a, b, chunk=0, stream=None):
    """family_probe_mul (op "mul" / "mul_ntt") on [batch * n] device tensors; returns the status"""
    n = _N[ps]
    assert c.numel() == a.numel() == b.numel() and a.numel() % n == 0
    assert c.is_contiguous() and a.is_contiguous() and b.is_contiguous()
    return L.family_probe_mul(family, int(op == "mul_ntt"), ntt.PARAM_SETS[ps], c.data_ptr(), a.data_ptr(), b.data_ptr(),
                              a.numel() // n, chunk, _raw_stream(ntt, c, stream))
