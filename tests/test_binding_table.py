"""The Python binding against include/qtesla_ntt.h as a whole, without a GPU:
every prototype of the header against ntt_amd.SIGNATURES (name, arity, the
class of each argument and of the result) and against what lib() applied,
every integer #define NTT_* against its Python counterpart, and every device
wrapper's refusal of well-formed CPU operands before any library call."""
import ctypes
import inspect
import re

import pytest
import torch

SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
RESULTS = {"int": ctypes.c_int, "void": None, "void *": ctypes.c_void_p, "const char *": ctypes.c_char_p}


def header(ntt) -> str:
    with open(ntt.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def prototypes(ntt) -> dict:
    """name -> (result type, [argument types]) of every `ret name(args);` of the header"""
    src = re.sub(r"^\s*#.*$", "", header(ntt), flags=re.M)
    out = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(\w+)\s*\(([^()]*)\)\s*;", src):
        args = [" ".join(a.split()) for a in args.split(",")]
        types = [] if args == ["void"] else [re.match(r"(.*?)\w+$", a).group(1).strip() for a in args]
        assert name not in out, name
        out[name] = (" ".join(ret.split()), types)
    return out


def is_pointer(ctype) -> bool:
    return ctype in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))


def test_header_against_table(ntt):
    protos = prototypes(ntt)
    assert len(protos) >= 53, sorted(protos)
    assert set(ntt.SIGNATURES) == set(protos)
    L = ntt.lib()
    for name, (ret, types) in protos.items():
        restype, argtypes = ntt.SIGNATURES[name]
        assert restype is RESULTS[ret], (name, ret, restype)
        assert len(argtypes) == len(types), (name, types, argtypes)
        for i, (ctype, t) in enumerate(zip(argtypes, types)):
            if "*" in t:
                assert is_pointer(ctype), (name, i, t, ctype)
            else:
                assert ctype is SCALARS[t.replace("const ", "")], (name, i, t, ctype)
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


PARAM_KEYS = {"REF": "ref", "P_I": "p-I", "P_III": "p-III", "N4096": "p-III-4096", "N8192": "p-III-8192"}
KEYED = {"PARAM_": "PARAM_SETS", "OP_": "SWITCH_OPS", "RING_": "RINGS", "XOF_SHAKE": "XOF_ALGOS", "XOF_PATH_": "XOF_PATHS"}
NO_COUNTERPART = {"NTT_CHALLENGE_BLOCKS_MAX"}   # the device code's own bound, nothing a caller passes


def counterpart(ntt, name: str) -> int:
    """The Python value that mirrors #define NTT_<name> (KeyError / AttributeError: none)"""
    if name == "OK" or name.startswith("ERR_"):
        return getattr(ntt, "NTT_" + name)
    for prefix, table in KEYED.items():
        if name.startswith(prefix):
            key = name[len(prefix):]
            key = PARAM_KEYS[key] if prefix == "PARAM_" else ("shake" + key if prefix == "XOF_SHAKE" else key).lower()
            value = getattr(ntt, table)[key]
            if prefix == "XOF_PATH_":
                assert getattr(ntt, name) == value, name
            return value
    return getattr(ntt, name)


def test_header_against_constants(ntt):
    defines = {nm: int(v) for nm, v in re.findall(r"^\s*#\s*define\s+(NTT_\w+)\s+\(?(-?\d+)\)?\s*$", header(ntt), flags=re.M)}
    assert len(defines) >= 39, sorted(defines)
    assert len(NO_COUNTERPART) <= 3 and NO_COUNTERPART <= set(defines)
    for name, value in defines.items():
        if name in NO_COUNTERPART:
            continue
        try:
            mirrored = counterpart(ntt, name[len("NTT_"):])
        except (KeyError, AttributeError):
            pytest.fail(f"#define {name} has no Python counterpart")
        assert mirrored == value, name
    for prefix, table in KEYED.items():   # and no key the header lacks
        assert len(getattr(ntt, table)) == sum(nm.startswith("NTT_" + prefix) for nm in defines), table


N = 1024   # p-I


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


# every device wrapper with well-formed CPU operands at its smallest shapes: batch 1, p-I, k = l = h = 1, 8-byte
# seeds and messages, 8-bit fields (rows of n bytes, a multiple of 16)
CPU_CALLS = {
    "poly_ntt": lambda ntt: ntt.poly_ntt(i32(1, N), "p-I"),
    "poly_invntt": lambda ntt: ntt.poly_invntt(i32(1, N), "p-I"),
    "poly_ntt_oop": lambda ntt: ntt.poly_ntt_oop(i32(1, N), i32(1, N), "p-I"),
    "poly_invntt_oop": lambda ntt: ntt.poly_invntt_oop(i32(1, N), i32(1, N), "p-I"),
    "poly_ntt_bitrev": lambda ntt: ntt.poly_ntt_bitrev(i32(1, N), i32(1, N), "p-I"),
    "poly_invntt_bitrev": lambda ntt: ntt.poly_invntt_bitrev(i32(1, N), i32(1, N), "p-I"),
    "poly_bitrev_copy": lambda ntt: ntt.poly_bitrev_copy(i32(1, N), i32(1, N), "p-I"),
    "poly_mul": lambda ntt: ntt.poly_mul(i32(1, N), i32(1, N), i32(1, N), "p-I"),
    "poly_mul_ntt": lambda ntt: ntt.poly_mul_ntt(i32(1, N), i32(1, N), i32(1, N), "p-I"),
    "poly_pointwise": lambda ntt: ntt.poly_pointwise(i32(1, N), i32(1, N), i32(1, N), "p-I"),
    "poly_mul_nussbaumer": lambda ntt: ntt.poly_mul_nussbaumer(i32(1, N), i32(1, N), i32(1, N), "p-I"),
    "poly_mul_ntt_k": lambda ntt: ntt.poly_mul_ntt_k(i32(1, 1, N), i32(1, N), i32(1, N), "p-I", add=i32(1, 1, N)),
    "poly_mul_ntt_kl": lambda ntt: ntt.poly_mul_ntt_kl(i32(1, 1, N), [i32(1, N)], i32(1, 1, N), "p-I"),
    "poly_scatter": lambda ntt: ntt.poly_scatter(i32(1, N), i32(1, 1), i32(1, 1), "p-I"),
    "poly_round": lambda ntt: ntt.poly_round(i32(1, N), "p-I", 22, norms=i32(1, 2)),
    "poly_mul_ntt_kl_round": lambda ntt: ntt.poly_mul_ntt_kl_round([i32(1, N)], i32(1, 1, N), "p-I", 22, hi=u8(1, 1, N)),
    "poly_mul_ntt_kl_keyed": lambda ntt: ntt.poly_mul_ntt_kl_keyed(i32(1, 1, N), [i32(1, N)], i32(1, 1, 1, N), i32(1), "p-I"),
    "poly_mul_ntt_kl_round_keyed": lambda ntt: ntt.poly_mul_ntt_kl_round_keyed([i32(1, N)], i32(1, 1, 1, N), None, "p-I", 22,
                                                                               norms=i32(1, 1, 2)),
    "xof": lambda ntt: ntt.xof(u8(1, 8), u8(1, 8)),
    "xof_ragged": lambda ntt: ntt.xof_ragged(u8(1, 8), u8(8), torch.zeros(2, dtype=torch.int64)),
    "poly_challenge": lambda ntt: ntt.poly_challenge(i32(1, 1), i32(1, 1), u8(1, 8), "p-I"),
    "poly_sample_y": lambda ntt: ntt.poly_sample_y(i32(1, N), u8(1, 8), "p-I", 20, nonces=i32(1)),
    "poly_gen_a": lambda ntt: ntt.poly_gen_a(i32(1, 1, N), u8(1, 8), "p-I", 1, 1),
    "poly_sample_gauss": lambda ntt: ntt.poly_sample_gauss(i32(1, N), u8(1, 8), i32(1, 1), "p-I"),
    "poly_hsum": lambda ntt: ntt.poly_hsum(torch.zeros(1, dtype=torch.int64), i32(1, N), "p-I", 1),
    "poly_pack": lambda ntt: ntt.poly_pack(u8(1, N), i32(1, 1, N), "p-I", 8),
    "poly_unpack": lambda ntt: ntt.poly_unpack(i32(1, 1, N), u8(1, N), "p-I", 8, maxima=i32(1)),
    "poly_unpack_ntt": lambda ntt: ntt.poly_unpack_ntt(i32(N), u8(1, N), "p-I", 8, 1),
    "rows_over": lambda ntt: ntt.rows_over(i32(1), i32(1, 1), [0]),
    "rows_differ": lambda ntt: ntt.rows_differ(i32(1), u8(1, 4), u8(1, 4)),
    "select": lambda ntt: ntt.select(i32(1), i32(1), i32(1), False),
    "rows_move": lambda ntt: ntt.rows_move(u8(1, 4), u8(1, 4), count=i32(1)),
    "fill_uniform": lambda ntt: ntt.fill_uniform(i32(1, N), "p-I", 1),
}


def test_cpu_calls_cover_every_device_wrapper(ntt):
    """a device wrapper is a public function of the package that takes a stream"""
    wrappers = {name for name, f in vars(ntt).items()
                if inspect.isfunction(f) and not name.startswith("_") and "stream" in inspect.signature(f).parameters}
    assert wrappers == set(CPU_CALLS)


@pytest.mark.parametrize("name", sorted(CPU_CALLS))
def test_cpu_operands_are_refused_before_the_library(ntt, name, monkeypatch):
    called = []   # _run finds the entry points in ntt_amd._FN: none of them may be reached
    monkeypatch.setattr(ntt, "_FN", {nm: (lambda *a, nm=nm: called.append(nm)) for nm in ntt.SIGNATURES})
    with pytest.raises(ValueError, match="device tensors"):
        CPU_CALLS[name](ntt)
    assert not called
