"""CPU checks of the 'H' decoder's interface: the header declares the entry points, the library
exports them, and the Python binding's argument types match the declarations."""
import ctypes
import os
import re

from bwtc_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bwtc_hip.h")).read()

_C = {"bwtc_hip_ctx*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p,
      "uint64_t": ctypes.c_uint64, "uint32_t*": ctypes.POINTER(ctypes.c_uint32),
      "uint64_t*": ctypes.POINTER(ctypes.c_uint64), "bwtc_hip_huffman_decode_stats*": None}
ENTRIES = ["bwtc_hip_huffman_decode", "bwtc_hip_huffman_decode_device", "bwtc_hip_decode_block_H",
           "bwtc_hip_huffman_decode_stats_get"]


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, HEADER)
    assert m, name
    return [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_and_library_exports():
    lib = ctypes.CDLL(os.path.join(ROOT, "bwtc_amd", "lib", "libbwtc_hip.so"))
    for name in ENTRIES:
        _params(name)
        assert hasattr(lib, name), name
    for code in ("NO_CODE", "SHAPE", "PAST_RECORD", "RUNS", "CAPACITY", "LENGTH"):
        m = re.search(r"#define BWTC_HIP_E_%s\s+\((-\d+)\)" % code, HEADER)
        assert m and int(m.group(1)) == getattr(hip, "E_" + code), code


def test_binding_argtypes_match_header():
    L = hip.load()
    for name in ENTRIES:
        want = _params(name)
        got = getattr(L, name).argtypes
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            c = _C[w]
            if c is None:
                continue
            if c is ctypes.c_void_p:
                assert g is ctypes.c_void_p, (name, w, g)
            elif isinstance(c, type) and issubclass(c, ctypes._Pointer):
                assert g in (c, ctypes.c_void_p) or (hasattr(g, "_type_") and g._type_ is c._type_), (name, w, g)
            else:
                assert g is c, (name, w, g)


def test_stats_struct_layout():
    m = re.search(r"typedef struct bwtc_hip_huffman_decode_stats \{(.*?)\} bwtc_hip_huffman_decode_stats;", HEADER, re.S)
    fields = re.findall(r"(uint32_t|uint64_t|float)\s+(\w+);", m.group(1))
    assert [f for _, f in fields] == [f for f, _ in hip.HuffmanDecodeStats._fields_]
    size = {"uint32_t": 4, "uint64_t": 8, "float": 4}
    off = 0
    for t, _ in fields:
        off = (off + size[t] - 1) // size[t] * size[t] + size[t]
    assert ctypes.sizeof(hip.HuffmanDecodeStats) == (off + 7) // 8 * 8
