"""The Python binding against the C header: every prototype of include/sextans_amd.h is declared in api._PROTOTYPES with the same kinds of
parameters and result, every declared name is in the header and exported by the built library, the rule for entry points that a library
lacks, and the arity check of the decorator that declares the forwarding Engine methods (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

from util import ROOT

# header functions deliberately left without a binding: (name, reason)
UNBOUND = []

SCALARS = {"int": "int", "int64_t": "int64", "uint64_t": "uint64", "size_t": "uint64", "float": "float", "double": "double"}
CTYPES = {C.c_int: "int", C.c_int64: "int64", C.c_uint64: "uint64", C.c_size_t: "uint64", C.c_float: "float", C.c_double: "double"}


def c_kind(decl, named):
    """Kind of a C parameter (named) or return type (not named) as the header writes it."""
    if "*" in decl or "[" in decl or "sextans_handle_t" in decl.split():
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if named and len(words) > 1:
        words = words[:-1]
    assert len(words) == 1 and (words[0] in SCALARS or (words[0] == "void" and not named)), decl
    return SCALARS.get(words[0], "void")


def ctypes_kind(t):
    if t is None:
        return "void"
    if issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)):   # (an ndpointer is a subclass of c_void_p)
        return "pointer"
    return CTYPES[t]


def header_prototypes():
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"(?<=[;{}])\s*([\w\s]+?[\s\*]+)(sextans_\w+)\s*\(([^()]*)\)\s*(?=;)", ";" + text):
        assert name not in out, name
        params = [] if params.strip() == "void" else params.split(",")
        out[name] = (c_kind(ret, False), [c_kind(q, True) for q in params])
    return out


@pytest.fixture(scope="module")
def header():
    return header_prototypes()


def test_parser_finds_every_prototype(header):
    assert len(header) >= 157, len(header)
    assert header["sextans_init_dense_B"] == ("void", ["int", "int", "pointer"])
    assert header["sextans_last_error"] == ("pointer", [])
    assert header["sextans_gflops"] == ("double", ["int", "int", "int64", "double"])
    assert header["sextans_dist_unique_id"] == ("int", ["pointer"])                    # char uid[128]
    assert header["sextans_device_alloc"] == ("int", ["int", "uint64", "pointer"])      # size_t
    assert header["sextans_update_values_device"] == ("int", ["pointer", "pointer", "pointer"])   # sextans_handle_t


def test_binding_matches_header(sx, header):
    from sextans_amd import api
    unbound = {name for name, _ in UNBOUND}
    for name, (ret, params) in header.items():
        if name in unbound:
            continue
        assert name in api._PROTOTYPES, name + " is declared in the header and not bound"
        restype, argtypes = api._PROTOTYPES[name]
        assert [ctypes_kind(t) for t in argtypes] == params, name
        assert ctypes_kind(restype) == ret, name
    assert set(api._PROTOTYPES) <= set(header), sorted(set(api._PROTOTYPES) - set(header))
    assert unbound.isdisjoint(api._PROTOTYPES)


def test_every_bound_name_is_exported(sx):
    from sextans_amd import api
    raw = C.CDLL(api.LIB_PATH)
    for name in api._PROTOTYPES:
        assert hasattr(raw, name), name
    assert api._ROUND4_SYMBOLS <= set(api._PROTOTYPES)
    assert api._OPTIONAL_SYMBOLS == set(api._PROTOTYPES) - api._ROUND4_SYMBOLS
    L = api.lib()
    for name, (restype, argtypes) in api._PROTOTYPES.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name


class FakeLibrary:
    """Every entry point of the binding but `lacking`, as objects that take a prototype."""
    class Function:
        restype = argtypes = "unset"

    def __init__(self, names, lacking):
        for name in names:
            if name != lacking:
                setattr(self, name, FakeLibrary.Function())


def test_load_rule_for_a_missing_symbol(sx):
    from sextans_amd import api
    optional, round4 = "sextans_edge_dot_device", "sextans_spmm_device"
    assert optional in api._OPTIONAL_SYMBOLS and round4 in api._ROUND4_SYMBOLS
    L = api._bind(FakeLibrary(api._PROTOTYPES, optional))       # an older build: the load succeeds, the others are declared
    assert not hasattr(L, optional)
    assert L.sextans_spmm_device.argtypes == api._PROTOTYPES["sextans_spmm_device"][1]
    assert L.sextans_host_free.restype is None
    with pytest.raises(AttributeError, match=round4 + r"\b"):
        api._bind(FakeLibrary(api._PROTOTYPES, round4))


def test_entry_checks_the_number_of_kinds_at_import():
    from sextans_amd import api
    before = dict(api._PROTOTYPES)
    with pytest.raises(TypeError, match="three_parameters"):
        @api._entry(api.i, api.p)
        def three_parameters(self, N, d_x, ldx, stream=None):
            """never bound"""
    with pytest.raises(TypeError, match="no_stream"):
        @api._entry(api.i, api.p, result=api.l)
        def no_stream(self, a, b, c):
            """never bound"""
    assert api._PROTOTYPES == before
