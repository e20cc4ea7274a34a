"""The C-ABI library loads without a GPU and exports every symbol include/seevcn_hip.h declares."""
import ctypes

import pytest

import seevcn_amd._lib as L


def _declarations():
    with open(L.HEADER_PATH) as f:
        return L.parse_declarations(f.read())


def _declared_symbols():
    return sorted(_declarations())


def test_header_symbols_exported(hip_lib):
    names = _declared_symbols()
    assert len(names) >= 5
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in seevcn_hip.h but not exported"


def test_binding_table_matches_header(hip_lib):
    assert sorted(L.SIGNATURES) == _declared_symbols()


def test_binding_signatures_match_header_prototypes(hip_lib):
    """ctypes argtypes / restype of every binding against the header: parameter count, pointer vs int vs int64 vs float vs double."""
    protos = _declarations()
    assert sorted(protos) == _declared_symbols()

    def kind(ctype_decl):
        t = ctype_decl.rsplit(" ", 1)[0] if not ctype_decl.endswith("*") else ctype_decl
        if "*" in ctype_decl:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}[t.replace("const ", "")]

    for name, (ret, params) in protos.items():
        restype, argtypes = L.SIGNATURES[name]
        want_ret = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}[ret]
        assert restype == want_ret, (name, restype, ret)
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for a, p in zip(argtypes, params):
            assert a == kind(p), (name, p, a)


def test_every_mapped_type_is_pinned_once_by_hand():
    """The derived table against literals a person wrote: one entry for each type the parser maps."""
    c_p, c_i, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L.SIGNATURES["sv_last_error"] == (ctypes.c_char_p, [])
    assert L.SIGNATURES["sv_isolate_cluster_scratch_bytes"] == (c_i64, [c_i, c_i64])
    assert L.SIGNATURES["sv_index_persistent_bytes"] == (ctypes.c_size_t, [c_i64])
    assert L.SIGNATURES["sv_fill_f32"] == (c_i, [c_p, c_i64, ctypes.c_float, c_p])
    assert L.SIGNATURES["sv_vcn_largest_cluster"] == (c_i, [c_p, c_i, c_i, ctypes.c_double, c_i, c_i, c_p, c_p, c_p])


def test_parser_on_snippets():
    text = "/* int sv_not_this(int a); */\nint sv_one(const float* x, int64_t n,\n           void* stream);\nsize_t sv_two(void);\n"
    assert L.parse_declarations(text) == {"sv_one": ("int", ["const float* x", "int64_t n", "void* stream"]), "sv_two": ("size_t", [])}
    assert L.parse_prototypes(text) == {"sv_one": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]), "sv_two": (ctypes.c_size_t, [])}
    with pytest.raises(L.SeevcnHipError, match="unsigned x"):                      # a parameter type the binding does not map
        L.parse_prototypes("int sv_one(unsigned x);")
    with pytest.raises(L.SeevcnHipError, match="sv_two"):                          # a symbol that is there but not as a prototype
        L.parse_prototypes("int sv_one(int x);\nstatic inline int sv_two(int y) { return y; }\n")


def test_abi_version_and_sizes(hip_lib):
    assert hip_lib.sv_abi_version() == 1
    # 1024 cells = one chunk: 32 words * 8 B + 2 ints
    assert hip_lib.sv_index_persistent_bytes(1024) == 32 * 8 + 8
    assert hip_lib.sv_index_persistent_bytes(1025) == 2 * (32 * 8 + 8)
    assert hip_lib.sv_voxelize_dynamic_scratch_bytes(1000, 1 << 20, 1000) >= 1000 * 12


def test_ops_refuse_cpu_tensors(hip_lib):
    import torch
    from seevcn_amd.pcdet.ops import voxel_ops
    with pytest.raises(L.SeevcnHipError):
        voxel_ops.voxelize_dynamic(torch.zeros(4, 4), [0, 0, 0, 1, 1, 1], [1, 1, 1], [1, 1, 1], 1)


def test_ptr_refuses_what_is_not_on_the_device():
    import torch
    assert L.ptr(None) is None
    with pytest.raises(L.SeevcnHipError, match="GPU only"):
        L.ptr(torch.zeros(3))
    with pytest.raises(AssertionError, match="contiguous"):
        L.ptr(torch.zeros(4, 4).t())


def test_unguarded_wrappers_refuse_cpu_tensors_before_launching(hip_lib, monkeypatch):
    """The wrappers that had no device guard of their own, with all-CPU inputs of the smallest legal shape: ptr() raises while the arguments are
    built, so the entry is never called."""
    import torch
    from seevcn_amd.pcdet.utils import loss_utils
    from seevcn_amd.spconv import functional as F
    launched = []
    monkeypatch.setattr(L, "launch", lambda name, *args: launched.append(name))
    with pytest.raises(L.SeevcnHipError):
        loss_utils._FocalFunction.apply(torch.zeros(2, 3), torch.zeros(2, 3), torch.ones(2), 0.25, 2.0)
    with pytest.raises(L.SeevcnHipError):
        loss_utils._SmoothL1Function.apply(torch.zeros(2, 7), torch.zeros(2, 7), torch.ones(7), torch.ones(2), 1.0 / 9.0)
    with pytest.raises(L.SeevcnHipError):
        F.gather_gemm(torch.zeros(4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, 3), 4)
    assert launched == []
