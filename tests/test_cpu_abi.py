"""The ctypes boundary without a GPU: ex4dgs_amd/_abi.py -- the structures and the prototype table every call into libex4d_hip.so goes
through -- read against include/*.h: names, return types, every parameter in order, every structure field; plus the built library's
exports, its pure-host queries and the helpers `call` and `ptr`."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from ex4dgs_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8, "unsigned long long": ctypes.c_ulonglong}
UNMIRRORED = {"Ex4dFrameStatus"}         # read as tensor words (_C.PendingFrame); no prototype may name it


# ------------------------------------------------------------------ the header parser: regular expressions over comment-stripped text
def parse(header):
    """(prototypes [(name, return type, [parameter types])], structs {name: [(field, type, stars, array length or None)]}, opaque struct
    names, defines) of one header.  Everything in the header has to be recognised: a leftover fails."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^#define[ \t]+(\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$|^extern \"C\" \{$|^\}$", "", text, flags=re.M)
    structs = {}
    for name, body, again in re.findall(r"typedef struct (\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        assert name == again, (header, name, again)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            one = r"\s*\**\s*\w+(?:\[\w+\])?\s*"                              # a declarator: stars, name, array length
            m = re.fullmatch(rf"(?:const\s+)?([\w ]+?)((?:{one},)*{one})", decl)
            assert m, f"{header}: cannot account for {decl!r} in {name}"
            for d in m.group(2).split(","):
                stars, field, length = re.fullmatch(r"\s*(\**)\s*(\w+)(?:\[(\w+)\])?\s*", d).groups()
                fields.append((field, m.group(1), len(stars), length))
        structs[name] = fields
    text = re.sub(r"typedef struct \w+\s*\{.*?\}\s*\w+\s*;|enum\s*\{.*?\}\s*;", "", text, flags=re.S)
    opaque = set(re.findall(r"typedef struct (\w+) \1;", text))
    text = re.sub(r"typedef[^;]*;|^struct \w+;$", "", text, flags=re.M)          # the opaque handle, ex4d_alloc_fn, forward declarations
    protos = []
    for chunk in filter(None, (c.strip() for c in text.split(";"))):
        m = re.fullmatch(r"([\w\s\*]+?)\b(ex4d_\w+)\s*\(([^()]*)\)", chunk)
        assert m, f"{header}: cannot account for {chunk!r}"
        params = [] if m.group(3).strip() == "void" else [re.sub(r"\w+\s*$", "", p) for p in m.group(3).split(",")]
        protos.append((m.group(2), m.group(1), params))
    return protos, structs, opaque, defines


PARSED = {h: parse(h) for h in HEADERS}
STRUCTS = {n: f for _, s, _, _ in PARSED.values() for n, f in s.items()}
OPAQUE = set().union(*(o for _, _, o, _ in PARSED.values()))
DEFINES = {n: v for _, _, _, d in PARSED.values() for n, v in d.items()}


def allowed(ctype, stars=None):
    """The table entries that may stand for a C type (the mapping the boundary promises): scalars exactly; const char * -> c_char_p;
    ex4d_alloc_fn -> ALLOC_FN; pointer to a header structure -> POINTER(its mirror); the opaque handle and data pointers -> c_void_p,
    or POINTER of the matching scalar; void -> None."""
    base = " ".join(re.sub(r"\b(const|struct)\b|\*", " ", ctype).split())
    stars = ctype.count("*") if stars is None else stars
    if stars == 0:
        return {"void": [None], "ex4d_alloc_fn": [_abi.ALLOC_FN]}.get(base) or [getattr(_abi, base) if base in STRUCTS else SCALARS[base]]
    if base == "char":
        return [ctypes.c_char_p if stars == 1 else ctypes.POINTER(ctypes.c_char_p)]
    if base in STRUCTS:
        assert stars == 1 and base not in UNMIRRORED, ctype
        return [ctypes.POINTER(getattr(_abi, base))]
    if base in OPAQUE or (base == "void" and stars == 1):
        return [ctypes.c_void_p]
    return [ctypes.c_void_p, ctypes.POINTER(SCALARS[base] if stars == 1 else ctypes.c_void_p)]


# ------------------------------------------------------------------ the table against the headers
def test_the_table_covers_exactly_the_headers():
    assert set(_abi.PROTOTYPES) == set(HEADERS), set(_abi.PROTOTYPES) ^ set(HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_declared_names_equal_the_table_and_the_library_exports_them(header):
    """What test_c_abi_library_builds_loads_and_exports_declared_symbols, test_densify_abi_exports_and_struct_sizes and
    test_abi_exports_and_struct_sizes compared per module: the ex4d_* functions a header declares are the table's group for it (the
    module's EXPORTS), both directions, and a fresh handle of the built library has every one."""
    from ex4dgs_amd import _C, attributes, build, densify, loss, native_trainer, optim, regularizers
    from ex4dgs_amd.simple_knn import _C as knn
    modules = {"ex4d_rasterizer.h": _C, "ex4d_attributes.h": attributes, "ex4d_loss.h": loss, "ex4d_optim.h": optim, "ex4d_knn.h": knn,
               "ex4d_densify.h": densify, "ex4d_regularizers.h": regularizers, "ex4d_trainer.h": native_trainer}
    declared = [name for name, _, _ in PARSED[header][0]]
    last_error, protos = _abi.PROTOTYPES[header]
    table = [name for name, _, _, _ in protos]
    assert len(set(declared)) == len(declared) and len(set(table)) == len(table)
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert declared == table, "the table keeps the header's order"
    assert set(modules[header].EXPORTS) == set(declared) and last_error in declared and last_error.endswith("_last_error")
    handle = ctypes.CDLL(build.build())
    for name in declared:
        assert hasattr(handle, name), name


@pytest.mark.parametrize("header", HEADERS)
def test_prototypes_match_the_header(header):
    table = {name: (restype, argtypes, is_status) for name, restype, argtypes, is_status in _abi.PROTOTYPES[header][1]}
    for name, ret, params in PARSED[header][0]:
        restype, argtypes, is_status = table[name]
        assert restype in allowed(ret), f"{name}: returns {ret.strip()!r}, the table says {restype}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table"
        for i, (c, a) in enumerate(zip(params, argtypes)):
            assert a in allowed(c), f"{name}: parameter {i} is {c.strip()!r}, the table says {a}"
        assert not is_status or ret.strip() == "int", f"{name}: only an int return can be a status"


def test_integer_returns_are_statuses_except_the_five_values():
    ints = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64)
    values = {n for _, protos in _abi.PROTOTYPES.values() for n, r, _, is_status in protos if r in ints and not is_status}
    assert values == {"ex4d_get_option", "ex4d_abi_version", "ex4d_profile_read", "ex4d_radam_sliced_reg_rows", "ex4d_trainer_replays"}


def test_struct_mirrors_match_the_headers():
    used = {" ".join(re.sub(r"\b(const|struct)\b|\*", " ", c).split()) for protos, _, _, _ in PARSED.values() for _, r, ps in protos for c in ps + [r]}
    assert len(STRUCTS) == sum(len(s) for _, s, _, _ in PARSED.values()), "a structure name is declared twice"
    for name, fields in STRUCTS.items():
        if name in UNMIRRORED:
            assert name not in used and not hasattr(_abi, name)
            continue
        mirror = getattr(_abi, name)
        assert [f for f, _ in mirror._fields_] == [f for f, _, _, _ in fields], f"{name}: field names / order"
        for (field, got), (_, base, stars, length) in zip(mirror._fields_, fields):
            if length is not None:
                n = int(length) if length.isdigit() else DEFINES[length]
                assert issubclass(got, ctypes.Array) and got._length_ == n, f"{name}.{field}: array of {n}"
                got = got._type_
            assert got in allowed(base, stars), f"{name}.{field} is {base.strip()!r} with {stars} '*', the mirror says {got}"
    assert used & set(STRUCTS) and _abi.Ex4dSplitSHGrad is _abi.Ex4dSplitSH
    assert (_abi.RADAM_MAX_WINDOWS, _abi.TRAINER_PARAMS) == (DEFINES["EX4D_RADAM_MAX_WINDOWS"], DEFINES["EX4D_TRAINER_PARAMS"])


def test_load_binds_the_whole_table_once():
    lib = _abi.load()
    assert lib is _abi.load()
    for _, protos in _abi.PROTOTYPES.values():
        for name, restype, argtypes, _ in protos:
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ------------------------------------------------------------------ the helpers
def test_call_raises_the_headers_own_message():
    lib = _abi.load()
    with pytest.raises(RuntimeError) as e:
        _abi.call("ex4d_set_option", b"no_such_option", 1)                # a pure-host refusal
    assert str(e.value) == lib.ex4d_last_error().decode() != "" and "unknown option" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        _abi.call("ex4d_reg_forward", None, 0, None, None, 0, 1, 0.0, 0.0, 0.0, None, None, None)     # no output: refused before any HIP call
    assert str(e.value) == lib.ex4d_reg_last_error().decode() != ""
    assert _abi.call("ex4d_set_option", b"depth_sort_msd", 3) is None
    with pytest.raises(KeyError):
        _abi.call("ex4d_get_option", b"depth_sort_msd")                   # a value, not a status: read it from load()


def test_ptr_is_null_for_absent_and_empty_tensors():
    t = torch.zeros(3)
    assert _abi.ptr(None) is None and _abi.ptr(torch.empty(0)) is None and _abi.ptr(torch.empty(0, 3)) is None
    assert _abi.ptr(t) == t.data_ptr() != 0


# ------------------------------------------------------------------ the built library: loads, answers its host-side queries
def test_c_abi_library_builds_loads_and_exports_declared_symbols():
    from ex4dgs_amd import build, _C, attributes, native_trainer as nt_mod, optim as optim_mod
    lib = build.build()
    assert os.path.exists(lib)
    assert ctypes.sizeof(attributes.Ex4dAttrParams) == 13 * 4
    assert ctypes.sizeof(optim_mod.Ex4dRadamTensor) == 64
    assert ctypes.sizeof(nt_mod.Ex4dTrainerConfig) == 280 and nt_mod.Ex4dTrainerConfig.optimizer.offset == 272
    l = _C.load()
    assert l.ex4d_abi_version() == 5 and l.ex4d_target_arch() == b"gfx950"
    # size / layout queries are pure host code
    P = 1000
    lay = _C.GeomLayout(); l.ex4d_geom_layout(P, ctypes.byref(lay))
    assert lay.total == l.ex4d_geom_bytes(P) and lay.cov3D >= 64 * P and lay.cov3D % 256 == 0 and lay.records == 0
    assert l.ex4d_binning_bytes(0, 64, 64) > 0 and l.ex4d_img_bytes(1352, 1014) >= 1352 * 1014 * 8 + 5440 * 8
    assert l.ex4d_backward_scratch_bytes(P) >= P * 64
    assert ctypes.sizeof(_C.Ex4dParams) == 17 * 4
    # library options are host state: the depth sort's default is "auto" (3), values beyond it and unknown names are refused
    assert _C.get_option("depth_sort_msd") == 3 and _C.get_option("depth_sort_hold") == 0 and _C.get_option("depth_sort_trips") == 0
    for v in (0, 1, 2, 3):
        _C.set_option("depth_sort_msd", v)
        assert _C.get_option("depth_sort_msd") == v
    with pytest.raises(RuntimeError):
        _C.set_option("depth_sort_msd", 4)
    with pytest.raises(RuntimeError):
        _C.set_option("depth_sort_hold", 1)              # read-only
    assert _C.get_option("no_such_option") == -1
    # the kernels are gfx950 code objects
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", f"--input={lib}"], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        assert "gfx950" in out.stdout


def test_densify_abi_exports_and_struct_sizes():
    from ex4dgs_amd import densify
    assert ctypes.sizeof(densify.Ex4dDensifyPlanGroup) == 104
    assert ctypes.sizeof(densify.Ex4dDensifyTensor) == 72
    assert ctypes.sizeof(densify.Ex4dDensifyApplyGroup) == 80
    assert _abi.load().ex4d_densify_scratch_bytes(0) == 0


def test_abi_exports_and_struct_sizes():
    from ex4dgs_amd import native_trainer, optim
    handle = _abi.load()
    assert {"ex4d_radam_step_sliced_reg", "ex4d_radam_sliced_reg_rows"} <= set(optim.EXPORTS)
    assert "ex4d_trainer_set_regularizers" in native_trainer.EXPORTS
    assert ctypes.sizeof(optim.Ex4dRadamSlicedRegTensor) == ctypes.sizeof(optim.Ex4dRadamSlicedTensor) + 24
    assert optim.Ex4dRadamSlicedRegTensor.t.offset == 0
    assert handle.ex4d_reg_scratch_bytes() % 8 == 0 and handle.ex4d_reg_scratch_bytes() > 0
    # rows per workgroup of the fused step: a multiple of 4 (16-byte aligned spans for odd K C), the staged span within the LDS budget,
    # 0 when four rows do not fit -- pure host code
    rows = handle.ex4d_radam_sliced_reg_rows
    for K in (1, 2, 4, 35, 100, 300, 682, 683, 1024, 1025, 5000):
        for Cc in (3, 4):
            R = rows(K, Cc)
            assert R % 4 == 0 and 0 <= R <= 32
            assert (R == 0) == (2 * 4 * K * Cc * 4 > 32768), (K, Cc, R)
            assert 2 * R * K * Cc * 4 <= 32768
    assert rows(35, 3) == 32 and rows(35, 4) >= 16
    assert rows(35, 5) == 0 and rows(0, 3) == 0
