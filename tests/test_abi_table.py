"""The ctypes ABI table of diff_gaussian_rasterization/_C.py held to the C headers under include/: the same names, the same
arity, the same kind of every parameter and return value, the same fields in the structs the ABI passes; an optional group a
library lacks is reported absent with its sentence; and the compiled extension's own list of entry points is a subset of the
table.  The package does not read include/ at run time: this test is the link between the two.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SCALARS = {"int": "int", "float": "float", "double": "double", "long long": "long long", "size_t": "size_t"}
CTYPES = {C.c_int: "int", C.c_float: "float", C.c_double: "double", C.c_longlong: "long long", C.c_size_t: "size_t", None: "void"}


def _code():
    """Every header with its comments and preprocessor lines taken out."""
    src = "\n".join(open(os.path.join(INCLUDE, h)).read() for h in sorted(os.listdir(INCLUDE)) if h.endswith(".h"))
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)


def c_kind(decl, named):
    """The kind of a C parameter declaration (named: its last word is the parameter's name) or of a return type."""
    decl = decl.strip()
    if "*" in decl or "[" in decl or "r3dgs_alloc_fn" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if named:
        assert len(words) >= 2, f"unnamed parameter: {decl!r}"
        words = words[:-1]
    kind = " ".join(words)
    if kind == "void" and not named:
        return "void"
    assert kind in SCALARS, f"a type this test does not know: {decl!r}"
    return SCALARS[kind]


def ctypes_kind(t):
    if t in CTYPES:
        return CTYPES[t]
    assert t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C._CFuncPtr)), f"a ctypes type this test does not know: {t!r}"
    return "pointer"


def header_prototypes():
    """{name: (return kind, [parameter kinds])} of every r3dgs_* prototype under include/."""
    out = {}
    for ret, name, params in re.findall(r"([\w \t\n\*]+?)\b(r3dgs_\w+)\s*\(([^()]*)\)\s*;", _code()):
        assert name not in out, f"{name} is declared twice"
        params = params.strip()
        kinds = [] if params in ("", "void") else [c_kind(p, True) for p in params.split(",")]
        out[name] = (c_kind(ret, False), kinds)
    return out


def header_structs():
    """{typedef name: [(field, kind)]} of every struct typedef under include/."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", _code()):
        fields = [f.strip() for f in body.split(";") if f.strip()]
        out[name] = [(re.sub(r"\[.*", "", f.split()[-1]).lstrip("*"), c_kind(f, True)) for f in fields]
    return out


@pytest.fixture(scope="module")
def mod():
    from diff_gaussian_rasterization import _C
    return _C


def table_rows(mod):
    rows = {}
    for group, (_, group_rows) in mod._ABI.items():
        for name, row in group_rows.items():
            assert name not in rows, f"{name} has two rows"
            rows[name] = row
    return rows


def test_parser_reads_what_the_headers_hold():
    protos = header_prototypes()
    assert "r3dgs_alloc_fn" not in protos and len(protos) >= 83
    assert protos["r3dgs_version"] == ("pointer", [])
    assert protos["r3dgs_forward_hint"] == ("void", ["int"])
    assert protos["r3dgs_ssim_window"] == ("void", ["pointer"])
    assert protos["r3dgs_binning_capacity"] == ("int", ["int", "int", "int", "size_t"])
    assert protos["r3dgs_row_mse_workspace_bytes"] == ("size_t", ["long long", "long long"])
    assert protos["r3dgs_forward"][1][:7] == ["pointer"] * 6 + ["int"]
    assert len(protos["r3dgs_backward"][1]) == 36


def test_every_prototype_has_its_row_and_every_row_its_prototype(mod):
    protos, rows = header_prototypes(), table_rows(mod)
    assert set(protos) - set(rows) == set(), "declared under include/ but not in the table"
    assert set(rows) - set(protos) == set(), "in the table but not declared under include/"
    for name, (ret, kinds) in sorted(protos.items()):
        restype, argtypes = rows[name]
        assert len(argtypes) == len(kinds), f"{name}: {len(argtypes)} argtypes, the header has {len(kinds)} parameters"
        assert ctypes_kind(restype) == ret, f"{name}: returns {ret}, the table says {restype!r}"
        for k, (t, kind) in enumerate(zip(argtypes, kinds)):
            assert ctypes_kind(t) == kind, f"{name}: parameter {k} is {kind}, the table says {t!r}"


def test_the_table_is_what_the_loaded_library_carries(mod):
    """_lib.<name>.argtypes stays readable: the one loop applied every row of every group the library has."""
    for group in mod._ABI:
        assert group in mod._present, f"the built library lacks the group {group}"
    for name, (restype, argtypes) in table_rows(mod).items():
        fn = getattr(mod._lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_structs_match_the_headers(mod):
    structs = header_structs()
    for name, cls in (("r3dgs_adam_segment", mod._AdamSegment), ("r3dgs_adam_capturable_segment", mod._AdamCapturableSegment),
                      ("r3dgs_densify_tensor", mod._DensifyTensor)):
        assert [(f, ctypes_kind(t)) for f, t in cls._fields_] == structs[name], name
    import r3dgs_densify
    assert r3dgs_densify._Tensor is mod._DensifyTensor
    # a pointer to each of them is what the entry points that take the struct are declared with
    rows = table_rows(mod)
    assert rows["r3dgs_adam_step_visible"][1][1] is C.POINTER(mod._AdamSegment)
    assert rows["r3dgs_adam_step_capturable"][1][1] is C.POINTER(mod._AdamCapturableSegment)
    assert rows["r3dgs_densify_move"][1][5] is C.POINTER(mod._DensifyTensor)


class _FakeFn:
    restype = argtypes = None


def _fake_library(mod, without=()):
    lib = type("FakeLibrary", (), {})()
    for name in table_rows(mod):
        if name not in without:
            setattr(lib, name, _FakeFn())
    return lib


def test_a_missing_optional_group_is_absent_and_says_so(mod, monkeypatch):
    optional = [g for g in mod._ABI if g != "required"]
    assert set(optional) == {"params", "quantised", "quantised_grad", "reduce_shards_mixed", "bwd_segments", "loss", "adam",
                             "adam_visible", "train_stats", "metrics", "densify"}
    todays = {   # the sentences of the eight _need_* functions and of r3dgs_densify's import, as they were
        "params": "the loaded libr3dgs_hip.so has no raw-parameter entry points: rebuild it with build.py",
        "quantised": "the loaded libr3dgs_hip.so has no quantised entry points: rebuild it with build.py",
        "quantised_grad": "the loaded libr3dgs_hip.so has no r3dgs_quantised_codebook_grad: rebuild it with build.py",
        "loss": f"{mod._LIB_PATH} has no fused loss (r3dgs_l1_ssim_forward): rebuild it with build.py",
        "adam": f"{mod._LIB_PATH} has no fused Adam (r3dgs_adam_step): rebuild it with build.py",
        "adam_visible": f"{mod._LIB_PATH} has no visibility-gated Adam (r3dgs_adam_step_visible): rebuild it with build.py",
        "train_stats": f"{mod._LIB_PATH} has no training statistics (r3dgs_visible_means): rebuild it with build.py",
        "metrics": f"{mod._LIB_PATH} has no evaluation metrics (r3dgs_image_metrics): rebuild it with build.py",
        "densify": f"{mod._LIB_PATH} has no densification (r3dgs_densify_plan): rebuild it with build.py",
    }
    assert mod._apply_abi(_fake_library(mod)) == set(mod._ABI)
    for group in optional:
        names = list(mod._ABI[group][1])
        lib = _fake_library(mod, without=names[-1:])   # one name short is the whole group short
        present = mod._apply_abi(lib)
        assert present == set(mod._ABI) - {group}
        assert all(getattr(lib, n).argtypes is None for n in names[:-1]), "rows of an absent group were applied"
        other = next(iter(mod._ABI["required"][1]))
        assert getattr(lib, other).argtypes == mod._ABI["required"][1][other][1]
        monkeypatch.setattr(mod, "_present", present)
        with pytest.raises(RuntimeError) as e:
            mod._need(group)
        assert "rebuild it with build.py" in str(e.value)
        if group in todays:
            assert str(e.value) == todays[group]
        for g in present - {"required"}:
            mod._need(g)
    with pytest.raises(AttributeError):   # the required group is not optional
        mod._apply_abi(_fake_library(mod, without=["r3dgs_backward"]))


def test_the_extension_names_entry_points_of_the_table(mod):
    assert mod._ext_loaded is not None, "the compiled binding is not built"
    listed = mod._ext_loaded.entry_points()
    names = [n for n, _ in listed]
    assert len(names) == len(set(names)) and len(names) >= 32
    rows = table_rows(mod)
    for name, required in listed:
        assert name in rows, f"{name}: bound by the extension, no row in the table"
        assert not required or name in mod._ABI["required"][1], f"{name}: marked required, not in the required group"
