"""CPU tests of the C ABI: libryolo_hip.so loads and exports every symbol include/ryolo.h declares (no compute without a GPU), the ctypes
binding that r-yolov4_amd/abi.py reads from the two headers is the one the C compiler sees (argument kinds pinned by hand, struct layouts
field by field against a compiled `offsetof` program), the reader refuses what it does not know, and the product path refuses CPU tensors
instead of silently falling back."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F, D, Z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
BLOCKS = ["TapClass", "ConvGemmParams", "WgradParams", "StemParams", "StemWgradParams", "StemBwdParams", "BnActParams", "PoolParams", "UpParams",
          "PackEntry", "LossParams"]
RECORDS = ["PasteRect", "ResizeItem", "WindowItem", "PasteItem", "LabelRow"]


def _declared():
    txt = open(os.path.join(ROOT, "include", "ryolo.h")).read()
    return sorted(set(re.findall(r"\b(ryolo_[a-z0-9_]+)\s*\(", txt)) - {"ryolo_stream_t"})


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from ryolov4_amd import hip
    L = hip.lib()
    declared = _declared()
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(L, name), name
    assert set(hip.exported_symbols()) == set(declared), set(hip.exported_symbols()) ^ set(declared)


def test_every_prototype_is_read():
    from ryolov4_amd import abi, hip
    declared = _declared()
    assert len(abi.PROTOTYPES) == len(declared) == 108
    assert sorted(abi.PROTOTYPES) == declared
    assert all(hip._SIGNATURES[n] == abi.PROTOTYPES[n] for n in declared)
    assert sorted(abi.STRUCTS) == sorted(BLOCKS + RECORDS)


def test_argument_mapping_pinned_by_hand():
    """One entry point per rule of abi.py, its argtypes written out from the C prototype by hand."""
    from ryolov4_amd import abi
    S, PTR = abi.STRUCTS, C.POINTER
    want = {
        # float* x4, int64_t, double x4, int64_t, float, int, stream
        "ryolo_adam": [P, P, P, P, L, D, D, D, D, L, F, I, P],
        # const float*, int, int, double, float, float, const float* x2, float* x3, stream
        "ryolo_bn_finalize": [P, I, I, D, F, F, P, P, P, P, P, P],
        "ryolo_scene_errors": [P, P, L, P, P, L, I, F, F, F, F, F, P, P, P, P, P, P, P, P, P, P, L, P, P, P, Z, P],
        # no stream: the scalar pointer is a host out-parameter
        "ryolo_nms_workspace_bytes": [I, L, PTR(Z)],
        "ryolo_paste_rect_bytes": [PTR(I)],
        "ryolo_conv_wgrad_plan": [PTR(S["WgradParams"]), PTR(I), PTR(Z)],
        "ryolo_stem3x3_plan": [I, I, I, I, PTR(I), PTR(Z)],
        # a stream: `int*` / `const int*` / `unsigned char*` are device addresses
        "ryolo_encode_labels": [P, L, I, I, P, P, I, P, P, P, P],
        "ryolo_conv_gemm": [PTR(S["ConvGemmParams"]), P],
        "ryolo_anchor_reach": [PTR(S["LossParams"]), P, P, P],
        # the explicit list
        "ryolo_loss_grad_scale_multi": [PTR(P * 8), PTR(L * 8), I, P, P],
        "ryolo_loss_owner_grids": [PTR(S["LossParams"]), PTR(P * 3)],
        "ryolo_loss_match_records": [PTR(S["LossParams"]), PTR(P * 3), PTR(P * 3)],
        "ryolo_decode": [I, P, P, I, I, I, I, F, PTR(F), L, L, P],
        "ryolo_pack_weights": [P, I, L, P],
    }
    assert len(want["ryolo_scene_errors"]) == 28
    for name, sig in want.items():
        assert abi.PROTOTYPES[name] == sig, (name, abi.PROTOTYPES[name])
    assert {f for f, _ in abi.OVERRIDES} == {"ryolo_decode", "ryolo_loss_owner_grids", "ryolo_loss_match_records", "ryolo_loss_grad_scale_multi",
                                             "ryolo_pack_weights"}


def test_struct_fields_pinned_by_hand():
    """The field kinds the reader must handle: comma-declared, fixed and multi-dimensional arrays, a nested struct array, signed char."""
    from ryolov4_amd import abi
    S = abi.STRUCTS
    assert S["TapClass"]._fields_ == [("ntaps", I), ("oh_add", I), ("ow_add", I), ("dh", C.c_byte * 9), ("dw", C.c_byte * 9), ("widx", C.c_byte * 9)]
    cg = dict(S["ConvGemmParams"]._fields_)
    assert cg["cls"] is S["TapClass"] * 4 and cg["A"] is P and cg["a_bytes"] is C.c_uint and cg["w_bytes"] is C.c_uint
    lp = dict(S["LossParams"]._fields_)
    assert lp["anchors"] is (F * 3 * 18) * 3 and lp["head"] is P * 3 and lp["gs"] is I * 3 and lp["ws_bytes"] is Z
    assert S["PasteItem"]._fields_ == [("src_off", L), ("SH", I), ("SW", I), ("slot", I), ("cls", F), ("quad", F * 8), ("M", D * 6), ("Minv", D * 6)]
    assert dict(S["WgradParams"]._fields_)["kchunk"] is L
    assert [n for n, _ in S["UpParams"]._fields_] == ["x", "ldx", "z", "ldz", "NB", "H", "W", "C", "accum"]


def test_layouts_match_the_c_compiler_field_by_field(tmp_path):
    """sizeof, and offsetof + sizeof of every field, of all sixteen structs as the host C compiler lays out include/ryolo_params.h."""
    from ryolov4_amd import abi
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler (cc) to check the struct layouts with"
    names = BLOCKS + RECORDS
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ryolo_params.h"', "int main(void) {"]
    for s in names:
        lines.append(f'    printf("{s} %zu\\n", sizeof({s}));')
        for f, _ in abi.STRUCTS[s]._fields_:
            lines.append(f'    printf("{s}.{f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out if ln}
    want = {}
    for s in names:
        t = abi.STRUCTS[s]
        want[s] = (C.sizeof(t),)
        for f, _ in t._fields_:
            want[f"{s}.{f}"] = (getattr(t, f).offset, getattr(t, f).size)
    assert len(names) == 16 and got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


def test_numpy_records_are_the_generated_classes():
    import numpy as np
    from ryolov4_amd import abi
    from ryolov4_amd.datasets import augment as A
    for dt, t in ((A.LABEL_ROW_DTYPE, A._LabelRow), (A.PASTE_ITEM_DTYPE, A._PasteItem)):
        assert t in (abi.STRUCTS["LabelRow"], abi.STRUCTS["PasteItem"])
        assert dt.itemsize == C.sizeof(t) and list(dt.names) == [f for f, _ in t._fields_]
        assert all(dt.fields[f][1] == getattr(t, f).offset for f in dt.names)
    assert np.zeros(2, dtype=A.PASTE_ITEM_DTYPE)["M"].shape == (2, 6) and A.LABEL_ROW_DTYPE["poly"].base == np.float32


@pytest.mark.parametrize("text, what", [
    ("int ryolo_x(widget_t a, ryolo_stream_t stream);", "unknown type"),
    ("int ryolo_x(struct foo* a);", "unknown type"),
    ("typedef struct X { int a : 3; } X;", "field not understood"),
    ("typedef struct X { float *a, *b; } X;", "field not understood"),
    ("typedef struct X { int a; union { int b; float c; } u; } X;", "unknown type"),
    ("int ryolo_x(int a)", "unterminated"),
    ("typedef struct X { int a;", "unterminated"),
    ("float ryolo_x(int a);", "declaration not understood"),
    ("int ryolo_x(int a); int ryolo_x(int b);", "declaration not understood"),
    ("#if FOO\nint ryolo_x(int a);\n#endif", "preprocessor"),
    ("int ryolo_x(LossParams p);", "by value"),
])
def test_reader_refuses_what_it_does_not_know(text, what):
    from ryolov4_amd import abi
    with pytest.raises(abi.AbiError, match=what):
        abi.parse("typedef struct LossParams { int mode; } LossParams;\ntypedef struct ihipStream_t* ryolo_stream_t;\n" + text)


def test_reader_reads_the_subset():
    from ryolov4_amd import abi
    structs, protos = abi.parse("""
        #define N 4   // a constant
        typedef unsigned short half_t;
        typedef struct ihipStream_t* ryolo_stream_t;
        typedef struct B { const half_t* p; int a, b[N]; signed char t[2][N]; /* c */ size_t n; } B;
        int ryolo_f(const B* p, half_t* out, int* dev, double x, ryolo_stream_t stream);
        int ryolo_q(int n, int* rows, size_t* bytes);
    """)
    assert structs["B"]._fields_ == [("p", P), ("a", I), ("b", I * 4), ("t", (C.c_byte * 4) * 2), ("n", Z)]
    assert protos == {"ryolo_f": [C.POINTER(structs["B"]), P, P, D, P], "ryolo_q": [I, C.POINTER(I), C.POINTER(Z)]}


def test_product_path_has_no_cpu_fallback():
    from ryolov4_amd.lib import general
    with pytest.raises(RuntimeError):
        general.post_process(torch.zeros(1, 4, 8))
    with pytest.raises(RuntimeError):
        general.nms_rotated(torch.zeros(3, 5), torch.zeros(3), 0.5)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "r-yolov4_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(d, f)
                assert "liboracle" not in src, os.path.join(d, f)
