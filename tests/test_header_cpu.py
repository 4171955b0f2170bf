"""imcui_hip/header.py, the reader of include/imcui_hip.h that the ctypes signatures and the descriptor classes come from: its result on
the declaration shapes that can go wrong against signatures typed in here by hand, its refusals, and the struct layouts against what a
C compiler makes of the same header."""
import ctypes as C
import os
import subprocess

import pytest

from imcui_hip import header

P = C.c_void_p
EXPECTED = {  # typed from the header by hand, independent of the reader
    "imcui_hip_create": (C.c_int, [C.c_int, P]),  # imcui_hip_t**
    "imcui_hip_destroy": (None, [P]),
    "imcui_hip_last_error": (C.c_char_p, [P]),
    "imcui_hip_version": (C.c_int, []),  # (void)
    "imcui_hip_set_option": (C.c_int, [P, C.c_char_p, C.c_int]),
    "imcui_hip_ffn_pack_w2": (C.c_float, [P, P, P]),
    "imcui_hip_ffn_set_debug": (C.c_int, [P, P]),  # long long*
    "imcui_hip_mutual_nn_dn": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, P, P, P, C.c_size_t, P]),
    "imcui_hip_superpoint_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "imcui_hip_sfd2_forward": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P,
                                         C.c_int, P, P, C.c_size_t, P]),  # fmt: skip
    "imcui_hip_png_reconstruct_batch": (C.c_int, [P, P, P, P, P, C.c_int, P, P, P, C.c_size_t, P]),  # const size_t*, unsigned char*
    "imcui_hip_select_probe": (C.c_int, [P, P, P]),  # const imcui_hip_select_desc*
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_reader_gives_the_hand_written_signature(name):
    assert header.read().functions[name] == EXPECTED[name]


def test_reader_gives_the_defines():
    d = header.read().defines
    assert (d["IMCUI_HIP_OK"], d["IMCUI_HIP_ERR_ARG"], d["IMCUI_HIP_ERR_WS"], d["IMCUI_HIP_ERR_HIP"], d["IMCUI_HIP_ERR_UNSUPPORTED"]) == (0, -1, -2, -3, -4)
    assert d["IMCUI_SELECT_MAXB"] == 8


GOOD = """
typedef struct imcui_hip_s imcui_hip_t;
/* imcui_hip_foo(...) is only talked about here */
int imcui_hip_one(imcui_hip_t* h, const float* const* w,
                  size_t n);  // and imcui_hip_bar(1) here
const char* imcui_hip_two(void);
"""
BAD = {
    "unknown type": ("int imcui_hip_a(widget_t w);", "widget_t"),
    "unknown pointee": ("int imcui_hip_a(const widget_t* w);", "widget_t"),
    "function pointer": ("int imcui_hip_a(void (*cb)(int), int n);", "imcui_hip_a"),
    "unnamed value": ("int imcui_hip_a(int, float x);", "unnamed"),
    "unnamed two-word value": ("int imcui_hip_a(long long);", "unnamed"),
    "unnamed pointer": ("int imcui_hip_a(const float*);", "const float*"),
    "cut off at the end": ("int imcui_hip_a(int x);\nint imcui_hip_b(int y)", "imcui_hip_b"),
    "cut off in the middle": ("int imcui_hip_a(int x)\nint imcui_hip_b(int y);", "imcui_hip_a"),
    "cut off inside the list": ("int imcui_hip_a(int x, \nint imcui_hip_b(int y);", "imcui_hip_a"),
    "declared twice": ("int imcui_hip_a(int x);\nint imcui_hip_a(int x);", "twice"),
    "empty list": ("int imcui_hip_a();", "(void)"),
    "void by value": ("int imcui_hip_a(void v);", "void"),
    "struct by value": ("typedef struct s { int a; } s_t;\nint imcui_hip_a(s_t d);", "s_t"),
    "array size": ("typedef struct s { int a[N]; } s_t;", "N"),
    "bit field": ("typedef struct s { int a : 3; } s_t;", "a : 3"),
    "function pointer field": ("typedef struct s { int (*f)(int); } s_t;", "s_t"),
    "other statement": ("int imcui_hip_a(int x);\nextern int counter;", "counter"),
}


def test_reader_keeps_exactly_the_declarations():
    h = header.parse(GOOD)
    assert h.functions == {"imcui_hip_one": (C.c_int, [P, P, C.c_size_t]), "imcui_hip_two": (C.c_char_p, [])}


@pytest.mark.parametrize("case", sorted(BAD))
def test_reader_refuses(case):
    text, offending = BAD[case]
    with pytest.raises(header.HeaderError) as e:
        header.parse(text)
    assert offending in str(e.value), str(e.value)


def test_reader_reads_struct_declarators():
    text = "#define N 3\ntypedef struct s { int M, N2, K; const float* A; long a_bs, *p, w_bs; unsigned long long k[N]; float v[2]; } s_t;"
    assert header.parse(text).structs["s_t"] == [("M", C.c_int), ("N2", C.c_int), ("K", C.c_int), ("A", P), ("a_bs", C.c_long), ("p", P), ("w_bs", C.c_long),
                                                  ("k", C.c_ulonglong * 3), ("v", C.c_float * 2)]  # fmt: skip


def _compile(src, exe):
    """With $CC, else cc, else the clang next to hipcc; the first that produces the program."""
    from imcui_hip.build import HIPCC, INCLUDE

    tried = []
    for cc in filter(None, (os.environ.get("CC"), "cc", os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "clang"))):
        try:
            r = subprocess.run([*cc.split(), "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
        except OSError as e:
            tried.append(f"{cc}: {e}")
            continue
        if r.returncode == 0:
            return
        tried.append(f"{cc}: {r.stderr[-400:]}")
    pytest.fail("no C compiler built the layout program:\n" + "\n".join(tried))


def test_descriptor_layouts_match_the_c_compiler(tmp_path):
    """sizeof, and offsetof / size of every field, of the five descriptor structs as a C compiler lays the header out, against the ctypes
    classes of backend (field names from the parsed structs, `inp` back to `in`)."""
    from imcui_hip import backend

    classes = {"imcui_hip_gemm_desc": backend.GemmDesc, "imcui_hip_attn_desc": backend.AttnDesc, "imcui_hip_conv_desc": backend.ConvDesc,
               "imcui_hip_ffn_desc": backend.FfnDesc, "imcui_hip_select_desc": backend.SelectDesc}  # fmt: skip
    structs = header.read().structs
    assert set(structs) == set(classes)
    lines = []
    for s, fields in structs.items():
        lines.append(f'printf("{s} . %zu 0\\n", sizeof({s}));')
        lines += [f'printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f, _ in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "imcui_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    _compile(src, tmp_path / "layout")
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        s, f, a, b = line.split()
        cls = classes[s]
        if f == ".":
            assert C.sizeof(cls) == int(a), s
        else:
            d = getattr(cls, backend.PY_FIELD_NAMES.get(f, f))
            assert (d.offset, d.size) == (int(a), int(b)), (s, f)
            seen += 1
    assert seen == sum(len(c._fields_) for c in classes.values()) and len(out.splitlines()) == seen + len(classes)
    assert "inp" in dict(backend.ConvDesc._fields_) and "in" not in dict(backend.ConvDesc._fields_)
