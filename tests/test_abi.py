"""CPU-side checks of the binding that retr_amd._lib derives from include/retr_hip.h: struct
layouts against a real C compiler, the header parser's corner cases, and the named tuning knobs
(retr_tune is host-only state, so these need no GPU)."""
import ctypes
import glob
import os
import shutil
import subprocess

import pytest

from retr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_c_compiler():
    """`cc` (or gcc / clang) from PATH, else the clang that ships with ROCm (the one hipcc
    drives, so it exists wherever the library was built)."""
    for name in ("cc", "gcc", "clang"):
        path = shutil.which(name)
        if path:
            return path
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = sorted(glob.glob(os.path.join(rocm, "llvm", "bin", "clang")) +
                   glob.glob(os.path.join(rocm, "lib", "llvm", "bin", "clang")))
    assert found, "no host C compiler: neither cc / gcc / clang on PATH nor ROCm's clang"
    return found[0]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every field's offsetof, as a C compiler lays out the header's structs, equal
    ctypes.sizeof and Struct.<field>.offset of the generated classes (multi-declarators such as
    `int M, N, K, relu;` and arrays such as `float f[3];` included)."""
    assert len(_lib.STRUCTS) == 11
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "retr_hip.h"',
             'int main(void) {']
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([host_c_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}
    want = {}
    for name, cls in _lib.STRUCTS.items():
        want[(name, "sizeof")] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            want[(name, field)] = getattr(cls, field).offset
    assert len(want) == 11 + 135              # 11 structs and their 135 fields, counted by hand
    assert got == want


def test_public_struct_names_are_the_generated_classes():
    for alias, name in [("LinearFwdDesc", "retr_linear_fwd_desc"),
                        ("LinearDgradDesc", "retr_linear_dgrad_desc"),
                        ("LinearWgradDesc", "retr_linear_wgrad_desc"),
                        ("ConvWgradDesc", "retr_conv_wgrad_desc"),
                        ("ConvUnpackDesc", "retr_conv_unpack_desc"),
                        ("PosItem", "retr_pos_item"), ("LnOut", "retr_ln_out"),
                        ("ConvPackDesc", "retr_conv_pack_desc"),
                        ("CatRowsDesc", "retr_cat_rows_desc"),
                        ("SlabSumDesc", "retr_slab_sum_desc"), ("PipeItem", "retr_pipe_item")]:
        assert getattr(_lib, alias) is _lib.STRUCTS[name]
    assert (_lib.F32, _lib.BF16) == (0, 1)
    restype, params = _lib.FUNCTIONS["retr_pipe_run"]
    assert restype is ctypes.c_int and params[1] == ("items", ctypes.POINTER(_lib.PipeItem))
    assert _lib.FUNCTIONS["retr_linear_wgrad_group_workspace"][0] is ctypes.c_size_t
    assert _lib.FUNCTIONS["retr_set_seed_base"][0] is None


CORNER_CASES = """
/* a comment with a prototype in it: int not_a_function(int x); */
#ifndef T_H
#define T_H
#define T_DTYPE_BF16 1
#define T_MASK 0x10
typedef struct {
  const float *a, *b;   /* two pointers in one declaration */
  int M, N; long ld; float f[3];
  unsigned long long seed; size_t bytes;
} t_desc;
typedef struct t_item { const void* d; double w; long long n; int pad_[2]; } t_item;
enum { T_TUNE_A = 0, T_TUNE_B = 7, T_TUNE_C, T_TUNE_COUNT = 40 };
const char* t_last_error(void);
size_t t_workspace(int n,
                   const t_desc* d,   // a line comment
                   t_item* items);
void t_set(const unsigned long long* p, float v, const unsigned char* mask, void* stream);
#endif
"""


def test_parser_corner_cases():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    functions, structs, constants = _lib.parse_header(CORNER_CASES)
    desc, item = structs["t_desc"], structs["t_item"]
    assert list(structs) == ["t_desc", "t_item"]
    assert desc._fields_ == [("a", P), ("b", P), ("M", I), ("N", I), ("ld", L), ("f", F * 3),
                             ("seed", ctypes.c_ulonglong), ("bytes", ctypes.c_size_t)]
    assert item._fields_ == [("d", P), ("w", ctypes.c_double), ("n", ctypes.c_longlong),
                             ("pad_", I * 2)]
    assert ctypes.sizeof(desc) == 64 and desc.f.offset == 32 and desc.seed.offset == 48
    assert ctypes.sizeof(item) == 32 and item.pad_.offset == 24
    assert list(functions) == ["t_last_error", "t_workspace", "t_set"]
    assert functions["t_last_error"] == (ctypes.c_char_p, [])
    assert functions["t_workspace"] == (ctypes.c_size_t, [
        ("n", I), ("d", ctypes.POINTER(desc)), ("items", ctypes.POINTER(item))])
    assert functions["t_set"] == (None, [("p", P), ("v", F), ("mask", P), ("stream", P)])
    assert constants == {"T_DTYPE_BF16": 1, "T_MASK": 16, "T_TUNE_A": 0, "T_TUNE_B": 7,
                         "T_TUNE_C": 8, "T_TUNE_COUNT": 40}


@pytest.mark.parametrize("decl,named", [
    ("int t_f(short x);", "short"),                          # never a silent int
    ("typedef struct { int a; uint64_t b; } t_s;", "uint64_t"),
    ("bool t_g(void);", "bool"),
    ("int t_h(const t_unknown* d);", "t_unknown"),           # a struct the header does not declare
    ("int t_k(int x) { return x; }", "t_k"),                 # not a declaration we know
])
def test_parser_rejects_what_it_does_not_know(decl, named):
    with pytest.raises(RuntimeError, match=named):
        _lib.parse_header("int t_ok(int a);\n" + decl + "\n")


def test_missing_header_is_a_clear_error(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "retr_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", missing)
    with pytest.raises(RuntimeError, match="retr_hip.h"):
        _lib._read_header()


def test_tune_table_and_scoped_knobs():
    """TUNE is the header's enum by name; tuned() sets its knobs for the block and puts back
    what they held before, also when the block raises or another tuned() block encloses it."""
    count = _lib.CONSTANTS["RETR_TUNE_COUNT"]
    assert "COUNT" not in _lib.TUNE
    assert _lib.TUNE["ATTN_MODE"] == 5 and _lib.TUNE["WGRAD_TILE"] == 2
    assert len(set(_lib.TUNE.values())) == len(_lib.TUNE) == 34
    assert all(0 <= n < count for n in _lib.TUNE.values())

    def get(name):                 # retr_tune returns the previous value: read = set twice
        v = _lib.tune(name, 0)
        _lib.tune(name, v)
        return v

    before = {n: get(n) for n in ("ATTN_MODE", "ATTN_SPLIT", "WGRAD_TILE")}
    with _lib.tuned(ATTN_MODE=2, ATTN_SPLIT=1):
        assert (get("ATTN_MODE"), get("ATTN_SPLIT")) == (2, 1)
    assert {n: get(n) for n in before} == before
    with pytest.raises(ZeroDivisionError):
        with _lib.tuned(ATTN_MODE=2, ATTN_SPLIT=1):
            assert (get("ATTN_MODE"), get("ATTN_SPLIT")) == (2, 1)
            1 / 0
    assert {n: get(n) for n in before} == before
    with _lib.tuned(ATTN_MODE=1):
        with _lib.tuned(ATTN_MODE=2, ATTN_SPLIT=4):
            assert (get("ATTN_MODE"), get("ATTN_SPLIT")) == (2, 4)
        assert (get("ATTN_MODE"), get("ATTN_SPLIT")) == (1, before["ATTN_SPLIT"])
    assert {n: get(n) for n in before} == before
    with pytest.raises(KeyError, match="ATTN_MODE"):      # the message lists the valid names
        _lib.tune("NOPE", 1)
    with pytest.raises(KeyError):
        with _lib.tuned(ATTN_SPLIT=3, NOPE=1):
            pass
    assert {n: get(n) for n in before} == before           # ATTN_SPLIT was put back
