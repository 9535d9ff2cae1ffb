"""CPU: the C-ABI library loads and exports every symbol include/pagraph_hip.h declares, and the
product fails loudly (no CPU fallback) when there is no GPU.  And the Python restatement of the ABI
(aligngraph2_amd/capi.py) is held against the headers: layouts and constants through a probe the C compiler
builds from capi itself, signatures through the headers' declarations, and nothing else in the tree restates them."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

import pagctl
from aligngraph2_amd import capi

HEADER = os.path.join(pagctl.ROOT, "include", "pagraph_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pag_[a-z_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pagctl.HIP_LIB):
        subprocess.run(["make", "-C", pagctl.ROOT, "product"], check=True, capture_output=True)
    return capi.bind(ctypes.CDLL(pagctl.HIP_LIB))


def test_header_declares_the_expected_surface():
    fns = declared_functions()
    for f in ("pag_create", "pag_destroy", "pag_reset", "pag_process", "pag_export_csr", "pag_csr_sizes",
              "pag_solid_count", "pag_last_error", "pag_device_available"):
        assert f in fns


def test_library_exports_every_declared_symbol(lib):
    for f in declared_functions():
        assert hasattr(lib, f), f"libpagraph_hip.so does not export {f}"


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    err = ctypes.c_int(0)
    codes = (ctypes.c_uint64 * 2)(8, 3)
    g = lib.pag_create(codes, 2, 8, 0, ctypes.byref(err))
    assert not g and err.value == -19, "pag_create must fail with PAG_ENODEV when no gfx950 device exists"
    # and the drop-in executable exits non-zero instead of computing anything on the CPU
    exe = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pagraph")
    r = subprocess.run([exe, "-k", "/nonexistent", "-p", "/nonexistent", "-o", "/tmp"], capture_output=True, text=True)
    assert r.returncode != 0


def test_cli_contract_without_gpu():
    exe = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pagraph")
    assert subprocess.run([exe], capture_output=True).returncode == 0          # no args: usage, exit 0
    assert subprocess.run([exe, "-h"], capture_output=True).returncode == 0     # help: exit 0
    assert subprocess.run([exe, "--bogus", "1"], capture_output=True).returncode == 1  # unknown flag: exit 1
    assert subprocess.run([exe, "-t", "abc"], capture_output=True).returncode == 1


# ---- aligngraph2_amd/capi.py against the headers -----------------------------------------------------------------------------
INCLUDE = os.path.join(pagctl.ROOT, "include")
PUBLIC_HEADERS = ("pagraph_hip.h", "pagraph_host.h")
ALL_HEADERS = PUBLIC_HEADERS + ("pagraph_debug.h",)


def header_text(names):
    """the headers without comments, preprocessor lines and the extern "C" braces"""
    text = "\n".join(open(os.path.join(INCLUDE, n)).read() for n in names)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    return re.sub(r'extern\s+"C"\s*\{|^\}\s*$', "", text, flags=re.M)


STRUCT_RE = re.compile(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*(\w+)\s*;")


def declared_structs(names):
    return STRUCT_RE.findall(header_text(names))


def c_class(decl):
    """a C parameter or result type as the class the issue's rule compares: 'ptr', 'void' or the scalar's name"""
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    return {"int32_t": "int"}.get(words[0], words[0])


def declared_signatures(names):
    """{function: (result class, [parameter classes])} of every `ret name(args);` the headers declare"""
    text = STRUCT_RE.sub("", header_text(names))
    out = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(\w+)\s*\(([^()]*)\)\s*", stmt, flags=re.S)
        if not m or m.group(1).split()[0] == "typedef":
            continue
        args = [a.strip() for a in m.group(3).split(",")]
        out[m.group(2)] = (c_class(m.group(1)), [] if args == ["void"] else [c_class(a) for a in args])
    return out


SCALARS = {ctypes.c_int: "int", ctypes.c_uint32: "uint32_t", ctypes.c_uint64: "uint64_t", ctypes.c_int64: "int64_t",
           ctypes.c_double: "double", None: "void"}


def ctypes_class(t, result=False):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (not result and isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return SCALARS.get(t, f"unexpected {t!r}")


def test_the_declaration_parser_misses_nothing():
    sigs = declared_signatures(ALL_HEADERS)
    for n in ALL_HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, n)).read(), flags=re.S)
        for f in set(re.findall(r"\b(pagh?_[a-z_0-9]+)\s*\(", text)):
            assert f in sigs, f"{n}: the parser did not find the declaration of {f}"
    assert set(declared_functions()) <= set(sigs)


def test_signatures_agree_with_the_headers():
    sigs = declared_signatures(ALL_HEADERS)
    assert sorted(capi.SIGNATURES) == sorted(sigs), \
        f"only in capi: {sorted(set(capi.SIGNATURES) - set(sigs))}; only in the headers: {sorted(set(sigs) - set(capi.SIGNATURES))}"
    for name, (c_res, c_args) in sorted(sigs.items()):
        restype, argtypes = capi.SIGNATURES[name]
        assert ctypes_class(restype, result=True) == c_res, f"{name}: result {restype!r} against the header's {c_res}"
        assert len(argtypes) == len(c_args), f"{name}: {len(argtypes)} argtypes, the header declares {len(c_args)} parameters"
        for i, (t, c) in enumerate(zip(argtypes, c_args)):
            assert ctypes_class(t) == c, f"{name}: parameter {i} is {t!r}, the header declares {c}"


def test_every_struct_of_the_headers_is_mirrored_or_excused():
    declared = declared_structs(ALL_HEADERS)  # (the test hooks' structs too: a mirror of one is held to its header like any other)
    assert len(declared) > 15, "the struct parser found too little"
    mirrored = set(capi.STRUCTS) | set(capi.DTYPES)
    for name in declared:
        assert name in mirrored or name in capi.NOT_MIRRORED, f"{name} is neither mirrored in capi.py nor listed in capi.NOT_MIRRORED"
    assert mirrored <= set(declared), f"capi.py mirrors what no header declares: {sorted(mirrored - set(declared))}"
    for name, reason in capi.NOT_MIRRORED.items():
        assert name in declared and name not in mirrored and reason.strip(), name


def mirror_layouts():
    """{C name: (size, [(field, offset, size)])} as ctypes / numpy lay the mirrors out"""
    out = {}
    for name, s in capi.STRUCTS.items():
        out[name] = (ctypes.sizeof(s), [(f[0], getattr(s, f[0]).offset, getattr(s, f[0]).size) for f in s._fields_])
    for name, dt in capi.DTYPES.items():
        out[name] = (dt.itemsize, [(f, dt.fields[f][1], dt.fields[f][0].itemsize) for f in dt.names])
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """sizes, offsets and constants as the C compiler sees the headers, from a program generated from capi itself"""
    d = tmp_path_factory.mktemp("abi_probe")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "pagraph_host.h"', '#include "pagraph_debug.h"', "int main(void) {"]
    for name, (_, fields) in mirror_layouts().items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        for f, _, _ in fields:
            lines.append(f'    printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));')
    for name in capi.CONSTANTS:
        lines.append(f'    printf("C {name} %lld\\n", (long long)({name}));')
    lines += ["    return 0;", "}"]
    src = d / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-o", str(d / "probe")], capture_output=True, text=True)
    assert r.returncode == 0, "capi.py names a struct, field or constant the headers do not have:\n" + r.stderr[-3000:]
    sizes, fields, consts = {}, {}, {}
    for ln in subprocess.run([str(d / "probe")], capture_output=True, text=True, check=True).stdout.splitlines():
        p = ln.split()
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            fields[(p[1], p[2])] = (int(p[3]), int(p[4]))
        else:
            consts[p[1]] = int(p[2])
    return sizes, fields, consts


@pytest.mark.parametrize("name", sorted(capi.STRUCTS) + sorted(capi.DTYPES))
def test_mirror_has_the_layout_of_the_header_s_struct(name, probe):
    sizes, fields, _ = probe
    size, mine = mirror_layouts()[name]
    for f, off, sz in mine:
        assert (off, sz) == fields[(name, f)], f"{name}.{f}: offset / size {(off, sz)} in capi.py, {fields[(name, f)]} in the header"
    assert size == sizes[name], f"{name}: {size} bytes in capi.py, {sizes[name]} in the header (a field is missing or padded differently)"


def test_constants_have_the_header_s_values(probe):
    _, _, consts = probe
    for name, value in capi.CONSTANTS.items():
        assert getattr(capi, name) == value == consts[name], f"{name}: {value} in capi.py, {consts[name]} in the header"


def test_nothing_else_restates_the_abi():
    """outside capi.py no file types a function of the table or defines a Structure with the fields of a mirrored struct"""
    files = [f for d in ("aligngraph2_amd", "tests") for f in glob.glob(os.path.join(pagctl.ROOT, d, "*.py")) if os.path.basename(f) != "capi.py"]
    assert len(files) > 40
    fieldsets = {tuple(f[0] for f in s._fields_): n for n, s in capi.STRUCTS.items()}
    for path in files:
        src = open(path).read()
        for fn, attr in re.findall(r"\b(\w+)\.(argtypes|restype)\s*=(?!=)", src):
            assert fn not in capi.SIGNATURES, f"{path} assigns {fn}.{attr}: the signature belongs to capi.SIGNATURES alone"
        for node in ast.walk(ast.parse(src, path)):
            if not isinstance(node, ast.ClassDef) or not any("Structure" in ast.unparse(b) for b in node.bases):
                continue
            for st in node.body:
                if isinstance(st, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "_fields_" for t in st.targets):
                    names = tuple(e.elts[0].value for e in getattr(st.value, "elts", []) if isinstance(e, ast.Tuple) and isinstance(e.elts[0], ast.Constant))
                    assert names not in fieldsets, f"{path}: class {node.name} restates {fieldsets.get(names)} (import it from capi)"
