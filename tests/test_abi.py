"""CPU checks of the drop-in boundary: the C-ABI library loads without a GPU, exports every symbol that
include/coslam_hip.h declares, refuses to run without a device (no CPU fallback), and the C++ shim header
compiles against it."""
import ctypes as C
import os
import re
import subprocess

import pytest

import coslam_amd
from coslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "coslam_hip.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = coslam_amd.lib()
    syms = declared_symbols()
    assert len(syms) >= 40
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.cs_version() >= 100


def test_klt_config_defaults_match_the_reference():
    from coslam_amd.klt import KLT_SequenceTrackerConfig

    cfg = KLT_SequenceTrackerConfig()  # defaults of v3d_gpuklt.h:181-191
    assert (cfg.nIterations, cfg.nLevels, cfg.levelSkip, cfg.windowWidth) == (12, 3, 2, 5)
    assert cfg.minDistance == 8 and cfg.trackWithGain == 0 and abs(cfg.SSD_Threshold - 5000.0) < 1e-6
    lib = coslam_amd.lib()
    d = KLT_SequenceTrackerConfig()
    d.nIterations = 0
    lib.cs_klt_config_default(C.byref(d))
    assert d.as_dict() == cfg.as_dict()


# ---- the mirrors: every ctypes Structure and numpy record type of the package against the compiler's layout of its C type ----------------

def header_structs():
    """{cs_x: [member names in order]} of every `typedef struct ... { ... } cs_x;` of the header (the bodies are flat)"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(cs_\w+)\s*;", _lib.header_text()):
        out[name] = [re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", d.strip()).group(1)
                     for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    return out


def compiler_layouts(tmp_path):
    """{cs_x: (sizeof, [(member, offsetof, sizeof)])} as the host compiler lays the header's structs out"""
    structs = header_structs()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "coslam_hip.h"', "int main(void) {"]
    for name, members in structs.items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("M {name} {m} %zu %zu\\n", offsetof({name}, {m}), sizeof((({name}*)0)->{m}));' for m in members]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout_probe.c", tmp_path / "layout_probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        f = ln.split()
        if f[0] == "S":
            out[f[1]] = (int(f[2]), [])
        else:
            out[f[1]][1].append((f[2], int(f[3]), int(f[4])))
    assert set(out) == set(structs) and len(out) >= 39
    return out


def package_mirrors():
    """[(python name, C type or None, sizeof, [(field, offset, size)])] of every Structure subclass and every numpy record type (a dtype
    with named fields held by a module) under coslam_amd/"""
    import importlib
    import pkgutil

    import numpy as np

    mods = [importlib.import_module("coslam_amd." + m.name) for m in pkgutil.iter_modules(coslam_amd.__path__)]
    out, todo, seen = [], list(C.Structure.__subclasses__()), set()
    while todo:
        cls = todo.pop()
        todo += cls.__subclasses__()
        if cls.__module__.split(".")[0] == "coslam_amd" and cls not in seen:
            seen.add(cls)
            fields = [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
            out.append((f"{cls.__module__}.{cls.__name__}", cls.__dict__.get("_c_type_"), C.sizeof(cls), fields))
    links = {id(getattr(m, k)): v for m in mods for k, v in getattr(m, "C_RECORD_TYPES", {}).items()}
    records = {}
    for m in mods:   # (a record type imported into other modules is one mirror, under the name of the module that links it)
        for k, v in vars(m).items():
            if isinstance(v, np.dtype) and v.names and (id(v) not in records or k in getattr(m, "C_RECORD_TYPES", {})):
                records[id(v)] = (f"{m.__name__}.{k}", v)
    for key, (name, dt) in records.items():
        out.append((name, links.get(key), dt.itemsize, [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names]))
    return sorted(out)


def test_every_mirror_names_its_c_type_and_matches_the_compilers_layout(tmp_path):
    """One table: every mirror has a link to its C type (Structure: the class attribute _c_type_; numpy record type: the module's
    C_RECORD_TYPES), and sizeof and, position by position, every member's offset and size are the host compiler's.  A field named
    differently from its C member is listed in the failure message and is no failure by itself."""
    want = compiler_layouts(tmp_path)
    mirrors = package_mirrors()
    assert len(mirrors) >= 35, [m[0] for m in mirrors]
    bad, renamed = [], []
    for name, ctype, size, fields in mirrors:
        if ctype is None:
            bad.append(f"{name}: no link to a C type")
        elif ctype not in want:
            bad.append(f"{name}: {ctype} is not a struct of include/coslam_hip.h")
        else:
            csize, members = want[ctype]
            if size != csize:
                bad.append(f"{name}: sizeof {size}, {ctype} has {csize}")
            if [f[1:] for f in fields] != [m[1:] for m in members]:
                bad.append(f"{name}: (offset, size) {[f[1:] for f in fields]}, {ctype} has {[m[1:] for m in members]}")
            renamed += [f"{name}.{f[0]} is {ctype}.{m[0]}" for f, m in zip(fields, members) if f[0] != m[0]]
    assert not bad, "\n".join(bad + ["fields named differently from their C members:"] + renamed)


# ---- the declaration: restype / argtypes of every function come from the header (coslam_amd/_lib.py) ------------------------------------

def header_prototypes():
    """{name: (result text, [parameter texts])}, read from the header independently of the loader's mapper"""
    txt = re.sub(r"\{[^{}]*\}", "", _lib.header_text())
    out = {}
    for res, name, params in re.findall(r"([\w\s\*]+?)\b(cs_\w+)\s*\(([^()]*)\)\s*;", txt):
        params = " ".join(params.split())
        out[name] = (" ".join(res.split()), [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


def test_every_declared_function_is_typed_from_the_header():
    lib = coslam_amd.lib()
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols() and len(protos) >= 285
    scalar_results = {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong, "double": C.c_double, "void": None}
    n_ptr_results = 0
    for name, (res, params) in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == len(params), name
        for i, p in enumerate(params):
            is_pointer = "*" in p or "[" in p or p.split()[0] == "cs_ba_followup_fn"
            assert (f.argtypes[i] is C.c_void_p) == is_pointer, (name, i, p, f.argtypes[i])
        if "*" in res:
            n_ptr_results += 1
            assert f.restype is (C.c_char_p if res == "const char*" else C.c_void_p), (name, res, f.restype)
        else:
            assert f.restype is scalar_results[res], (name, res, f.restype)
    assert n_ptr_results >= 21
    assert len(lib.cs_register_revisit_rounds_dev.argtypes) == 36 and len(lib.cs_version.argtypes) == 0
    assert lib.cs_pinned_alloc.restype is C.c_void_p and lib.cs_pinned_alloc.argtypes == [C.c_size_t]
    assert lib.cs_ba_completed.restype is C.c_longlong and lib.cs_newpts_scratch_bytes.restype is C.c_size_t
    assert lib.cs_last_error.restype is C.c_char_p and lib.cs_klt_config_default.restype is None
    with pytest.raises(C.ArgumentError):   # a numpy scalar as a pointer: refused before the call
        import numpy as np

        lib.cs_klt_destroy(np.int64(0))
    with pytest.raises(TypeError):         # one argument short
        getattr(lib, "cs_klt_set_fused")(None)


def test_an_unknown_parameter_type_is_an_error_that_names_the_function(tmp_path, monkeypatch):
    hdr = tmp_path / "coslam_hip.h"
    hdr.write_text("/* a comment */\nint cs_fine(const double* a, int n);\nint cs_odd(short n);\n")
    monkeypatch.setattr(_lib, "HEADER_PATH", str(hdr))
    with pytest.raises(coslam_amd.CoslamHipError, match="cs_odd"):
        _lib.declarations()
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "missing.h"))
    with pytest.raises(coslam_amd.CoslamHipError, match="missing.h"):
        _lib.declarations()


def python_sources():
    for sub in ("coslam_amd", "tests", "tools"):
        for f in sorted(os.listdir(os.path.join(ROOT, sub))):
            if f.endswith(".py"):
                yield os.path.join(sub, f)


def test_every_direct_call_passes_the_declared_number_of_arguments():
    """Every `<expr>.cs_name(...)` under coslam_amd/, tests/ and tools/*.py: as many positional arguments as the header declares and no
    keywords.  Calls with a starred argument and calls through an alias (f = lib().cs_name) cannot be judged here: counted and printed."""
    import ast

    protos = header_prototypes()
    calls, starred, aliases, bad = 0, [], [], []
    for path in python_sources():
        for node in ast.walk(ast.parse(open(os.path.join(ROOT, path)).read())):
            if isinstance(node, ast.Assign) and isinstance(node.value, ast.Attribute) and node.value.attr in protos:
                aliases.append(f"{path}:{node.lineno} {node.value.attr}")
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in protos):
                continue
            calls += 1
            where = f"{path}:{node.lineno} {node.func.attr}"
            if node.keywords:
                bad.append(where + ": keyword arguments")
            if any(isinstance(a, ast.Starred) for a in node.args):
                starred.append(where)
            elif len(node.args) != len(protos[node.func.attr][1]):
                bad.append(where + f": {len(node.args)} arguments, the header declares {len(protos[node.func.attr][1])}")
    print(f"{calls} direct calls, {len(starred)} starred {starred}, {len(aliases)} aliases {aliases}")
    assert not bad, bad
    assert calls >= 289, calls   # the walk sees the calls: 289 before the declaration moved into coslam_amd/_lib.py


def test_only_the_loader_declares_prototypes():
    """The header is the only declaration: no module of the package but _lib.py sets .argtypes or .restype."""
    pkg = os.path.join(ROOT, "coslam_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py") and f != "_lib.py":
            src = open(os.path.join(pkg, f)).read()
            for pat in (".argtypes", ".restype"):
                assert pat not in src, (f, pat)


def test_a_bare_address_reaches_the_library_whole():
    """cs_merge_match_fmat (host code only: two 3 x 3 inverses and two products) called with the bare integer addresses of numpy buffers,
    which do not fit 32 bits: F = iK1^T E^T iK2 as numpy has it.  In a child process: a truncated pointer would be a crash of the child."""
    import sys

    code = """
import numpy as np, coslam_amd
rng = np.random.default_rng(5)
K1 = np.array([[520.0, 0.0, 321.5], [0.0, 515.0, 238.0], [0.0, 0.0, 1.0]])
K2 = np.array([[610.0, 0.0, 300.0], [0.0, 605.0, 250.5], [0.0, 0.0, 1.0]])
E, F = rng.normal(size=(3, 3)), np.zeros((3, 3))
addr = [a.ctypes.data for a in (K1, K2, E, F)]
assert all(type(a) is int for a in addr) and min(addr) >= 2 ** 32, addr
assert coslam_amd.lib().cs_merge_match_fmat(*addr) == 0
want = np.linalg.inv(K1).T @ E.T @ np.linalg.inv(K2)
# both sides binary64; cond(K) ~ 1e3, so the inverses and the two products agree to ~1e3 eps relative to the largest entry
assert np.max(np.abs(F - want)) <= 1e-12 * np.max(np.abs(want)), (F, want)
print("fmat ok")
"""
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fmat ok" in out.stdout, out.stdout + out.stderr


def test_no_device_means_loud_failure_not_cpu_fallback():
    lib = coslam_amd.lib()
    if lib.cs_device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(coslam_amd.CoslamHipError):
        coslam_amd.KLT_SequenceTracker(coslam_amd.KLT_SequenceTrackerConfig(), device=0)
    import numpy as np

    with pytest.raises(coslam_amd.CoslamHipError):
        coslam_amd.intraCamEstimate(np.eye(3), np.eye(3), np.zeros(3), 4, None, np.ones((4, 3)), np.ones((4, 2)), 10.0)
    with pytest.raises(coslam_amd.CoslamHipError):
        coslam_amd.bundleAdjustRobust(0, np.eye(3)[None], np.eye(3)[None].copy(), np.zeros((1, 3)), 0, np.ones((1, 3)),
                                      [[(0, 1.0, 1.0)]], 6.0, 1, 1)


def test_product_package_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under coslam_amd/ may import, include, link or load it."""
    pkg = os.path.join(ROOT, "coslam_amd")
    banned = ("import oracle", "from oracle", "liboracle", "libintracam_ref", "oracle.h\"", "_oracle.c")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                for pat in banned:
                    assert pat not in src, (f, pat)


def test_cxx_shim_compiles_and_links():
    """include/v3d_gpuklt.h + SL_IntraCamPose.h + SL_BundleAdjust.h: the reference's C++ signatures over the C-ABI."""
    src = os.path.join(ROOT, "tests", "cxx", "shim_link_test.cpp")
    exe = os.path.join(ROOT, "tests", "cxx", "shim_link_test.bin")
    libdir = os.path.join(ROOT, "coslam_amd", "lib")
    cmd = ["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "shim"), src,
           "-L", libdir, "-lcoslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
           "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shim ok" in out.stdout


def test_cxx_dropin_bench_compiles():
    """tools/cxx/dropin_bench.cpp (latency of the reference-shaped synchronous calls) builds against the shims."""
    src = os.path.join(ROOT, "tools", "cxx", "dropin_bench.cpp")
    exe = os.path.join(ROOT, "tools", "cxx", "dropin_bench.bin")
    libdir = os.path.join(ROOT, "coslam_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "shim"),
           src, "-L", libdir, "-lcoslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
           "-o", exe]
    subprocess.check_call(cmd)
    assert os.path.exists(exe)
