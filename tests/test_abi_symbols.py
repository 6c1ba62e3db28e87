"""The ctypes ABI table matches the built HIP library and the Python call sites.

A renamed or removed ``extern "C"`` entry point would otherwise be skipped silently by
``_abi.declare`` and only fail as an AttributeError on the GPU box.  Loading the library needs
no GPU (the HIP runtime initialises lazily), so this runs in the CPU suite.  The signatures themselves are
compared with the `extern "C"` definitions parsed from the kernel sources (no library needed).
"""
import ctypes
import pathlib
import re

import pytest

from biscotti_amd import native
from biscotti_amd.ops import _abi

_ROOT = pathlib.Path(__file__).resolve().parent.parent


def _python_call_sites():
    names = set()
    files = list((_ROOT / "biscotti_amd").rglob("*.py")) + [_ROOT / "bench.py"]
    for p in files:
        names |= set(re.findall(r"\b(bsc_[a-z0-9_]+)\b", p.read_text()))
    return names


def test_every_python_call_site_is_declared():
    undeclared = sorted(_python_call_sites() - set(_abi.SIGNATURES))
    assert not undeclared, f"bsc_* symbols used from Python without a ctypes signature: {undeclared}"


def test_every_declared_symbol_is_exported():
    path = native.hip_library_path()
    if not path.exists():
        pytest.skip("libbiscotti_hip.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(path))
    missing = sorted(n for n in _abi.SIGNATURES if not hasattr(lib, n))
    assert not missing, f"declared in _abi.SIGNATURES but not exported by {path.name}: {missing}"


_KERNELS = _ROOT / "biscotti_amd" / "csrc" / "kernels"
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "void*": ctypes.c_void_p, "void": None}


def _strip_comments(text):
    return re.sub(r"//[^\n]*|/\*.*?\*/", " ", text, flags=re.S)


def _ctype_of(param):
    """The ctypes class of one C parameter declaration (`const uint32_t* pts`); KeyError on an unknown type."""
    ctype = " ".join(re.sub(r"\w+\s*$", "", param.strip()).replace("*", " * ").split())   # the name dropped
    if "*" in ctype:
        return ctypes.c_char_p if ctype == "const char *" else ctypes.c_void_p
    return _SCALARS[ctype]


def _c_definitions():
    """name -> (argument classes, return class, file) of every `extern "C"` bsc_* definition in kernels/*.hip."""
    defs = {}
    for p in sorted(_KERNELS.glob("*.hip")):
        for ret, name, params in re.findall(r'extern\s+"C"\s+([\w\s*]+?)\s*\b(bsc_\w+)\s*\(([^)]*)\)\s*\{',
                                            _strip_comments(p.read_text())):
            assert name not in defs, f"{name} is defined in {defs[name][2]} and in {p.name}"
            params = [] if params.strip() in ("", "void") else params.split(",")
            defs[name] = ([_ctype_of(a) for a in params], _RETURNS["".join(ret.split())], p.name)
    return defs


def _names(classes):
    return [getattr(c, "__name__", c) for c in classes]


def test_ctypes_table_matches_the_c_definitions():
    """Every entry of _abi.SIGNATURES against the parsed C definition: argument count, the class at every
    position, the return type.  An `int` declared where the C side takes `long long`, or a dropped argument,
    would otherwise misplace arguments silently at the first call."""
    defs = _c_definitions()
    assert len(defs) > 80, f"parsed only {len(defs)} definitions: the pattern no longer matches the sources"
    bad = []
    for name, args in _abi.SIGNATURES.items():
        if name not in defs:
            bad.append(f"{name}: no extern \"C\" definition in kernels/*.hip")
            continue
        c_args, c_ret, where = defs[name]
        if len(args) != len(c_args):
            bad.append(f"{name} ({where}): {len(args)} arguments declared, the definition takes {len(c_args)}")
        else:
            bad += [f"{name} ({where}): argument {i} is declared {a.__name__}, the definition takes {b.__name__}"
                    for i, (a, b) in enumerate(zip(args, c_args)) if a is not b]
        ret = _abi.RESTYPES.get(name, ctypes.c_int)
        if ret is not c_ret:
            bad.append(f"{name} ({where}): returns {_names([c_ret])[0]}, declared {_names([ret])[0]}")
    assert not bad, "\n".join(bad)


def test_every_export_is_reachable():
    """An `extern "C"` bsc_* definition is either callable from Python (_abi.SIGNATURES) or called from another
    kernel file (declared in launchers.h, which covers the macro-generated wave priority setters too)."""
    cross_file = set(re.findall(r"\b(bsc_\w+)\s*\(", _strip_comments((_KERNELS / "launchers.h").read_text())))
    orphans = sorted(set(_c_definitions()) - set(_abi.SIGNATURES) - cross_file)
    assert not orphans, f"exported but neither in _abi.SIGNATURES nor in launchers.h: {orphans}"


def test_no_static_device_variables_in_kernels():
    """A `static __device__`/`__constant__` variable that the host addresses is externalised with default
    visibility and read through the GOT (two dependent scalar loads per kernel entry, measured ~0.04 ms/round on
    the wave-priority flags); kernel files use externally linked, per-file names instead (wave_prio.h)."""
    bad = []
    for p in sorted((_ROOT / "biscotti_amd" / "csrc" / "kernels").glob("*")):
        if p.suffix in (".hip", ".h", ".hpp"):
            for i, line in enumerate(p.read_text().splitlines(), 1):
                if re.search(r"\bstatic\s+__(device|constant)__\s+(?!__forceinline__|inline)[\w:<>]+\s+\w+\s*[=;\[]",
                             line):
                    bad.append(f"{p.name}:{i}: {line.strip()}")
    assert not bad, bad
