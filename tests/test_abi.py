"""The C ABI: pings_amd/_abi.py mirrors include/pings_hip.h, and the library loads and exports every symbol it declares.

The mirror checks read the header with tests/abi_header.py and need neither a GPU nor the built library.
"""
import ctypes
import re
import shutil
import subprocess

import pytest

import abi_header as hdr
from pings_amd import _abi, _lib

# C scalar -> the ctypes type a binding must pass it as (int and int32_t are the same ctypes type on every target)
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
RETURNS = {**SCALARS, "const char*": ctypes.c_char_p}


def _mirrors():
    """{C typedef: ctypes mirror} of every struct in _abi; `RasterSettings` mirrors `pings_raster_settings`."""
    return {"pings_" + re.sub(r"(?<!^)(?=[A-Z])", "_", v.__name__).lower(): v for v in vars(_abi).values()
            if isinstance(v, type) and issubclass(v, ctypes.Structure)}


def test_header_declares_symbols():
    names = hdr.header_symbols()
    assert "pings_abi_version" in names and "pings_ssim_forward" in names
    assert len(names) == len(set(names))


def test_signatures_declare_exactly_the_header_symbols():
    assert sorted(_abi.SIGNATURES) == sorted(hdr.header_symbols())


def test_signatures_match_the_header_prototypes():
    mirrors = _mirrors()
    bad = []
    for name, (ret, params) in hdr.prototypes().items():
        restype, argtypes = _abi.SIGNATURES[name]
        if restype is not RETURNS.get(ret):
            bad.append(f"{name}: returns {ret}, restype {restype.__name__}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters, {len(argtypes)} argtypes")
            continue
        for (ctype, pname), t in zip(params, argtypes):
            struct = re.fullmatch(r"const (pings_\w+)\*", ctype)
            if "*" not in ctype:
                ok = t is SCALARS.get(ctype)
            elif struct and struct.group(1) in mirrors:
                ok = t is ctypes.POINTER(mirrors[struct.group(1)])
            else:
                ok = t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)
            if not ok:
                bad.append(f"{name}({ctype} {pname}): argtype {t.__name__}")
    assert not bad, "\n".join(bad)


def test_struct_mirrors_list_the_header_fields_in_order():
    structs, mirrors = hdr.structs(), _mirrors()
    assert sorted(mirrors) == sorted(structs)
    for cname, cls in mirrors.items():
        assert [f[0] for f in cls._fields_] == [n for _, n in structs[cname]], cname


def test_struct_mirrors_match_the_c_layout(tmp_path):
    """sizeof of every struct and offsetof / sizeof of every field, from a C probe compiled against the header."""
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on PATH")
    mirrors = _mirrors()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "pings_hip.h"', "int main(void) {"]
    want = []
    for cname, cls in mirrors.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        want.append(f"{cname} {ctypes.sizeof(cls)}")
        for f in cls._fields_:
            lines.append(f'  printf("{cname}.{f[0]} %zu %zu\\n", offsetof({cname}, {f[0]}), '
                         f"sizeof((({cname}*)0)->{f[0]}));")
            d = getattr(cls, f[0])
            want.append(f"{cname}.{f[0]} {d.offset} {d.size}")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cc, f"-I{hdr.HEADER.parent}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert got == want


def test_abi_version_and_constants_match_the_header_defines():
    defines = hdr.defines()
    mirrored = {n: v for n, v in vars(_abi).items() if n.isupper() and isinstance(v, int)}
    assert {"ABI_VERSION", "RASTER_SURFEL", "RASTER_3DGS", "RASTER_2DGS", "HEAD_COLOR", "HEAD_SEMANTIC",
            "REG_SINGULAR", "REG_ILL_CONDITIONED", "REG_NONFINITE", "REG_F_NORMALS", "REG_F_DIV_GRAD",
            "REG_F_WEIGHTED"} <= set(mirrored)
    assert {n: defines.get("PINGS_" + n) for n in mirrored} == mirrored


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    missing = [n for n in hdr.header_symbols() if not hasattr(L, n)]
    assert not missing, f"symbols declared in include/pings_hip.h but not exported: {missing}"
    assert L.pings_abi_version() == hdr.expected_abi() >= 7
    assert L.pings_last_error() is not None


def test_argument_errors_are_status_codes_not_crashes():
    L = _lib.lib()
    # null pointers / empty shapes are rejected before any GPU work is attempted
    st = L.pings_ssim_forward(None, None, 3, 8, 8, 0, None, None, None, None, None, None)
    assert st == 1
    assert b"null" in L.pings_last_error()
    assert L.pings_ssim_partials_count(0, 8, 8) == 0


def test_a_library_of_another_abi_version_is_refused(monkeypatch):
    """a stale or A/B library must not be called with this package's argtypes."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, "ABI_VERSION", 10_000)
    with pytest.raises(_lib.PingsHipError, match="ABI version"):
        _lib.lib()
    monkeypatch.undo()
    assert _lib.lib().pings_abi_version() == hdr.expected_abi()


def test_double_backward_entry_rejects_other_shapes_before_any_gpu_work():
    """`pings_mlp_double_backward` covers the SDF decoder shape (hidden 64, one output); anything else is a status code
    (the host wrapper then composes the node from device operators), decided before a single HIP call."""
    L = _lib.lib()
    assert L.pings_mlp_double_backward_supported(35, 64, 1) == 1
    assert L.pings_mlp_double_backward_supported(11, 64, 1) == 1
    assert L.pings_mlp_double_backward_supported(32, 128, 24) == 0
    assert L.pings_mlp_double_backward_supported(35, 64, 3) == 0
    st = L.pings_mlp_double_backward(None, None, None, 10, 32, 128, 24, None, None, None, None, None, None, None, None)
    assert st == 1 and b"double backward" in L.pings_last_error()
    st = L.pings_mlp_double_backward(None, None, None, 10, 35, 64, 1, None, None, None, None, None, None, None, None)
    assert st == 1 and b"null" in L.pings_last_error()
