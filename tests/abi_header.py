"""A small reader of include/pings_hip.h for the ABI tests: prototypes, `typedef struct` field lists and `#define`s.

It understands the subset of C the header is written in (one declarator list per field line, `void` for no
parameters, no function pointers); the tests compare what it reads with pings_amd/_abi.py.
"""
from __future__ import annotations

import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "pings_hip.h"


def _code() -> str:
    txt = HEADER.read_text()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return re.sub(r"//[^\n]*", " ", txt)


def _ctype(t: str) -> str:
    """Canonical spelling of a C type: single spaces, `*` attached to what precedes it."""
    t = re.sub(r"\s+", " ", t).strip()
    return re.sub(r"\s*(\*+)\s*", r"\1 ", t).strip()


def _split_decl(decl: str) -> tuple[str, str]:
    """'const float* x' -> ('const float*', 'x')."""
    m = re.fullmatch(r"(.*?)(\w+)", decl.strip(), flags=re.S)
    return _ctype(m.group(1)), m.group(2)


def prototypes() -> dict[str, tuple[str, list[tuple[str, str]]]]:
    """{name: (return type, [(parameter type, parameter name), ...])} of every PINGS_API function, in header order."""
    out = {}
    for ret, name, params in re.findall(r"PINGS_API\s+([\w\s\*]+?)\s*\b(pings_\w+)\s*\(([^)]*)\)\s*;", _code()):
        params = params.strip()
        out[name] = (_ctype(ret), [] if params in ("", "void") else [_split_decl(p) for p in params.split(",")])
    return out


def header_symbols() -> list[str]:
    """Names of every PINGS_API function declared in include/pings_hip.h."""
    return list(prototypes())


def structs() -> dict[str, list[tuple[str, str]]]:
    """{typedef name: [(field type, field name), ...]} of every `typedef struct`, fields in declaration order."""
    out = {}
    for body, typedef in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", _code(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")     # `const float *W1, *b1` declares two `const float*`
            base, stars, name = re.fullmatch(r"(.*?)([\s\*]*)(\w+)", first.strip(), flags=re.S).groups()
            fields.append((_ctype(base + stars), name))
            for d in more:
                fields.append((_ctype(base + "*" * d.count("*")), d.replace("*", "").strip()))
        out[typedef] = fields
    return out


def defines() -> dict[str, int]:
    """{name: value} of every `#define NAME <integer>`."""
    return {n: int(v) for n, v in re.findall(r"^\s*#define\s+(\w+)\s+(-?\d+)\b", _code(), flags=re.M)}


def expected_abi() -> int:
    """PINGS_ABI_VERSION of the header."""
    return defines()["PINGS_ABI_VERSION"]
