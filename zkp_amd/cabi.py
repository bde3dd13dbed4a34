"""ctypes signatures of the C ABI, read from the headers in include/ -- the one description of the boundary.

Every prototype `ret zkp_name(params);` of a header maps to (restype, argtypes) by a fixed table: uint32_t, uint64_t,
size_t and int by value, a void return as None, char* (const or not) as c_char_p, and every other pointer or array
parameter as c_void_p.  Anything else raises, naming the function: no function is left untyped without notice.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from typing import Dict, List, Optional, Tuple

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
_BY_VALUE = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
_HOOKS = re.compile(r"#ifdef ZKP_BUILD_TEST_HOOKS(.*?)#endif", re.S)
_PROTO = re.compile(r"([^;{}]*?)\b(zkp_\w+)\s*\(([^;{}]*?)\)\s*;")

Signature = Tuple[Optional[type], List[type]]


def _ctype(decl: str, fn: str, param: bool):
    """one parameter (type and name) or return type -> its ctypes type"""
    tokens = re.findall(r"\[[^\]]*\]|\*|\w+|\S", decl)
    words = [t for t in tokens if re.match(r"[A-Za-z_]\w*$", t) and t != "const"]
    stars = sum(t == "*" or t[0] == "[" for t in tokens)
    plain = len(words) + stars + tokens.count("const") == len(tokens)          # no '...', '(' or other punctuation
    if param and len(words) == 2:
        words = words[:1]                                   # drop the parameter's name
    if plain and len(words) == 1:
        base = words[0]
        if stars == 0 and base in _BY_VALUE:
            return _BY_VALUE[base]
        if stars == 0 and base == "void" and not param:
            return None
        if stars == 1 and base == "char" and "[" not in decl:
            return ctypes.c_char_p
        if stars >= 1:
            return ctypes.c_void_p
    raise TypeError(f"{fn}: no ctypes mapping for {'parameter' if param else 'return'} type {decl.strip()!r}")


def parse(src: str, test_hooks: bool = False) -> Dict[str, Signature]:
    """{name: (restype, argtypes)} of the prototypes in header text `src`: those outside the `#ifdef ZKP_BUILD_TEST_HOOKS` section,
    or those inside it"""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    src = "".join(_HOOKS.findall(src)) if test_hooks else _HOOKS.sub("", src)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    sigs = {}
    for m in _PROTO.finditer(src):
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params])
    missed = set(re.findall(r"\b(zkp_\w+)\s*\(", src)) - set(sigs)
    if missed:
        raise TypeError(f"declarations that are not plain prototypes: {sorted(missed)}")
    return sigs


@functools.lru_cache(maxsize=None)
def signatures(header: str, test_hooks: bool = False) -> Dict[str, Signature]:
    """parse() of include/<header>"""
    with open(os.path.join(INCLUDE, header)) as f:
        return parse(f.read(), test_hooks)


def bind(lib: ctypes.CDLL, header: str, test_hooks: bool = False) -> ctypes.CDLL:
    """set restype / argtypes of every function include/<header> declares (and of its test-hook section when asked for)"""
    sigs = dict(signatures(header))
    if test_hooks:
        sigs.update(signatures(header, test_hooks=True))
    for name, (restype, argtypes) in sigs.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib
