"""The one reader of the C headers' text: what include/*.h declare, for the tests that hold the library and the binding to it.

Regular expressions on this project's own header style, not a C parser.  A header is comments, preprocessor lines, one
`extern "C"` block and statements that end in `;` — an `SCG_API` prototype, a `typedef struct NAME { ... } NAME`, or an `enum
{ NAME = value, ... }`.  Anything else raises AbiTextError: nothing is skipped.

    read()                the Abi of every include/*.h (found by glob), or of the paths given
    parse(text, header)   the Abi of one header's text
    declared_in(abi)      {function name: header}; raises when a name is declared twice
    header_of(name)       the header under include/ that declares the function, or None
    declared_by(header)   the functions a header under include/ declares
"""
import functools
import glob
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# base: the C type's name without const / struct; pointer: the number of `*`; array: the length in `[...]`, 0 without
Decl = namedtuple("Decl", "name base pointer array")
Function = namedtuple("Function", "name header ret params")           # ret: a Decl without a name; params: Decls
# functions: a list in the order of declaration; structs: {name: [Decl]}; defines: {SCG_NAME: int}; enums: {NAME: int}
Abi = namedtuple("Abi", "functions structs defines enums")


class AbiTextError(ValueError):
    pass


def _decl(text, what):
    """`const float* x`, `size_t`, `void** out`, `const struct ScgMono* a`, `float w2c[12]`."""
    m = re.fullmatch(r"(?:const\s+)?(?:struct\s+)?(\w+)\s*(\**)\s*(\w*)\s*(?:\[(\d+)\])?", text.strip())
    if not m or m.group(1) in ("const", "struct"):
        raise AbiTextError(f"{what}: cannot read the declaration {text.strip()!r}")
    return Decl(m.group(3), m.group(1), len(m.group(2)), int(m.group(4) or 0))


def _fields(body, what):
    """The members of a struct: `type a, *b, c[3];` declares three, each with its own stars and length."""
    fields = []
    for member in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.+)", member, flags=re.S)
        if not m:
            raise AbiTextError(f"{what}: cannot read the member {member!r}")
        fields += [_decl(m.group(1) + " " + d, what) for d in m.group(2).split(",")]
    if not fields or any(not f.name for f in fields) or len({f.name for f in fields}) != len(fields):
        raise AbiTextError(f"{what}: empty, or a member without a name or named twice")
    return fields


def _define(line, header, defines):
    """`#define SCG_<NAME> <integer>` is recorded; include guards, SCG_API and the other directives are the only lines passed over."""
    m = re.fullmatch(r"#\s*define\s+(\w+)(?:\s+(.+))?", line)
    if not m:
        if re.match(r"#\s*(ifn?def|endif|include|pragma once)\b", line):
            return
        raise AbiTextError(f"{header}: cannot read the directive {line!r}")
    name, value = m.group(1), (m.group(2) or "").strip()
    if (name.endswith("_H") and not value) or name == "SCG_API":
        return
    if not re.fullmatch(r"SCG_[A-Z0-9_]+", name) or not re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+)[uUlL]*", value) or name in defines:
        raise AbiTextError(f"{header}: cannot read #define {name} {value}, or it is defined twice")
    defines[name] = int(value.rstrip("uUlL"), 0)


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def parse(text, header):
    abi = Abi([], {}, {}, {})
    code = []
    for line in strip_comments(text).splitlines():
        if line.strip().startswith("#"):
            _define(line.strip(), header, abi.defines)
        else:
            code.append(line)
    code, blocks = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(code))
    depth, start, statements = 0, 0, []
    for i, ch in enumerate(code):                                    # statements end at a `;` outside braces
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            statements.append(" ".join(code[start:i].split()))
            start = i + 1
    if code[start:].split() != ["}"] * blocks:                       # what is left closes the extern "C" block, nothing else
        raise AbiTextError(f"{header}: cannot read the end of the header: {' '.join(code[start:].split())!r}")
    for st in statements:
        fn = re.fullmatch(r"SCG_API\s+(.+?)\b(scg_[a-z0-9_]+)\s*\(([^()]*)\)", st)
        struct = re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", st)
        enum = re.fullmatch(r"enum \{(.*)\}", st)
        if fn:
            params = [] if fn.group(3).strip() == "void" else [_decl(p, fn.group(2)) for p in fn.group(3).split(",")]
            abi.functions.append(Function(fn.group(2), header, _decl(fn.group(1), fn.group(2))._replace(name=""), params))
        elif struct and struct.group(1) == struct.group(3) and struct.group(1) not in abi.structs:
            abi.structs[struct.group(1)] = _fields(struct.group(2), struct.group(1))
        elif enum:
            for entry in enum.group(1).split(","):
                m = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\w+)\s*", entry)
                if not m or m.group(1) in abi.enums:
                    raise AbiTextError(f"{header}: cannot read the enumerator {entry.strip()!r}, or it is named twice")
                abi.enums[m.group(1)] = int(m.group(2), 0)
        else:
            raise AbiTextError(f"{header}: cannot read {st!r}")
    return abi


def read(paths=None):
    """One Abi over the headers (default: every include/*.h).  A struct, #define or enumerator named in two headers raises; a
    function declared twice is kept twice, for declared_in to name both headers."""
    paths = sorted(glob.glob(os.path.join(INCLUDE, "*.h"))) if paths is None else paths
    total = Abi([], {}, {}, {})
    for path in paths:
        with open(path) as fh:
            abi = parse(fh.read(), os.path.basename(path))
        total.functions.extend(abi.functions)
        for mine, theirs in zip(total[1:], abi[1:]):
            if set(mine) & set(theirs):
                raise AbiTextError(f"{os.path.basename(path)}: {sorted(set(mine) & set(theirs))} declared in another header too")
            mine.update(theirs)
    return total


def declared_in(abi):
    where = {}
    for fn in abi.functions:
        if fn.name in where:
            raise AbiTextError(f"{fn.name} is declared twice: in {where[fn.name]} and in {fn.header}")
        where[fn.name] = fn.header
    return where


@functools.lru_cache(maxsize=None)
def _where():
    return declared_in(read())


def header_of(name):
    """The header under include/ that declares the function, or None (the headers are read once)."""
    return _where().get(name)


def declared_by(header):
    """The sorted names of the functions that the header under include/ declares."""
    return sorted(name for name, where in _where().items() if where == header)
