"""The one comparison of a ctypes binding with the headers' text (tests/abi_text.py reads it), and the checks every side library
(scgaussian_amd/build.py SIDE_LIBRARIES) shares.

    matches(decl, ctype, structs, ...)          does the ctypes type stand for the C declaration, under a pointer rule?
    prototype_differences / struct_differences  the differences of one function / one struct, as text
    bound_structs(module)                       {name: class} of the ctypes structs a binding module defines
    check_side_library(module, key, ...)        a side library against its header: exports, names, prototypes, structs, constants
"""
import ctypes as C
import os
import subprocess

import abi_text
from scgaussian_amd import _lib, build

# The C scalar types of the headers and their ctypes types.  (On the LP64 targets of this library ctypes has one class for int and
# int32_t, and one for size_t and uint64_t; int32_t against int64_t, float against double and every count or order are told apart.)
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float,
           "double": C.c_double, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "char": C.c_char}

# How a pointer may be bound.  Every rule binds a returned `char*` as c_char_p.
ANY = "any"          # c_void_p, or POINTER(T) for `T*`, or POINTER(c_void_p) for `void**`
TYPED = "typed"      # `void*` as c_void_p, `T*` as exactly POINTER(T)
VOID = "void"        # every pointer has depth 1 and is exactly c_void_p


def matches(decl, ctype, structs, returned=False, pointers=ANY):
    """Does the ctypes type stand for the C declaration?  structs: {name: ctypes class} for the struct types a header may name."""
    if decl.array:
        return (issubclass(ctype, C.Array) and ctype._length_ == decl.array
                and matches(decl._replace(array=0), ctype._type_, structs, pointers=pointers))
    if decl.pointer == 0:
        return ctype is (structs[decl.base] if decl.base in structs else SCALARS.get(decl.base, False))
    if returned and decl.base == "char":
        return decl.pointer == 1 and ctype is C.c_char_p
    if pointers == VOID or (pointers == TYPED and decl.base == "void"):
        return decl.pointer == 1 and ctype is C.c_void_p
    if pointers == ANY and ctype is C.c_void_p:
        return True
    if decl.pointer == 2:
        return pointers == ANY and decl.base == "void" and ctype is C.POINTER(C.c_void_p)
    target = structs.get(decl.base, SCALARS.get(decl.base))
    return target is not None and ctype is C.POINTER(target)


def prototype_differences(fn, restype, argtypes, structs, pointers=ANY):
    diffs = []
    if not matches(fn.ret, restype, structs, returned=True, pointers=pointers):
        diffs.append(f"{fn.name} ({fn.header}): returns {fn.ret.base}{'*' * fn.ret.pointer}, bound as {restype}")
    if len(fn.params) != len(argtypes):
        diffs.append(f"{fn.name} ({fn.header}): {len(fn.params)} parameters, bound with {len(argtypes)}")
    for i, (decl, ctype) in enumerate(zip(fn.params, argtypes)):
        if not matches(decl, ctype, structs, pointers=pointers):
            diffs.append(f"{fn.name} ({fn.header}): parameter {i} is {decl}, bound as {ctype}")
    return diffs


def struct_differences(name, fields, cls, structs, pointers=ANY):
    bound = list(cls._fields_)
    if [f.name for f in fields] != [n for n, _ in bound]:
        return [f"{name}: members {[f.name for f in fields]}, bound as {[n for n, _ in bound]}"]
    return [f"{name}.{f.name} is {f}, bound as {t}" for f, (_, t) in zip(fields, bound)
            if not matches(f, t, structs, pointers=pointers)]


def bound_structs(module):
    return {k: v for k, v in vars(module).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


def exported_names(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def side_header(key, name):
    return os.path.join(build.INCLUDE, build.SIDE_LIBRARIES[key][0], name)


def check_side_library(module, key, header, pointers, prefixes=None, constant_prefixes=None):
    """The part every side library's test shares; returns the Abi of the header for the test's own literals.

    The header is read alone; it alone declares the names, each with one of the library's prefixes; `nm -D` of the library, the
    header and the binding's SYMBOLS name the same functions, none of them one of the main library's (whose glob does not see
    this header); every prototype is bound as declared under the library's pointer rule; the header's structs are the binding's
    STRUCTS in order, field by field, a pointer member being exactly c_void_p; every #define SCG_<NAME> is the binding's <NAME>
    and the binding has no <KEY>_* constant (or one with another of constant_prefixes) the header lacks; the version is the same in the library, the binding, the header."""
    abi = abi_text.read([side_header(key, header)])
    where = abi_text.declared_in(abi)
    assert set(where.values()) == {header}
    assert all(n.startswith(tuple(prefixes or (f"scg_{key}_",))) for n in where), sorted(where)
    assert module.LIB_PATH == build.side_library(key)[0]
    assert exported_names(module.LIB_PATH) == sorted(where) == sorted(module.SYMBOLS)
    main = abi_text.declared_in(abi_text.read())
    assert not set(where) & set(main) and header not in set(main.values()) and not set(module.SYMBOLS) & set(_lib.SYMBOLS)
    structs = dict(bound_structs(_lib), **bound_structs(module))
    diffs = [d for fn in abi.functions for d in prototype_differences(fn, *module.SYMBOLS[fn.name], structs, pointers)]
    own = getattr(module, "STRUCTS", ())
    assert list(abi.structs) == [s.__name__ for s in own]
    diffs += [d for s in own for d in struct_differences(s.__name__, abi.structs[s.__name__], s, structs, VOID)]
    assert not diffs, "\n".join(diffs)
    defined = {n[4:]: v for n, v in abi.defines.items()}
    assert {n: getattr(module, n, None) for n in defined} == defined
    assert {n for n in vars(module) if n.startswith(tuple(constant_prefixes or (key.upper() + "_",)))} <= set(defined)
    version = getattr(module.load(), f"scg_{key}_abi_version")()
    assert version == module.ABI_VERSION == abi.defines[f"SCG_{key.upper()}_ABI_VERSION"]
    return abi
