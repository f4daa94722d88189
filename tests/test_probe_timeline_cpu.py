"""CPU-only checks of the per-wave timeline probe: the probe build compiles and links, the layout of its log reads the same in
csrc/probe_timeline.h and in tools/probes/_timeline_log.py, and no other file under csrc tests the probe build's macro.

The header is read as text, in the manner of abi_text.py: regular expressions on this project's own style.  Its constants are
`constexpr <type> kTl<Name> = <integer expression>;`, its record accessors and the log's size are function-like macros whose
bodies are integer / pointer expressions in those constants; here they are evaluated with cost_out = 0 and index = 0, which
leaves the region's offset in words."""
import importlib.util
import os
import re

import abi_text
from scgaussian_amd import build

HEADER = os.path.join(build.CSRC, "probe_timeline.h")
MACRO = "SCG_PROBE_TIMELINE"
N_TILES = (1, 7, 8, 9, 2040)


def _python_side():
    spec = importlib.util.spec_from_file_location("_timeline_log", os.path.join(abi_text.ROOT, "tools", "probes", "_timeline_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _expression(text, names):
    """A C integer expression of the header in Python: casts, the namespace and integer suffixes dropped."""
    text = re.sub(r"\(size_t\)|scg::", "", text)
    text = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\b", r"\1", text)
    if not re.fullmatch(r"[\w\s()+*\-]+", text):
        raise ValueError(f"probe_timeline.h: cannot read the expression {text!r}")
    return eval(text, {"__builtins__": {}}, dict(names))                            # noqa: S307 (checked against the pattern above)


def _header_side():
    """({kTl name: value}, {macro name: (parameters, body)}) of csrc/probe_timeline.h."""
    with open(HEADER) as fh:
        code = abi_text.strip_comments(fh.read())
    constants = {}
    for name, value in re.findall(r"constexpr\s+(?:int|uint32_t)\s+(kTl\w+)\s*=\s*([^;]+);", code):
        assert name not in constants, name
        constants[name] = _expression(value, constants)
    macros = {name: ([p.strip() for p in params.split(",")], body.strip())
              for name, params, body in re.findall(r"#define\s+(SCG_TL_\w+)\(([^)]*)\)\s+(.+)", code)}
    return constants, macros


def _offset(macros, constants, name, n_tiles):
    params, body = macros[name]
    values = dict(constants, cost_out=0, index=0)
    assert set(params) <= {"cost_out", "n_tiles", "index"}, (name, params)
    return _expression(body, dict(values, n_tiles=n_tiles))


def test_the_probe_build_compiles_and_links():
    assert build.PROBE_TIMELINE_TAG == "tl"
    including = set()
    for src in build.SOURCES:
        with open(os.path.join(build.CSRC, src)) as fh:
            if re.search(r'#include\s+"(probe_timeline|tile_sort)\.h"', fh.read()):    # (tile_sort.h includes the header)
                including.add(src)
    assert including == set(build.PROBE_TIMELINE_SOURCES)
    path = build.build_probe_timeline_variant()
    assert path == build.LIB_PATH.replace(".so", "_tl.so") and os.path.getsize(path) > 0
    for src in build.PROBE_TIMELINE_SOURCES:                                        # objects of its own, stamped: a rerun is free
        obj = os.path.join(build.OBJ_DIR, src.replace(".hip", "_tl.o"))
        assert os.path.exists(obj) and os.path.exists(obj + ".sha"), src


def test_header_and_python_module_hold_the_same_layout():
    tl = _python_side()
    c, macros = _header_side()
    assert (c["kTlScatterRecord"], c["kTlGeometryRecord"], c["kTlBlendRecord"], c["kTlBackwardRecord"]) == (
        tl.SCATTER_RECORD, tl.GEOMETRY_RECORD, tl.BLEND_RECORD, tl.BACKWARD_RECORD) == (8, 8, 8, 4)
    assert (c["kTlSigScatter"], c["kTlSigGeometry"], c["kTlSigBlend"], c["kTlSigSort"], c["kTlSigBackward"]) == (
        tl.SIG_SCATTER, tl.SIG_GEOMETRY, tl.SIG_BLEND, tl.SIG_SORT, tl.SIG_BACKWARD) == (
        0xC0FFEE, 0xC0FFEE00, 0xB1E9D000, 0x50B70000, 0xBAC00000)
    for n in N_TILES:
        # offsets from the first word of the buffer: the cost words come first
        assert _offset(macros, c, "SCG_TL_SCATTER_RECORD", n) == n + tl.SCATTER_AT == n
        assert _offset(macros, c, "SCG_TL_GEOMETRY_RECORD", n) == n + tl.GEOMETRY_AT == n + 65792
        assert _offset(macros, c, "SCG_TL_BLEND_RECORD", n) == n + tl.BLEND_AT == n + 65792 + 32768
        assert _offset(macros, c, "SCG_TL_BACKWARD_RECORD", n) == n + tl.backward_at(n) == n + 65792 + 32768 + (n + 8) * 40
        assert _offset(macros, c, "SCG_TL_LOG_WORDS", n) == tl.log_words(n) == 65792 + 32768 + (n + 8) * 40 + (n + 8) * 16 + 64
        # a record index advances by the record's size, and the regions do not overlap at the launch's record counts
        for name, size in (("SCATTER", tl.SCATTER_RECORD), ("GEOMETRY", tl.GEOMETRY_RECORD), ("BLEND", tl.BLEND_RECORD),
                           ("BACKWARD", tl.BACKWARD_RECORD)):
            params, body = macros[f"SCG_TL_{name}_RECORD"]
            one = _expression(body, dict(c, cost_out=0, n_tiles=n, index=1))
            assert one - _offset(macros, c, f"SCG_TL_{name}_RECORD", n) == size
        slots = (n + 7) // 8 * 8                                                    # tile_order_slots
        assert tl.BLEND_AT + 5 * slots * tl.BLEND_RECORD <= tl.backward_at(n)
        assert tl.backward_at(n) + 4 * slots * tl.BACKWARD_RECORD <= tl.log_words(n)


def test_only_the_header_tests_the_probe_builds_macro():
    allowed_line = re.compile(r"\s*uint32_t probe\[8\];")                            # tile_sort.h's LDS field, if it is guarded there
    for name in sorted(os.listdir(build.CSRC)):
        path = os.path.join(build.CSRC, name)
        if not os.path.isfile(path) or name == "probe_timeline.h":
            continue
        with open(path, errors="replace") as fh:
            lines = fh.read().splitlines()
        hits = [i for i, line in enumerate(lines) if MACRO in line]
        if name == "tile_sort.h" and hits:
            assert len(hits) == 1 and lines[hits[0]].strip() in ("#ifdef " + MACRO, "#if defined(" + MACRO + ")"), hits
            assert allowed_line.fullmatch(lines[hits[0] + 1]) and lines[hits[0] + 2].strip() == "#endif"
        else:
            assert not hits, f"{name} names {MACRO} in line {hits[0] + 1}: the probe lives behind csrc/probe_timeline.h"
    with open(HEADER) as fh:
        assert MACRO in fh.read()
