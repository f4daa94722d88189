"""CPU-only checks of the C-ABI boundary: the library exports exactly what the headers under include/ declare, the ctypes binding
agrees with the headers' text declaration by declaration (tests/abi_text.py reads it), the library validates arguments without
touching a GPU, and the Python operator mirrors the reference's error behaviour.  No compute calls."""
import ctypes as C
import os
import re

import pytest
import torch

import abi_text
from abi_compare import ANY, TYPED, VOID, bound_structs, exported_names, prototype_differences, struct_differences
from scgaussian_amd import _lib
from scgaussian_amd._lib import ScgFrame
from scgaussian_amd import rasterizer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = abi_text.read()


def test_library_exports_every_declared_symbol():
    """The dynamic table of the library is the set of names the headers declare, each in exactly one header, and NOTHING ELSE: the
    sources are compiled with -fvisibility=hidden (the declarations carry SCG_API) and linked with csrc/exports.map, so no internal
    scg:: function, kernel handle or __hip_cuid_* symbol leaks, and a definition that does not see its declaration is missed here."""
    where = abi_text.declared_in(ABI)                                # raises, naming both headers, when a name is declared twice
    assert len(where) == 73 and len(set(where.values())) == 8
    exported = exported_names(_lib.LIB_PATH)
    assert exported == sorted(where), {n: where.get(n, "not declared") for n in set(exported) ^ set(where)}
    lib = _lib.load()
    for name, header in where.items():
        assert hasattr(lib, name), f"libscg_raster.so does not export {name} ({header})"
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name} ({header})"
    assert lib.scg_abi_version() == _lib.ABI_VERSION == ABI.defines["SCG_ABI_VERSION"] == 10
    # the structs the binding declares have the size the library was compiled with (all of them: the size test below)
    for which, struct in enumerate((_lib.ScgFrame, _lib.ScgWorkspaceLayout, _lib.ScgStageEvents)):
        assert lib.scg_struct_bytes(which) == C.sizeof(struct) > 0
    assert lib.scg_struct_bytes(99) == 0


def test_every_prototype_is_bound_as_declared():
    where = abi_text.declared_in(ABI)
    assert sorted(_lib.SYMBOLS) == sorted(where), {n: where.get(n, "not declared") for n in set(_lib.SYMBOLS) ^ set(where)}
    structs = bound_structs(_lib)
    diffs = [d for fn in ABI.functions for d in prototype_differences(fn, *_lib.SYMBOLS[fn.name], structs)]
    assert not diffs, "\n".join(diffs)


def test_every_struct_is_bound_field_by_field():
    structs = bound_structs(_lib)
    assert sorted(structs) == sorted(ABI.structs) and len(structs) == 17
    diffs = [d for name, fields in ABI.structs.items() for d in struct_differences(name, fields, structs[name], structs)]
    assert not diffs, "\n".join(diffs)


def test_every_size_checked_struct_has_the_librarys_size():
    lib = _lib.load()
    assert {q: len(s) for q, s in _lib.SIZE_CHECKED.items()} == {"scg_struct_bytes": 8, "scg_mono_struct_bytes": 4}
    for query, structs in _lib.SIZE_CHECKED.items():
        for which, struct in enumerate(structs):
            assert getattr(lib, query)(which) == C.sizeof(struct) > 0, (query, which, struct.__name__)
        assert getattr(lib, query)(len(structs)) == 0 and getattr(lib, query)(99) == 0


def test_mirrored_constants_are_the_headers():
    """Every integer #define SCG_<NAME> that the binding mirrors as <NAME> has the header's value; the ten it is known to mirror are
    all there, and the rasterizer's three are the binding's."""
    mirrored = {n[4:]: v for n, v in ABI.defines.items() if hasattr(_lib, n[4:])}
    assert sorted(mirrored) == sorted(("ABI_VERSION", "TILE", "SPLAT_FLOATS", "DSPLAT_FLOATS", "ADAM_MAX_SEGMENTS", "ADAM_FORCE_FULL",
                                       "INIT_STAGE_MAX_STEPS", "SEED_MAX_SEGMENTS", "MONO_MAX_VIEWS", "MONO_MAX_SEGMENTS"))
    assert {n: getattr(_lib, n) for n in mirrored} == mirrored
    assert (R.TILE, R.SPLAT_FLOATS, R.DSPLAT_FLOATS) == (_lib.TILE, _lib.SPLAT_FLOATS, _lib.DSPLAT_FLOATS) == (16, 12, 16)


def test_option_and_flag_bits_of_the_binding_are_the_headers():
    """Every SCG_FORWARD_* / SCG_BACKWARD_* / SCG_DEBUG_* / SCG_BINNING_* enumerator of the headers and of csrc/scg_debug.h has a
    constant of the same name (minus SCG_) and value in _lib, and _lib has none the headers lack."""
    kinds = r"(FORWARD|BACKWARD|DEBUG|BINNING)_[A-Z0-9_]+"
    both = abi_text.read([os.path.join(ROOT, "scgaussian_amd", "csrc", "scg_debug.h")]).enums
    assert not set(both) & set(ABI.enums)
    both.update(ABI.enums)
    declared = {k[4:]: v for k, v in both.items() if re.fullmatch("SCG_" + kinds, k)}
    assert len(declared) >= 11 and declared["FORWARD_ARM_PARTIAL_SUMS"] == 64 and declared["BINNING_AUTO"] == 0
    bound = {k: v for k, v in vars(_lib).items() if re.fullmatch(kinds, k)}
    assert bound == declared, sorted(set(bound.items()) ^ set(declared.items()))
    # the bits of one option word do not collide: scg_forward's `options` carries the FORWARD_* and the DEBUG_* bits together
    word = [v for k, v in declared.items() if k.startswith(("FORWARD_", "DEBUG_"))]
    assert all(v > 0 and v & (v - 1) == 0 for v in word) and len(set(word)) == len(word)


# ---- the reader and the comparison above, on short headers with one known difference each: neither passes everything ----------

_TOY = """
#ifndef SCG_TOY_H
#define SCG_TOY_H
#define SCG_TOY_MAX 7      /* a constant */
extern "C" {
typedef struct ScgToy {
    int32_t rows, cols;    // two members of one size
    const float* data;
    double m[9];
} ScgToy;
SCG_API int scg_toy_run(const ScgToy* toy, int64_t n, float* out, void* stream);
SCG_API size_t scg_toy_bytes(void);
}
#endif
"""


class ScgToy(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("data", C.c_void_p), ("m", C.c_double * 9)]


_TOY_SYMBOLS = {"scg_toy_run": (C.c_int, [C.POINTER(ScgToy), C.c_int64, C.c_void_p, C.c_void_p]), "scg_toy_bytes": (C.c_size_t, [])}


def _toy_differences(text):
    abi = abi_text.parse(text, "toy.h")
    structs = {"ScgToy": ScgToy}
    assert sorted(abi_text.declared_in(abi)) == sorted(_TOY_SYMBOLS) and list(abi.structs) == ["ScgToy"]
    return ([d for fn in abi.functions for d in prototype_differences(fn, *_TOY_SYMBOLS[fn.name], structs)]
            + struct_differences("ScgToy", abi.structs["ScgToy"], ScgToy, structs))


def test_the_toy_header_as_bound_shows_no_difference():
    assert _toy_differences(_TOY) == []
    abi = abi_text.parse(_TOY, "toy.h")
    assert abi.defines == {"SCG_TOY_MAX": 7} and [f.header for f in abi.functions] == ["toy.h", "toy.h"]
    assert abi.structs["ScgToy"] == [abi_text.Decl("rows", "int32_t", 0, 0), abi_text.Decl("cols", "int32_t", 0, 0),
                                     abi_text.Decl("data", "float", 1, 0), abi_text.Decl("m", "double", 0, 9)]


def test_the_pointer_rules_tell_the_toy_bindings_pointers_apart():
    """scg_toy_run is bound with POINTER(ScgToy) for `const ScgToy*` and c_void_p for `float*` and `void*`: the rule of the main
    library takes all three, the typed rule refuses the float*, the void-only rule the struct pointer."""
    run = abi_text.parse(_TOY, "toy.h").functions[0]
    per_rule = {rule: prototype_differences(run, *_TOY_SYMBOLS["scg_toy_run"], {"ScgToy": ScgToy}, rule) for rule in (ANY, TYPED, VOID)}
    assert per_rule[ANY] == [] and len(per_rule[TYPED]) == len(per_rule[VOID]) == 1
    assert "parameter 2" in per_rule[TYPED][0] and "parameter 0" in per_rule[VOID][0]


@pytest.mark.parametrize("what, old, new", [
    ("two swapped members of one size", "int32_t rows, cols;", "int32_t cols, rows;"),
    ("int64_t against int32_t", "int64_t n", "int32_t n"),
    ("a dropped parameter", "int64_t n, float* out", "int64_t n"),
    ("a changed array length", "double m[9]", "double m[12]"),
    ("a pointer against a value", "const float* data", "float data"),
    ("another return type", "SCG_API size_t scg_toy_bytes", "SCG_API int32_t scg_toy_bytes"),
])
def test_a_mutated_toy_header_shows_a_difference(what, old, new):
    assert _TOY.count(old) == 1
    assert _toy_differences(_TOY.replace(old, new)), what


def test_a_name_declared_twice_is_named_with_both_headers():
    one, two = abi_text.parse(_TOY, "toy.h"), abi_text.parse("SCG_API size_t scg_toy_bytes(void);", "other.h")
    with pytest.raises(abi_text.AbiTextError, match=r"scg_toy_bytes is declared twice: in toy\.h and in other\.h"):
        abi_text.declared_in(abi_text.Abi(one.functions + two.functions, {}, {}, {}))


@pytest.mark.parametrize("old, new", [
    ("SCG_API int scg_toy_run(", "SCG_API int scg_toy_run(void (*callback)(int), "),        # a function pointer
    ("int64_t n,", "unsigned long n,"),                                                      # a two-word type
    ("SCG_API size_t scg_toy_bytes(void);", "size_t scg_toy_bytes(void);"),                  # a prototype without SCG_API
    ("SCG_API size_t scg_toy_bytes(void);", "struct ScgOther;"),                             # a forward declaration
    ("double m[9];", "double m[SCG_TOY_MAX];"),                                              # a length that is not a number
    ("double m[9];", "double m[9]; union { int a; float b; } u;"),                           # a nested block
    ("#define SCG_TOY_MAX 7", "#define SCG_TOY_MAX (3 + 4)"),                                # a #define that is not an integer
    ("#define SCG_TOY_MAX 7", "#define SCG_TOY_MAX 7\n#define SCG_TOY_MAX 8"),               # ... or is there twice
    ("} ScgToy;", "} ScgToy2;"),                                                             # two names for one struct
    ("#endif", "}\n#endif"),                                                                 # a brace too many at the end
])
def test_an_unreadable_declaration_raises(old, new):
    assert _TOY.count(old) == 1
    with pytest.raises(abi_text.AbiTextError):
        abi_text.parse(_TOY.replace(old, new), "toy.h")


def test_scratch_size_queries_are_monotone():
    lib = _lib.load()
    assert lib.scg_geometry_scratch_bytes(1) > 0
    assert lib.scg_geometry_scratch_bytes(1_000_000) >= 1_000_000 // 256 * 4
    auto, global_sort = _lib.BINNING_AUTO, _lib.BINNING_GLOBAL_SORT
    a = lib.scg_binning_scratch_bytes(500, 1000, 256, 256, auto)
    b = lib.scg_binning_scratch_bytes(500_000, 1_000_000, 1920, 1080, auto)
    c = lib.scg_binning_scratch_bytes(500_000, 1_000_000, 1920, 1080, global_sort)      # global 64-bit sort: 20 B / instance
    assert 0 < a < b and c >= 1_000_000 * 20
    # the tile-first path never materialises the R 64-bit key/value pairs twice: smaller scratch than the global sort
    assert lib.scg_binning_scratch_bytes(500_000, 4_000_000, 1920, 1080, auto) < \
        lib.scg_binning_scratch_bytes(500_000, 4_000_000, 1920, 1080, global_sort)
    assert lib.scg_sort_scratch_bytes(10) > 0 and lib.scg_scan_scratch_bytes(10) > 0


def _frame(**kw):
    base = dict(P=4, sh_degree=3, sh_coeffs=16, width=64, height=48, tanfovx=0.5, tanfovy=0.4,
                scale_modifier=1.0, prefiltered=0, debug=0, viewmatrix=0x1000, projmatrix=0x1000, campos=0x1000, bg=0x1000)
    base.update(kw)
    return ScgFrame(**base)


def test_argument_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: validation fails first
    # NULL frame
    rc = lib.scg_geometry_forward(None, *([fake] * 7), *([fake] * 6), fake, 1 << 20, None)
    assert rc == -1 and b"frame" in lib.scg_last_error()
    # degree out of range
    fr = _frame(sh_degree=5)
    rc = lib.scg_geometry_forward(C.byref(fr), *([fake] * 7), *([fake] * 6), fake, 1 << 20, None)
    assert rc == -2
    # both shs and colors_precomp
    fr = _frame()
    rc = lib.scg_geometry_forward(C.byref(fr), fake, fake, fake, fake, fake, fake, None, *([fake] * 6), fake, 1 << 20, None)
    assert rc == -3 and b"exactly one" in lib.scg_last_error()
    # neither scale/rot nor cov3D
    rc = lib.scg_geometry_forward(C.byref(fr), fake, fake, fake, None, None, None, None, *([fake] * 6), fake, 1 << 20, None)
    assert rc == -3
    # scratch too small
    rc = lib.scg_geometry_forward(C.byref(fr), fake, fake, fake, None, fake, fake, None, *([fake] * 6), fake, 0, None)
    assert rc == -4
    # misaligned splats
    rc = lib.scg_geometry_forward(C.byref(fr), fake, fake, fake, None, fake, fake, None, fake + 4, fake, fake, fake, fake, fake, fake, 1 << 20, None)
    assert rc == -5
    # binning: unknown algorithm selector
    assert lib.scg_binning(C.byref(fr), 10, fake, fake, fake, fake, None, 7, fake, 1 << 30, None) == -2
    # sort: bad end_bit
    assert lib.scg_sort_pairs(fake, fake, fake, fake, 10, 0, fake, 1 << 20, None) == -2
    # geometry backward: gradient outputs must match the input path
    rc = lib.scg_geometry_backward(C.byref(fr), fake, fake, fake, None, fake, fake, None, fake, fake, fake,
                                   fake, fake, fake, None, None, fake, fake, None, 0, None)
    assert rc == -3


def test_operator_error_behaviour_matches_reference_api():
    st = R.GaussianRasterizationSettings(48, 64, 0.5, 0.4, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 3,
                                         torch.zeros(3), False, False)
    assert st._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                          "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    rast = R.GaussianRasterizer(raster_settings=st)
    P = 5
    m, m2, op = torch.zeros(P, 3), torch.zeros(P, 3), torch.ones(P, 1)
    sh, col = torch.zeros(P, 16, 3), torch.zeros(P, 3)
    sc, rot, cov = torch.ones(P, 3), torch.zeros(P, 4), torch.zeros(P, 6)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        rast(means3D=m, means2D=m2, opacities=op, shs=sh, colors_precomp=col, scales=sc, rotations=rot)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        rast(means3D=m, means2D=m2, opacities=op, scales=sc, rotations=rot)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        rast(means3D=m, means2D=m2, opacities=op, shs=sh, scales=sc, rotations=rot, cov3D_precomp=cov)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        rast(means3D=m, means2D=m2, opacities=op, shs=sh, scales=sc)
    # no silent CPU fallback: CPU tensors are refused loudly
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        rast(means3D=m, means2D=m2, opacities=op, shs=sh, scales=sc, rotations=rot)


def test_drop_in_module_name():
    import diff_gaussian_rasterization as dgr
    assert dgr.GaussianRasterizer is R.GaussianRasterizer
    assert dgr.GaussianRasterizationSettings is R.GaussianRasterizationSettings


def test_one_call_entry_points_layout_and_validation_without_a_gpu():
    """scg_workspace_layout: aligned, non-overlapping, monotone in the capacity; scg_forward / scg_backward /
    scg_wait_num_rendered reject bad arguments with codes, before anything touches a device."""
    lib = _lib.load()
    L = _lib.ScgWorkspaceLayout()
    assert lib.scg_workspace_layout(200_000, 1_500_000, 1008, 756, C.byref(L)) == 0
    names = ("splats", "rects", "depth_keys", "clamped", "point_list", "ranges", "final_T", "n_contrib", "bin_scratch")
    offs = [int(getattr(L, n)) for n in names] + [int(L.total)]
    assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and offs[0] == 0
    assert offs[1] - offs[0] >= 200_000 * 48 and offs[5] - offs[4] >= 1_500_000 * 4
    assert offs[7] - offs[6] >= 1008 * 756 * 4 and int(L.partial_words) * 4 == lib.scg_geometry_scratch_bytes(200_000)
    L2 = _lib.ScgWorkspaceLayout()
    assert lib.scg_workspace_layout(200_000, 3_000_000, 1008, 756, C.byref(L2)) == 0 and L2.total > L.total
    assert lib.scg_workspace_layout(200_000, -1, 1008, 756, C.byref(L2)) == -2                  # SCG_E_RANGE
    assert lib.scg_workspace_layout(200_000, 10, 1008, 756, None) == -1                         # SCG_E_NULL
    fr = _frame()
    fake = 0x1000
    args = [C.byref(fr), fake, fake, fake, None, fake, fake, None]
    # NULL workspace
    assert lib.scg_forward(*args, 100, None, 0, fake, fake, fake, fake, fake, None, None, 0, None, None) == -1
    # workspace too small
    rc = lib.scg_forward(*args, 100, fake, 16, fake, fake, fake, fake, fake, None, None, 0, None, None)
    assert rc == -4 and b"workspace" in lib.scg_last_error()
    # both colour inputs: SCG_E_EXCLUSIVE, with the reference's wording
    bad = [C.byref(fr), fake, fake, fake, fake, fake, fake, None]
    assert lib.scg_forward(*bad, 100, fake, 1 << 30, fake, fake, fake, fake, fake, None, None, 0, None, None) == -3
    assert b"exactly one of either SHs or precomputed colors" in lib.scg_last_error()
    assert lib.scg_backward(None, *([fake] * 7), fake, 100, fake, fake, None, None, fake, 0, *([fake] * 8), 0, None, None) == -1
    assert lib.scg_wait_num_rendered(None, None, 10) < 0
    # the host-side sum of the per-workgroup partial sums (no event: nothing to wait for)
    part = (C.c_uint32 * 8)(5, 7, 11, 0, 0, 0, 0, 0)
    assert lib.scg_wait_num_rendered(None, C.cast(part, C.c_void_p), 600) == 23
    assert lib.scg_event_elapsed_ms(None, None, None) == -1
    # ABI 9: armed words (scg_forward's SCG_FORWARD_ARM_PARTIAL_SUMS) are WATCHED until their workgroup has written them — here a
    # thread plays the geometry kernel, writing the three words of P = 600 one by one
    import threading
    import time
    armed = (C.c_uint32 * 3)(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)

    def kernel():
        for i, v in ((1, 40), (0, 2), (2, 100)):
            time.sleep(0.02)
            armed[i] = v
    th = threading.Thread(target=kernel)
    t0 = time.perf_counter()
    th.start()
    assert lib.scg_wait_num_rendered(None, C.cast(armed, C.c_void_p), 600) == 142
    assert time.perf_counter() - t0 >= 0.05
    th.join()


def test_debug_flag_dumps_the_arguments_of_a_failing_call(tmp_path, monkeypatch):
    """arguments/__init__.py:68 `--debug` -> gaussian_renderer/__init__.py:50: with debug=True a failing rasterizer call leaves
    a snapshot of its arguments behind (upstream: snapshot_fw.dump) and re-raises; without it nothing is written."""
    monkeypatch.chdir(tmp_path)
    P = 5
    base = dict(image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=3, campos=torch.zeros(3), prefiltered=False)
    kw = dict(means3D=torch.rand(P, 3), means2D=torch.zeros(P, 3), opacities=torch.rand(P, 1), shs=torch.rand(P, 16, 3),
              scales=torch.rand(P, 3), rotations=torch.rand(P, 4))
    with pytest.raises(_lib.ScgError):                       # CPU tensors: the product has no CPU path
        R.GaussianRasterizer(R.GaussianRasterizationSettings(debug=False, **base))(**kw)
    assert not os.path.exists(R.DEBUG_SNAPSHOT_FW)
    with pytest.raises(_lib.ScgError):
        R.GaussianRasterizer(R.GaussianRasterizationSettings(debug=True, **base))(**kw)
    snap = torch.load(R.DEBUG_SNAPSHOT_FW, weights_only=False)
    assert torch.equal(snap["means3D"], kw["means3D"]) and torch.equal(snap["sh"], kw["shs"]) and snap["cov3Ds_precomp"] is None
    assert snap["raster_settings"][0] == 48 and snap["raster_settings"][-1] is True
