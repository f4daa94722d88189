"""CPU-only checks of the scene-file path (scgaussian_amd/ply.py, libscg_io.so, include/io/scg_ply.h): the numpy restatement the
GPU tests compare against (tests/ply_refs.py) is held to the files ply_io.save_ply writes, the byte rule to numpy's cast where
numpy's cast is defined, the second library and its binding to the header's text, and the library's validation to its codes."""
import ctypes as C

import numpy as np
import pytest
import torch

import ply_refs as R
from abi_compare import ANY, check_side_library
from scgaussian_amd import _lib, _lib_io, ply, ply_io


def _ray_bound(m):
    kw = {k: torch.from_numpy(m[k].copy()) for k in R.RAY_KEYS + R.BG_KEYS}
    return ply_io.RayBoundModel(**kw)


# ---- the restatement against ply_io's files ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr", [0, 1, 5])
@pytest.mark.parametrize("nb", [0, 3])
def test_restated_bodies_and_headers_are_ply_ios_files(tmp_path, nr, nb):
    m = R.make_model(nr, nb, seed=10 * nr + nb)
    path = tmp_path / "point_cloud.ply"
    ply_io.save_ply(str(path), _ray_bound(m))
    assert path.read_bytes() == R.header(R.names(), nr) + R.pack_ray(m).tobytes()
    bg_path = tmp_path / "point_cloud_bg.ply"
    assert bg_path.exists() == (nb > 0)
    if nb:
        assert bg_path.read_bytes() == R.header(R.names(bg=True), nb) + R.pack_bg(m).tobytes()
    want = R.header(R.COLOR_NAMES, nr + nb, ["float"] * 6 + ["uchar"] * 3) + R.pack_color(m).tobytes()
    assert (tmp_path / "point_cloud_color.ply").read_bytes() == want
    # ... and the package's own header text is the same
    assert ply.header(ply.RAY_NAMES, nr) == R.header(R.names(), nr) and ply.BG_NAMES == R.names(bg=True)
    assert ply.header(ply.COLOR_NAMES, nr + nb, ply.COLOR_TYPES) == R.header(R.COLOR_NAMES, nr + nb, ["float"] * 6 + ["uchar"] * 3)


def test_byte_rule_is_numpys_cast_where_the_cast_is_defined():
    rng = np.random.default_rng(7)
    x = np.concatenate((rng.uniform(-600, 600, 4000), rng.uniform(-2.0 ** 31, 2.0 ** 31, 3000),
                        rng.normal(size=3000) * 10.0 ** rng.integers(-40, 9, 3000))).astype(np.float32)
    x = x[np.isfinite(x) & (np.abs(x) < np.float32(2.0 ** 31))]
    x = np.concatenate((x, rng.uniform(-1, 1, 10_000 - x.size).astype(np.float32)))
    assert x.size == 10_000
    with np.errstate(all="ignore"):
        assert np.array_equal(R.byte_rule(x), x.astype(np.uint8))
        planted = np.array(R.PLANTED, dtype=np.float32)
        assert np.array_equal(R.byte_rule(planted), planted.astype(np.uint8))
    assert R.byte_rule(planted).tolist() == [62, 0, 1, 255, 0, 0, 0, 0, 1, 254, 255, 255, 0, 1, 194, 0, 128]
    # at and beyond 2^31 and for the non-finite values the rule alone decides (another CPU's vector cast may differ): all 0
    assert R.byte_rule(np.array(R.PLANTED_BEYOND, dtype=np.float32)).tolist() == [0] * len(R.PLANTED_BEYOND)
    assert R.byte_rule(np.array([1e-45, -1e-45, 2147483520.0, -2147483520.0], dtype=np.float32)).tolist() == [0, 0, 128, 128]


@pytest.mark.parametrize("nr, nb", [(0, 0), (1, 0), (5, 3), (70, 65)])
def test_unpack_of_pack_is_the_identity_on_bit_patterns(nr, nb):
    m = R.make_model(nr, nb, seed=3)
    if nr:
        m["opacity"][0, 0] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]          # a NaN with a payload
        m["scaling"][0, 1] = np.float32(-0.0)
        m["features_rest"][0, 7, 2] = np.float32(1e-41)                                     # a denormal
    got = R.unpack(R.pack_ray(m), R.column_table(R.names()))
    got.update(R.unpack(R.pack_bg(m), R.column_table(R.names(bg=True), bg=True), bg=True))
    assert sorted(got) == sorted(R.RAY_KEYS + R.BG_KEYS)
    for k in got:
        assert got[k].shape == m[k].shape and np.array_equal(got[k], R.bits(m[k])), k


def test_column_table_reordered_extra_and_suffix_sort():
    base = R.names()
    assert R.column_table(base).tolist() == [0] * 6 + list(range(6, 69)) == ply.column_table(base).tolist()
    assert R.column_table(R.names(bg=True), bg=True).tolist() == [0, 1, 2, 0, 0, 0] + list(range(6, 62))
    assert ply.column_table(R.names(bg=True), bg=True).tolist() == R.column_table(R.names(bg=True), bg=True).tolist()
    # a permutation with two extra properties: f_rest_10 stands in front of f_rest_2 (a sort by text would keep it there)
    rng = np.random.default_rng(5)
    names = base + ["confidence", "extra_1"]
    names = [names[i] for i in rng.permutation(len(names))]
    i10, i2 = names.index("f_rest_10"), names.index("f_rest_2")
    names[min(i10, i2)], names[max(i10, i2)] = "f_rest_10", "f_rest_2"
    table = R.column_table(names)
    assert table.tolist() == ply.column_table(names).tolist()
    assert [names[t] for t in table[6:]] == base[6:] and table[9 + 2] == max(i10, i2) and table[9 + 10] == min(i10, i2)
    # the round trip through that order
    m = R.make_model(4, 0, seed=1)
    own = R.pack_ray(m)
    body = np.zeros((4, len(names)), np.uint32)
    for j, n in enumerate(names):
        body[:, j] = own[:, base.index(n)] if n in base else 0xDEADBEEF
    got = R.unpack(body, table)
    assert all(np.array_equal(got[k], R.bits(m[k])) for k in R.RAY_KEYS)
    # what load_ply refuses
    with pytest.raises(ValueError, match="expected 45 f_rest_"):
        ply.column_table([n for n in base if n != "f_rest_44"])
    with pytest.raises(ValueError, match="opacity"):
        ply.column_table([n for n in base if n != "opacity"])
    with pytest.raises(ValueError, match="rayd"):
        ply.column_table([n for n in base if not n.startswith("rayd")])


# ---- the second library against its header -------------------------------------------------------------------------------------
def test_second_library_exports_and_binds_exactly_its_header():
    abi = check_side_library(_lib_io, "io", "scg_ply.h", ANY, prefixes=("scg_io_", "scg_ply_"))
    assert len(abi.functions) == 7 and list(abi.structs) == ["ScgPlyLayout"]
    assert all(f.base == "uint64_t" and not f.pointer for f in abi.structs["ScgPlyLayout"])
    assert sorted(abi.defines) == sorted("SCG_" + n for n in (
        "IO_ABI_VERSION", "PLY_TILE_ROWS", "PLY_RAY_FLOATS", "PLY_BG_FLOATS", "PLY_COLOR_BYTES", "PLY_MAX_STRIDE"))
    assert _lib_io.load().scg_ply_layout_bytes() == C.sizeof(_lib_io.ScgPlyLayout) == 56
    assert ply.TILE_ROWS == abi.defines["SCG_PLY_TILE_ROWS"] and ply.TILE_ROWS % 4 == 0


def test_layout():
    lib = _lib_io.load()
    L = _lib_io.ScgPlyLayout()
    for nr, nb in ((0, 0), (1, 0), (0, 1), (5, 3), (65, 129), (1_000_000, 250_000), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.scg_ply_layout(nr, nb, C.byref(L)) == 0
        assert (L.ray_offset, L.ray_bytes, L.bg_bytes) == (0, nr * 276, nb * 248)
        assert L.color_bytes == (27 * (nr + nb) + 3) // 4 * 4
        assert L.bg_offset % 256 == L.color_offset % 256 == L.total % 256 == 0
        assert 0 <= L.bg_offset - L.ray_bytes < 256 and 0 <= L.color_offset - (L.bg_offset + L.bg_bytes) < 256
        assert 0 <= L.total - (L.color_offset + L.color_bytes) < 256
    assert lib.scg_ply_layout(-1, 0, C.byref(L)) == -2 and lib.scg_ply_layout(0, -5, C.byref(L)) == -2
    assert lib.scg_ply_layout(1, 1, None) == -1 and b"out is NULL" in lib.scg_io_last_error()


def _fake_model(nr, nb, fake=0x1000):
    m = _lib.ScgModel()
    m.ray.count, m.bg.count = nr, nb
    for n in ("zval", "rayo", "rayd", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(m.ray, n, fake)
    for n in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(m.bg, n, fake)
    return m


def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the pointers are never dereferenced."""
    lib = _lib_io.load()
    fake = 0x1000
    m = _fake_model(5, 3)
    big = 1 << 20
    # pack
    assert lib.scg_ply_pack(None, fake, big, None) == -1 and b"model" in lib.scg_io_last_error()
    assert lib.scg_ply_pack(C.byref(m), None, big, None) == -1
    assert lib.scg_ply_pack(C.byref(m), fake, 100, None) == -4 and b"buffer of 100 bytes" in lib.scg_io_last_error()
    assert lib.scg_ply_pack(C.byref(m), fake + 4, big, None) == -5
    neg = _fake_model(-1, 0)
    assert lib.scg_ply_pack(C.byref(neg), fake, big, None) == -2
    hole = _fake_model(5, 3)
    hole.ray.rayd = None
    assert lib.scg_ply_pack(C.byref(hole), fake, big, None) == -1 and b"ray-bound" in lib.scg_io_last_error()
    hole = _fake_model(5, 3)
    hole.bg.xyz = None
    assert lib.scg_ply_pack(C.byref(hole), fake, big, None) == -1 and b"background" in lib.scg_io_last_error()
    empty = _fake_model(0, 0, fake=None)
    assert lib.scg_ply_pack(C.byref(empty), None, 0, None) == 0                        # nothing to do, nothing launched
    # the view-dependent colour
    assert lib.scg_ply_pack_color_view(C.byref(m), 4, fake, fake, big, None) == -2
    assert lib.scg_ply_pack_color_view(C.byref(m), -1, fake, fake, big, None) == -2
    assert lib.scg_ply_pack_color_view(C.byref(m), 3, None, fake, big, None) == -1
    assert lib.scg_ply_pack_color_view(C.byref(m), 3, fake, fake, 8 * 27 - 1, None) == -4
    assert lib.scg_ply_pack_color_view(C.byref(m), 3, fake, fake + 8, big, None) == -5
    assert lib.scg_ply_pack_color_view(None, 3, fake, fake, big, None) == -1
    # unpack
    table = (C.c_int32 * 69)(*range(69))
    assert lib.scg_ply_unpack(None, 5 * 276, table, 5, 69, 0, C.byref(m), None) == -1
    assert lib.scg_ply_unpack(fake, 5 * 276, None, 5, 69, 0, C.byref(m), None) == -1
    assert lib.scg_ply_unpack(fake, 5 * 276, table, 5, 69, 0, None, None) == -1
    assert lib.scg_ply_unpack(fake, 5 * 276, table, -5, 69, 0, C.byref(m), None) == -2
    assert lib.scg_ply_unpack(fake, 5 * 276 - 4, table, 5, 69, 0, C.byref(m), None) == -4 and b"not 5 rows" in lib.scg_io_last_error()
    assert lib.scg_ply_unpack(fake, 0, table, 5, 0, 0, C.byref(m), None) == -2
    assert lib.scg_ply_unpack(fake, 5 * 4 * 225, table, 5, 225, 0, C.byref(m), None) == -2
    assert lib.scg_ply_unpack(fake, 5 * 4 * 68, table, 5, 68, 0, C.byref(m), None) == -2 and b"table[68] = 68" in lib.scg_io_last_error()
    table[7] = -1
    assert lib.scg_ply_unpack(fake, 5 * 276, table, 5, 69, 0, C.byref(m), None) == -2 and b"table[7] = -1" in lib.scg_io_last_error()
    table[7] = 7
    assert lib.scg_ply_unpack(fake + 4, 5 * 276, table, 5, 69, 0, C.byref(m), None) == -5
    assert lib.scg_ply_unpack(fake, 4 * 276, table, 4, 69, 0, C.byref(m), None) == -2 and b"holds 5 rows" in lib.scg_io_last_error()
    hole = _fake_model(5, 3)
    hole.bg.rotation = None
    assert lib.scg_ply_unpack(fake, 3 * 248, table, 3, 62, 1, C.byref(hole), None) == -1


def test_python_entry_points_refuse_host_models():
    m = _ray_bound(R.make_model(2, 0))
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        ply.pack(m)
    with pytest.raises(_lib.ScgError, match="raw tensors"):
        ply.pack(object())
    with pytest.raises(_lib.ScgError, match="ROCm GPU"):
        ply.load_ply(m, "nowhere.ply", device="cpu")
