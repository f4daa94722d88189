"""Host-side logic of the binding that needs no GPU (round 6): the capacity policy, what a settled count does to a camera's capacity,
camera identity without a device read, the model path's attribute mapping and its refusal of models the kernels cannot take, the
counters' summary per SH degree, the gradient arena's layout, pool and SH-tail promise (_grads.py)."""
import os
import sys
import types
import weakref

import pytest
import torch

from scgaussian_amd import _counts as C
from scgaussian_amd import _grads as G
from scgaussian_amd import model_path as mp
from scgaussian_amd import rasterizer as R
from scgaussian_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capacity_policy_head_room_and_stability():
    for count in (0, 1, 4095, 22_000, 1_285_028, 5_455_250, 123_456_789):
        cap = R._capacity_for(count)
        assert cap >= count + count // 8 and cap <= 2 * count + 65536 + 8192, (count, cap)
        # a count that moves by a per cent keeps the capacity (the workspace plan keyed by it stays cached)
        assert R._next_capacity(cap, int(count * 1.01)) == cap
        assert R._next_capacity(cap, count) == cap
        # growth beyond the head room, or a count that fell to less than half: re-derived
        assert R._next_capacity(cap, cap) > cap
        if count > 200_000:
            assert R._next_capacity(cap, count // 3) < cap
    assert R._next_capacity(None, 1000) == R._capacity_for(1000)


def test_a_settled_count_moves_the_cameras_capacity():
    spec = types.SimpleNamespace(hint={}, cam_hint={}, pending={})
    key = (640, 480, b"camera")
    w = R._CountWord()
    w.slot, w.np, w.ptr, w.cap, w.P, w.key, w.device_index, w.captured = 0, None, 0, 100_000, 5000, key, 0, False
    before = dict(R._OVERFLOW)
    R._settle_word(spec, w, 80_000)                              # inside the capacity: kept
    assert spec.cam_hint[key] == (100_000, 80_000, 5000) and spec.hint[(5000, 640, 480)] == 100_000
    assert R._OVERFLOW["overflows"] == before["overflows"] and R._OVERFLOW["settled"] == before["settled"] + 1
    R._settle_word(spec, w, 150_000)                             # clipped: counted, room for the count next time
    assert R._OVERFLOW["overflows"] == before["overflows"] + 1
    assert spec.cam_hint[key][0] >= 150_000 + 150_000 // 8 and spec.cam_hint[key][1:] == (150_000, 5000)


def _capacity_by_hand(count):
    """The policy's head-room formula written out: 12.5 % + 4 096 on top of the count, rounded up to 1/16 of its magnitude."""
    need = int(count * 1.125) + 4096
    grain = 1 << max(12, need.bit_length() - 4)
    return -(-need // grain) * grain


def test_capacity_lookup_order_camera_then_shape_then_first_sight():
    spec = types.SimpleNamespace(hint={}, cam_hint={}, pending={})
    W, H, cam = 640, 480, b"camera"
    assert R._capacity_for(160_001) == _capacity_by_hand(160_001) == 196_608
    # nothing known: the staged path — or the 4 P bound where a first sight may launch (model path, no host read)
    assert C.lookup(spec, 5000, W, H, cam) is None and C.lookup(spec, 5000, W, H, cam, True) is None
    assert C.lookup(spec, 5000, W, H, cam, False, True) == C.first_sight_capacity(5000) == _capacity_by_hand(20_000) == 28_672
    # an unknown camera falls back to the shape's entry (whatever the mode), and only at this Gaussian count
    spec.hint[(5000, W, H)] = 77_777
    assert C.lookup(spec, 5000, W, H, cam) == C.lookup(spec, 5000, W, H, cam, True, True) == C.lookup_shape(spec, 5000, W, H) == 77_777
    assert C.lookup(spec, 5001, W, H, cam) is None and C.lookup_shape(spec, 5001, W, H) is None
    # a known camera at the same P: its stored capacity, before the shape's
    spec.cam_hint[(W, H, cam)] = (100_000, 80_000, 5000)
    assert C.lookup(spec, 5000, W, H, cam) == 100_000
    assert C.lookup(spec, 5000, W, H, b"another") == 77_777 and C.lookup(spec, 5000, W + 16, H, cam) is None
    # at a changed P: the last count rescaled by the ratio of the Gaussian counts (no shape entry at that P is needed)
    assert C.lookup(spec, 10_000, W, H, cam) == _capacity_by_hand(int(80_000 * 10_000 / 5000) + 1) == 196_608
    assert C.lookup(spec, 2500, W, H, cam) == _capacity_by_hand(int(80_000 * 2500 / 5000) + 1) == 49_152
    # capturing: at least the 1.25x form, never below what the camera already has
    assert C.lookup(spec, 5000, W, H, cam, True) == _capacity_by_hand(int(80_000 * 5000 / 5000 * 1.25) + 1) == 122_880
    assert C.lookup(spec, 10_000, W, H, cam, True) == _capacity_by_hand(int(80_000 * 10_000 / 5000 * 1.25) + 1) == 229_376
    spec.cam_hint[(W, H, cam)] = (400_000, 80_000, 5000)
    assert C.lookup(spec, 5000, W, H, cam, True) == 400_000
    assert spec.hint == {(5000, W, H): 77_777} and spec.cam_hint == {(W, H, cam): (400_000, 80_000, 5000)}      # a look-up writes nothing


def test_capacity_commit_orders_and_bounds_both_tables():
    spec = types.SimpleNamespace(hint={}, cam_hint={}, pending={})
    W, H = 640, 480
    for i in range(3):
        C.commit(spec, 5000, W, H, i, 100_000 + i, 80_000 + i)
    assert list(spec.cam_hint) == [(W, H, 0), (W, H, 1), (W, H, 2)] and spec.hint == {(5000, W, H): 100_002}
    C.commit(spec, 6000, W, H, 0, 120_000, 90_000)               # the camera's entry moves to the recently-used end
    assert list(spec.cam_hint) == [(W, H, 1), (W, H, 2), (W, H, 0)] and spec.cam_hint[(W, H, 0)] == (120_000, 90_000, 6000)
    assert spec.hint == {(5000, W, H): 100_002, (6000, W, H): 120_000}
    C.forget(spec, 6000, W, H, 0)                                # the bound no longer fits the tile-first binning: both entries go
    assert list(spec.cam_hint) == [(W, H, 1), (W, H, 2)] and spec.hint == {(5000, W, H): 100_002}
    C.forget(spec, 6000, W, H, 0)                                # (nothing there: nothing happens)
    # 1 024 entries are kept as they are; with 1 025 present the 128 oldest go — never the one just written, although it was the oldest
    spec.cam_hint = {(W, H, i): (1, 1, 5000) for i in range(1024)}
    spec.hint = {(i, W, H): 1 for i in range(1023)}
    C.commit(spec, 5000, W, H, 0, 2, 2)
    assert len(spec.cam_hint) == 1024 and len(spec.hint) == 1024 and list(spec.cam_hint)[0] == (W, H, 1)
    spec.cam_hint[(W, H, 1024)] = (1, 1, 5000)
    C.commit(spec, 5001, W, H, 1, 3, 3)
    assert list(spec.cam_hint) == [(W, H, i) for i in range(130, 1024)] + [(W, H, 0), (W, H, 1024), (W, H, 1)]
    assert spec.cam_hint[(W, H, 1)] == (3, 3, 5001) and spec.cam_hint[(W, H, 0)] == (2, 2, 5000)
    assert list(spec.hint) == [(i, W, H) for i in range(128, 1023)] + [(5000, W, H), (5001, W, H)] and spec.hint[(5001, W, H)] == 3
    # a settled count writes through the same function: the camera's entry ends up last, the tables stay bounded
    w = R._CountWord()
    w.slot, w.np, w.ptr, w.cap, w.P, w.key, w.device_index, w.captured = 0, None, 0, 100_000, 5000, (W, H, 500), 0, False
    spec.cam_hint.update({(W, H, i): (1, 1, 5000) for i in range(2000, 2128)})
    assert len(spec.cam_hint) == 1025
    R._settle_word(spec, w, 80_000)
    assert len(spec.cam_hint) == 897 and list(spec.cam_hint)[-1] == (W, H, 500) and list(spec.cam_hint)[0] == (W, H, 258)
    assert spec.cam_hint[(W, H, 500)] == (100_000, 80_000, 5000) and spec.hint[(5000, W, H)] == 100_000
    # the staged forward's update knows a count and no camera: first the head-room formula, then kept while the count fits
    spec = types.SimpleNamespace(hint={}, cam_hint={}, pending={})
    C.commit_shape(spec, 5000, W, H, 160_001)
    assert spec.hint == {(5000, W, H): 196_608} and spec.cam_hint == {}
    C.commit_shape(spec, 5000, W, H, 170_000)
    assert spec.hint == {(5000, W, H): 196_608}
    C.commit_shape(spec, 5000, W, H, 196_608)
    assert spec.hint == {(5000, W, H): _capacity_by_hand(196_608)} and spec.hint[(5000, W, H)] > 196_608 * 9 // 8


def test_camera_identity_without_a_device_read():
    a, b = torch.eye(4), torch.eye(4)
    b[3, 2] = 1.5
    assert R._camera_key(a) == R._camera_key(a.clone()) != R._camera_key(b)      # host memory: the content itself
    assert len(R._CAM_KEYS) == 0 or all(not isinstance(k, bytes) for k in R._CAM_KEYS)
    R.tag_camera(b, ("scene", 7))
    assert R._camera_key(b) == b"id:('scene', 7)"
    assert R._camera_key(None) == b""


def test_model_path_maps_the_reference_models_attribute_names():
    """scene/gaussian_model.py:452-468 keeps `_zval`, `_features_dc`, ... with a leading underscore and the background set without;
    a model without a background set gets empty stand-ins; on the CPU the model path declines (render() takes the getters)."""
    sc = syn.make_scene(50, 64, 48)
    m = syn.make_raw_model(sc, ray_fraction=1.0)
    ref_like = types.SimpleNamespace(**{"_" + k: getattr(m, k) for k in ("zval", "rayo", "rayd", "features_dc", "features_rest",
                                                                          "opacity", "scaling", "rotation")})
    t = mp.tensors_of(ref_like)
    assert t is not None and t["zval"] is m.zval and t["bg_xyz"].shape == (0, 3) and t["bg_features_rest"].shape == (0, 15, 3)
    assert tuple(t) == mp.ARG_NAMES
    assert mp.tensors_of(types.SimpleNamespace(_zval=m.zval)) is None           # not a Gaussian model
    assert not mp.supported(t)                                                   # CPU tensors: no kernels for them
    assert mp.model_for(m) is None and mp.model_for(ref_like) is None
    bad = dict(t, scaling=t["scaling"].double())
    assert not mp.supported(bad)


def test_counter_summary_keeps_the_degrees_apart(tmp_path, monkeypatch):
    """tools/pmc_summary.py `<dirs> <dirs>@deg0`: the second collection's workloads are stored as S2_deg0 — the kernels carry
    the same names at every degree, so they must never be averaged into the headline workload's entry."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary as ps

    def collection(d, fetch_kib):
        p = d / "p1"
        p.mkdir(parents=True)
        rows = ["Dispatch_Id,Kernel_Name,Grid_Size,Counter_Name,Counter_Value"]
        for i, (name, grid) in enumerate((("void scg::geometry_hist_kernel<3>(scg::FrameDev)", 262144),
                                          ("void scg::tile_blend_forward_kernel<1536, 1024, 8, 4>(scg::FrameDev)", 774144),
                                          ("scg::blend_backward_kernel(scg::FrameDev)", 774144)), start=1):
            rows.append(f'{i},"{name}",{grid},FETCH_SIZE,{fetch_kib}')
            rows.append(f'{i},"{name}",{grid},WRITE_SIZE,10')
        (p / "c_counter_collection.csv").write_text("\n".join(rows) + "\n")
        return str(d)
    a, b = collection(tmp_path / "pmc", 1000), collection(tmp_path / "pmc_deg0", 400)
    out = tmp_path / "summary.json"
    monkeypatch.setattr(ps, "static_mix", lambda: {})
    monkeypatch.setattr(sys, "argv", ["pmc_summary.py", a, b + "@deg0", "--out", str(out)])
    ps.main()
    import json
    d = json.loads(out.read_text())
    assert d["S2"]["blend_backward"]["hbm_bytes"] == (2 * 1000 + 10) * 1024
    assert d["S2_deg0"]["blend_backward"]["hbm_bytes"] == (2 * 400 + 10) * 1024
    assert d["S2"]["geometry_forward"]["hbm_bytes"] != d["S2_deg0"]["geometry_forward"]["hbm_bytes"]
    assert "kernel_source_sha256" in d["_stamp"]


def _carries(grads, names):
    """Parameters whose .grad are the given views (what autograd leaves behind after a backward)."""
    params = []
    for n in names:
        p = torch.zeros(grads[n].shape, requires_grad=True)
        p.grad = grads[n]
        params.append(p)
    return params


def test_gradient_arena_layout_of_both_paths():
    """One flat arena per backward: every gradient has its parameter's shape and starts on a 16-byte boundary, the large SH
    segments come last, and grad_arena finds the one span again from the .grad tensors alone."""
    P, cpu = 5, torch.device("cpu")
    inputs = (torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 16, 3), None, torch.zeros(P, 3), torch.zeros(P, 4), None)
    out = R._grad_outputs(inputs, None, None, cpu, False)
    names = ("means3D", "opacities", "scales", "rotations", "shs")
    for n, i in zip(names, (0, 1, 4, 5, 2)):
        assert out[n].shape == inputs[i].shape and out[n].storage_offset() % 4 == 0 and out[n].is_contiguous(), n
    assert out["colors_precomp"] is None and out["cov3D_precomp"] is None and out["_pooled"] is None
    assert out["means2D"].shape == (P, 3) and out["means2D"].untyped_storage().data_ptr() != out["shs"].untyped_storage().data_ptr()
    # segments padded to 4 floats: 15 -> 16, 5 -> 8, 15 -> 16, 20, 240; the four small ones in front of the SH segment
    assert [out[n].storage_offset() for n in names] == [0, 16, 24, 40, 60]
    lay = G.layout(tuple((n, out[n].shape) for n in names))
    assert G._take_arena("tensors", lay, lay[3], cpu, False)[0].numel() == 300
    assert lay == (names, [16, 8, 16, 20, 240], ((P, 3), (P, 1), (P, 3), (P, 4), (P, 16, 3)), 300)
    assert out["shs"].untyped_storage().nbytes() == 4 * 300
    assert G.layout(tuple((n, out[n].shape) for n in names)) is lay                  # looked up, not rebuilt
    assert G.layout(()) == ((), [], (), 4)
    params = _carries(out, names)
    assert R.grad_arena(params).numel() == 300 and R.grad_arena(params[:4]).numel() == 60
    assert R.grad_arena(params).untyped_storage().data_ptr() == out["shs"].untyped_storage().data_ptr()
    # the model path, a model without a background set: the non-empty tensors in _ARENA_ORDER, features_rest last
    m = syn.make_raw_model(syn.make_scene(P, 64, 48), ray_fraction=1.0)
    args = mp._ModelArgs(mp.tensors_of(m))
    g = mp._grad_arena(args, None)
    mnames = ("zval", "opacity", "scaling", "rotation", "features_dc", "features_rest")
    assert tuple(n for n in g if not n.startswith("_")) == mnames and g["_c"] is not None
    for n in mnames:
        assert g[n].shape == getattr(m, n).shape and g[n].storage_offset() % 4 == 0, n
    assert [g[n].storage_offset() for n in mnames] == [0, 8, 16, 32, 52, 68]
    assert g["features_rest"].untyped_storage().nbytes() == 4 * (68 + P * 45 + 3)      # 225 floats in a 228-float segment
    mparams = _carries(g, mnames)
    assert R.grad_arena(mparams).numel() == 68 + P * 45 and R.grad_arena(mparams[:5]).numel() == 67


def test_gradient_arena_pool_keeps_two_layouts_and_never_hands_out_an_arena_in_use():
    cpu, path = torch.device("cpu"), "pool-test"

    def take(key):
        arena, pa = G._take_arena(path, key, 8, cpu)
        assert pa is not None and pa.arena is arena
        return pa, arena[:4]                                     # a view, as autograd keeps one as .grad
    assert G._take_arena(path, "A", 8, cpu, False)[1] is None and (path, None) not in G._ARENA_POOLS      # the switch is off
    a, view = take("A")
    a2, view2 = take("A")                                        # the first one's view is alive: another arena
    assert a2 is not a and a2.storage.data_ptr() != a.storage.data_ptr()
    view = None
    a3, view3 = take("A")                                        # released: handed out again, the one still in use is not
    assert a3 is a
    held = G._ARENA_POOLS[(path, None)]                          # [(layout, arenas)], least recently used first
    assert held == [("A", [a, a2])]
    gone = weakref.ref(a.arena)
    a = a2 = a3 = view2 = view3 = None
    b, view_b = take("B")
    assert [k for k, _ in held] == ["A", "B"]
    c, view_c = take("C")                                        # a third layout: the least recently used one's arenas go
    assert held == [("B", [b]), ("C", [c])] and gone() is None
    take("B")                                                    # use moves a layout to the recently-used end
    take("D")
    assert [k for k, _ in held] == ["B", "D"] and len(held[0][1]) == 2      # (b is still referenced by view_b: a second arena)
    held_keeps = [take("D") for _ in range(5)]                   # the caller keeps these gradients: never the same arena twice,
    assert len({pa.storage.data_ptr() for pa, _ in held_keeps}) == 5 and len(held[1][1]) == G._ARENA_POOL_DEPTH    # bounded
    del G._ARENA_POOLS[(path, None)]


def test_sh_tail_promise_is_decided_before_and_recorded_after_the_launch():
    cpu = torch.device("cpu")
    arena, pa = G._take_arena("promise-test", "L", 64, cpu)
    try:
        assert R._sh_tail_promise(None, 1) == 0                  # not pooled: nothing is known
        assert R._sh_tail_promise(pa, 1) == 0                    # a fresh arena: the kernel writes the zeros
        assert R._sh_tail_promise(pa, 1) == 0                    # ... deciding records nothing
        G.commit_promise(pa, 4, False)
        assert R._sh_tail_promise(pa, 4) == 2 and R._sh_tail_promise(pa, 9) == 2 and R._sh_tail_promise(pa, 16) == 2
        assert R._sh_tail_promise(pa, 1) == 0                    # a lower degree: coefficients 1-3 hold old values
        arena[:8].mul_(1.0)                                      # a torch write through a view: the promise is off
        assert R._sh_tail_promise(pa, 4) == 0
        G.commit_promise(pa, 4, False)
        assert R._sh_tail_promise(pa, 4) == 2
        # the failed-launch path: decided, the library call raised, no commit
        assert R._sh_tail_promise(pa, 4) == 2
        G.invalidate_promise(pa)
        assert R._sh_tail_promise(pa, 4) == 0 and R._sh_tail_promise(pa, 16) == 0
        G.commit_promise(pa, 16, True)                           # adding to an arena nobody knows anything about: still nothing
        assert R._sh_tail_promise(pa, 16) == 0
        # views of mixed degree in one step: the first WRITES at degree 0, the second ADDS at degree 1
        G.commit_promise(pa, 1, False)
        G.commit_promise(pa, 4, True)
        assert R._sh_tail_promise(pa, 1) == 0 and R._sh_tail_promise(pa, 4) == 2
        G.commit_promise(pa, 1, True)                            # a lower-degree view adds: the zeros stay where they begin
        assert R._sh_tail_promise(pa, 1) == 0 and R._sh_tail_promise(pa, 4) == 2
        arena[:8].mul_(1.0)
        G.commit_promise(pa, 4, True)                            # a torch write between two views of a step: unknown from here on
        assert R._sh_tail_promise(pa, 16) == 0
        G.invalidate_promise(None)
        G.commit_promise(None, 1, False)
    finally:
        del G._ARENA_POOLS[("promise-test", None)]


def _hand_built_word(slot, value, cap=100_000, device_index=977):
    """A _CountWord over a one-element numpy word (no pinned memory); device 977 is nobody's: its state is the test's own."""
    import numpy as np
    w = C._CountWord()
    w.slot, w.np, w.ptr, w.cap, w.P, w.key, w.device_index, w.captured = \
        slot, np.array([value], dtype=np.uint32), 0, cap, 5000, (640, 480, b"camera"), device_index, False
    return w


def test_capture_record_nests_and_restores_the_outer_list():
    spec = types.SimpleNamespace(pending={})
    outer_before = C._CAPTURE_RECORD
    anon_before, renders = list(C._ANON_CAPTURED), C._OVERFLOW["renders"]
    a, b, c = (_hand_built_word(i, C._COUNT_ARMED) for i in range(3))
    with C.capture_record() as outer:
        assert outer == [] and C._CAPTURE_RECORD is outer
        C.file_word(spec, a, a.key, True)
        with C.capture_record() as inner:
            assert inner == [] and inner is not outer and C._CAPTURE_RECORD is inner
            C.file_word(spec, b, b.key, True)
        assert C._CAPTURE_RECORD is outer
        with pytest.raises(ZeroDivisionError):
            with C.capture_record():
                raise ZeroDivisionError
        assert C._CAPTURE_RECORD is outer
        C.file_word(spec, c, c.key, False)                       # not captured: the camera's next render looks at it
    assert C._CAPTURE_RECORD is outer_before
    assert outer == [a] and inner == [b] and a.captured and b.captured and not c.captured
    assert spec.pending == {c.key: [c]} and C._ANON_CAPTURED == anon_before and C._OVERFLOW["renders"] == renders + 3


def test_release_puts_each_slot_back_once():
    free_before = list(C._COUNT_FREE)
    try:
        C.release([_hand_built_word(s, 0) for s in (900_001, 900_002, 900_003)])
        assert C._COUNT_FREE == free_before + [900_001, 900_002, 900_003]
        C.release([])
        assert C._COUNT_FREE == free_before + [900_001, 900_002, 900_003]
    finally:
        C._COUNT_FREE[:] = free_before


def test_settle_replayed_rearms_the_word_and_settles_the_count():
    spec = C._SPEC_STATE[977] = types.SimpleNamespace(hint={}, cam_hint={}, pending={})
    try:
        before = dict(C._OVERFLOW)
        w = _hand_built_word(0, C._COUNT_ARMED)
        assert C.settle_replayed(w) is None                      # armed: nothing has arrived, nothing is touched
        assert C._OVERFLOW == before and int(w.np[0]) == C._COUNT_ARMED and spec.cam_hint == {} and spec.hint == {}
        w.np[0] = 80_000                                         # a count within the capacity
        assert C.settle_replayed(w) == 80_000
        assert int(w.np[0]) == C._COUNT_ARMED and w.value() is None
        assert C._OVERFLOW["settled"] == before["settled"] + 1 and C._OVERFLOW["overflows"] == before["overflows"]
        assert spec.cam_hint[w.key] == (100_000, 80_000, 5000)
        w.np[0] = 150_000                                        # beyond it: counted, and the camera has room for it next time
        assert C.settle_replayed(w) == 150_000
        assert int(w.np[0]) == C._COUNT_ARMED
        assert C._OVERFLOW["settled"] == before["settled"] + 2 and C._OVERFLOW["overflows"] == before["overflows"] + 1
        assert spec.cam_hint[w.key][0] >= 150_000 + 150_000 // 8 and spec.cam_hint[w.key][1:] == (150_000, 5000)
        assert C._OVERFLOW["renders"] == before["renders"]
    finally:
        del C._SPEC_STATE[977]
