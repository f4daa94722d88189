"""The blend stage ALONE (csrc/blend.hip): scg_blend_forward and scg_blend_backward called directly on the frames of
tests/blend_refs.py — splat records, tile lists, launch-order tables and upstream gradients of the test's own making, a list entry
exactly where the kernels branch (chunk, flush, cull, termination and image edges).

Held to fp64 through loss_refs.held_to, per frame and output: err = max |hip - r64| / (sum of the absolute terms of the
element) <= max(4 e32, 1e-6), e32 the larger of two independent fp32 evaluations' errors (the kernel's formulation; cumprod and
suffix sums); n_contrib equals the reference exactly; no pixel is left out.  Everything else is equality of BITS: the arithmetic
of a hit does not depend on where in the list, the tile or the image it sits, and on the frames whose every Gaussian is blended
in one quadrant only each gradient record receives a single atomic, so the records have no summation order either."""
import numpy as np
import pytest

import blend_refs as B
import loss_refs as LR

pytestmark = pytest.mark.gpu

HELD = B.BASE_FRAMES + B.EXTRA_FRAMES
SINGLE = ("a", "b", "depth_only", "alpha_only", "translation-d", "translation-e", "padding-0", "padding-64")
UNUSED = tuple(k for k in range(16) if k not in B.USED)


def _hold(tag, out, ref):
    """The five forward outputs and every used component of every record against fp64; the exact statements."""
    fr, r64, e32 = ref["frame"], ref["r64"], ref["e32"]
    assert np.array_equal(out["n_contrib"].astype(np.int64), r64["n_contrib"]), tag
    for k in ("color", "depth", "alpha", "final_T"):
        e = B.normalised_error(out[k], r64[k], r64["norm"][k])
        LR.held_to(f"blend {tag} {k}", float(e.max()), e32[k], LR.GRAD_FLOOR, elements=e.size)
    ds = out["dsplats"]
    assert np.isfinite(ds).all(), tag
    assert not ds[:, UNUSED].any(), tag                                           # slots [7], [11..15]: cleared, never written
    unblended = ~r64["blended_in"].reshape(fr.P, -1).any(1)
    assert not ds[unblended].any(), tag                                           # nobody blends it: exactly 0
    for j, name in enumerate(B.REC_NAMES):
        e = B.normalised_error(ds[:, B.USED[j]], r64["rec"][:, j], r64["rec_abs"][:, j])
        LR.held_to(f"blend {tag} {name}", float(e.max()), e32[name], LR.GRAD_FLOOR, elements=e.size)


def _same_forward(a, b, tag):
    for k in B.FORWARD_OUTPUTS:
        assert np.array_equal(a[k], b[k]), (tag, k)


def _same_records(a, b, tag):
    assert np.array_equal(a["dsplats"], b["dsplats"]), tag


@pytest.mark.parametrize("cull", [True, False], ids=["cull", "cull_off"])
@pytest.mark.parametrize("key", HELD)
def test_both_directions_hold_every_edge_class_to_fp64(key, cull):
    ref = B.reference(key)
    assert ref["same_decisions"]
    _hold(f"{key} {'cull' if cull else 'cull off'}", B.run_staged(ref["frame"], cull=cull), ref)


@pytest.mark.parametrize("key", HELD + ("translation-d", "padding-64"))
def test_cull_fields_never_enter_a_blended_value(key):
    """cull_thr = +inf (every quadrant walks every entry) against the true cull fields: the forward outputs bit for bit on every
    frame, the records bit for bit where they receive a single atomic (elsewhere both runs are held to fp64 above)."""
    ref = B.reference(key)
    on, off = B.run_staged(ref["frame"], cull=True), B.run_staged(ref["frame"], cull=False)
    _same_forward(on, off, key)
    if B.single_atomic(ref):
        _same_records(on, off, key)


@pytest.mark.parametrize("key", HELD + ("translation-d", "translation-e"))
def test_launch_order_never_enters_a_result(key):
    ref = B.reference(key)
    base = B.run_staged(ref["frame"], order="identity")
    for order in ("reversed", "shuffled"):
        out = B.run_staged(ref["frame"], order=order, order_seed=11)
        _same_forward(base, out, (key, order))
        if B.single_atomic(ref):
            _same_records(base, out, (key, order))
        else:
            _hold(f"{key} order {order}", out, ref)


@pytest.mark.parametrize("key", ["d", "e"])
def test_translated_copies_of_a_pattern_give_the_same_bits(key):
    """The same pattern, upstream gradients included, in every quadrant of every tile: every in-image pixel of every copy
    equals the copy in tile 0, quadrant 0, and so do the records of every member whose blending pixels are all in the image."""
    ref = B.reference(f"translation-{key}")
    fr, r64 = ref["frame"], ref["r64"]
    assert B.single_atomic(ref)
    out = B.run_staged(fr)
    _hold(f"translation-{key}", out, ref)
    ids0 = fr.copy_ids[(0, 0)]
    # the pixels that blend member j of copy (0, 0), as an 8 x 8 mask
    tl = r64["tiles"][0]
    q0 = tl["quad"] == 0
    masks = [tl["contrib"][q0][:, list(tl["ids"]).index(i)].reshape(8, 8) for i in ids0]
    assert sum(m.any() for m in masks) >= 11
    compared = partial = 0
    for (t, q), ids in fr.copy_ids.items():
        x0, y0 = 16 * (t % fr.gx) + 8 * (q & 1), 16 * (t // fr.gx) + 8 * (q >> 1)
        w, h = max(0, min(8, fr.W - x0)), max(0, min(8, fr.H - y0))
        if w == 0 or h == 0:
            assert not out["dsplats"][ids].any()
            continue
        for k in B.FORWARD_OUTPUTS:
            a, b = out[k][..., y0:y0 + h, x0:x0 + w], out[k][..., 0:h, 0:w]
            if k == "n_contrib":                                                   # list positions differ from copy to copy: the MEMBER is the same
                la, l0 = list(fr.tile_ids(t)), list(fr.tile_ids(0))
                a = np.array([[ids.index(la[v - 1]) if v else -1 for v in row] for row in a])
                b = np.array([[ids0.index(l0[v - 1]) if v else -1 for v in row] for row in b])
            assert np.array_equal(a, b), (t, q, k)
        partial += (w, h) != (8, 8)
        for j, m in enumerate(masks):
            if not m[h:, :].any() and not m[:, w:].any():                         # all of its blending pixels are in the image
                assert np.array_equal(out["dsplats"][ids[j]], out["dsplats"][ids0[j]]), (t, q, j)
                compared += 1
    assert partial > 0 and compared > 13 * (fr.T - 1)


@pytest.mark.parametrize("k", B.PAD_KS)
def test_list_padding_changes_n_contrib_and_nothing_else(k):
    """k padding entries in front of the list and padding interleaved between the hits — entries that fail the cull, entries that
    pass it and blend nowhere, entries that blend in a sibling quadrant only: images, final_T and the pattern's records keep
    their bits, n_contrib is the reference's."""
    base_ref, ref = B.reference("padding-0"), B.reference(f"padding-{k}")
    base, out = B.run_staged(base_ref["frame"]), B.run_staged(ref["frame"])
    _hold(f"padding-{k}", out, ref)
    for name in ("color", "depth", "alpha", "final_T"):
        assert np.array_equal(out[name][..., :8, :8], base[name][..., :8, :8]), (k, name)
    assert np.array_equal(out["n_contrib"].astype(np.int64), ref["r64"]["n_contrib"])
    assert not np.array_equal(out["n_contrib"], base["n_contrib"])
    ids = ref["frame"].pattern_ids
    assert ids == base_ref["frame"].pattern_ids
    assert np.array_equal(out["dsplats"][ids], base["dsplats"][ids]) and base["dsplats"][ids].any()
    off = B.run_staged(ref["frame"], cull=False)                                   # ... and every padding entry walked
    _same_forward(out, off, k)
    _same_records(out, off, k)


@pytest.mark.parametrize("k", B.PHASE_KS)
def test_a_member_sums_the_same_bits_in_every_row_and_flush_of_the_block(k):
    """k more blended entries in the quadrant's list, on pixels the pattern does not reach: the pattern's members move k rows in
    the backward's four-row block (12 blended entries are three full flushes; 12 + k end in a partial one, which is the
    compiler's code in the hand-written walk too) — their records and every pixel they touch keep their bits."""
    base_ref, ref = B.reference("padding-0"), B.reference(f"phase-{k}")
    assert B.single_atomic(ref)
    base, out = B.run_staged(base_ref["frame"]), B.run_staged(ref["frame"])
    _hold(f"phase-{k}", out, ref)
    ids = ref["frame"].pattern_ids
    blended = [int(base_ref["r64"]["blended_in"][i].any()) for i in ids]
    assert sum(blended) == 12 and int(ref["r64"]["blended_in"].any((1, 2)).sum()) == 12 + k
    touched = base["n_contrib"] > 0
    for name in ("color", "depth", "alpha", "final_T"):
        assert np.array_equal(out[name][..., touched], base[name][..., touched]), (k, name)
    assert np.array_equal(out["dsplats"][ids], base["dsplats"][ids]), k


@pytest.mark.parametrize("key", ["b", "translation-d", "depth_only", "alpha_only"])
def test_a_missing_upstream_is_a_zero_upstream(key):
    """dL_ddepth = NULL against a zero tensor, dL_dalpha = NULL against a zero tensor (single-atomic frames: the records too)."""
    ref = B.reference(key)
    fr = ref["frame"]
    assert B.single_atomic(ref)
    full = B.run_staged(fr)
    for which in ("depth", "alpha"):
        null, zero = B.run_staged(fr, **{which: None}), B.run_staged(fr, **{which: "zero"})
        _same_forward(null, zero, (key, which))
        _same_records(null, zero, (key, which))
        _same_forward(null, full, (key, which))
        carries = getattr(fr, "dL_d" + which).any()
        assert np.array_equal(null["dsplats"], full["dsplats"]) != bool(carries), (key, which)   # premise: the upstream matters where it is not zero


@pytest.mark.parametrize("key", ["b", "translation-e", "padding-127"])
def test_clearing_the_records(key):
    """dsplats_zero handed to the forward, then prezeroed = 1, equals prezeroed = 0 on a NaN-filled buffer; prezeroed = 1 on a
    buffer holding a known finite pattern equals pattern + result (one atomic per record: one fp32 addition per element)."""
    ref = B.reference(key)
    fr = ref["frame"]
    assert B.single_atomic(ref)
    memset, by_forward = B.run_staged(fr, clear="memset"), B.run_staged(fr, clear="forward")
    _same_forward(memset, by_forward, key)
    _same_records(memset, by_forward, key)
    prior = np.random.default_rng(9).standard_normal((fr.P, 16)).astype(np.float32)
    added = B.run_staged(fr, clear="prefill", prefill=prior)
    assert np.array_equal(added["dsplats"], prior + memset["dsplats"])
    assert memset["dsplats"].any() and np.array_equal(added["dsplats"][:, UNUSED], prior[:, UNUSED])


@pytest.mark.parametrize("clear, costs", [("memset", False), ("forward", False), ("memset", True)], ids=["memset", "by_forward", "costs"])
def test_what_the_buffers_held_before_the_calls_changes_no_bit(clear, costs):
    """The runner starts every buffer the two calls write or add into from ONE pattern (NaN; -1).  The binding's come from
    torch.empty: here they start from the two fills of tests/guarded_alloc.py, per way of clearing the records and with the cost
    words on, and every output must come out with the same bits — a record that is added to before it was cleared, a pixel or a
    cost word that is left as it was, differs.  (Single-atomic frames: the records' sums have no order.)"""
    import guarded_alloc as G
    for key in ("b", "translation-e", "padding-127"):
        ref = B.reference(key)
        fr = ref["frame"]
        assert B.single_atomic(ref)
        a, b = (B.run_staged(fr, clear=clear, costs=costs, start=fill) for fill in (G.FILL_A, G.FILL_B))
        plain = B.run_staged(fr, clear=clear, costs=costs)
        assert a.keys() == b.keys() == plain.keys()
        for k in a:
            assert G.same_bits(a[k], b[k]) and G.same_bits(a[k], plain[k]), (key, clear, costs, k)


@pytest.mark.parametrize("key", B.BASE_FRAMES + ("padding-127",))
def test_cost_hints_count_what_the_walks_do(key):
    """With the cull switched off every quadrant walks every entry until all its pixels have terminated: tile_cost_out[t] is the
    list length of t (whole chunks up to the one in which the busiest quadrant's last pixel terminates), bwd_cost_out[4 t + q] the
    quadrant's highest n_contrib; neither changes a result."""
    ref = B.reference(key)
    fr = ref["frame"]
    out, plain = B.run_staged(fr, cull=False, costs=True), B.run_staged(fr, cull=False)
    tile_cost, bwd_cost = B.expected_costs(fr, ref["r64"])
    assert np.array_equal(out["tile_cost"].astype(np.int64), tile_cost), key
    assert np.array_equal(out["bwd_cost"].astype(np.int64), bwd_cost), key
    lens = (fr.ranges[:, 1] - fr.ranges[:, 0]).astype(np.int64)
    untouched = [t for t in range(fr.T) if tile_cost[t] == lens[t]]
    assert len(untouched) >= fr.T - 1                                              # (frame e: quadrant 0 of tile 3 terminates — its siblings walk on)
    _same_forward(out, plain, key)
    if B.single_atomic(ref):
        _same_records(out, plain, key)
