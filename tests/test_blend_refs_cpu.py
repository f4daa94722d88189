"""tests/blend_refs.py is right, without a GPU: its fp64 forward against the oracle's blend on every planted frame, its fp64 raw
sums (mapped to derivatives as include/scg_raster.h says) against the oracle's autograd, the decision margin, the coverage of
the edge classes and the validity of the launch-order tables."""
import numpy as np
import pytest
import torch

import blend_refs as B
from oracle import torch_rasterizer as orc

ORACLE_FRAMES = B.BASE_FRAMES + B.EXTRA_FRAMES
FP32_AGREES = 3e-5        # of the sum of absolute terms: above the worst e32 of the frames (1.7e-5 where 1 - alpha amplifies the
                          # rounding of an alpha next to 0.99 a hundredfold), three orders below any error of formulation


def _oracle(fr, grad=False):
    sp = torch.from_numpy(fr.splats)
    leaves = dict(xy=sp[:, 0:2].clone(), conic=sp[:, 2:5].clone(), opacity=sp[:, 5].clone(), rgb=sp[:, 8:11].clone(), depth=sp[:, 11].clone())
    if grad:
        for v in leaves.values():
            v.requires_grad_(True)
    pre = dict(leaves, grid=(fr.gx, fr.gy))
    st = orc.Settings(fr.H, fr.W, 1.0, 1.0, torch.from_numpy(fr.bg), 1.0, None, None, 0, None, False, False)
    out = orc.blend(pre, dict(ranges=fr.ranges, point_list=fr.point_list), st)
    return leaves, out


@pytest.mark.parametrize("key", ORACLE_FRAMES)
def test_fp64_forward_equals_the_oracle_blend(key):
    ref = B.reference(key)
    fr, r64 = ref["frame"], ref["r64"]
    _, (color, depth, alpha, fT, nC) = _oracle(fr)
    assert np.array_equal(nC.numpy().astype(np.int64), r64["n_contrib"])
    for name, got in (("color", color), ("depth", depth[0]), ("alpha", alpha[0]), ("final_T", fT)):
        e = B.normalised_error(got.detach().numpy(), r64[name], r64["norm"][name])
        assert float(e.max()) < FP32_AGREES, (key, name, float(e.max()))


@pytest.mark.parametrize("key", ORACLE_FRAMES)
def test_fp64_raw_sums_mapped_to_derivatives_equal_the_oracle_autograd(key):
    ref = B.reference(key)
    fr, r64 = ref["frame"], ref["r64"]
    leaves, (color, depth, alpha, _, _) = _oracle(fr, grad=True)
    loss = (color * torch.from_numpy(fr.dL_dcolor)).sum() + (depth[0] * torch.from_numpy(fr.dL_ddepth)).sum() + \
        (alpha[0] * torch.from_numpy(fr.dL_dalpha)).sum()
    loss.backward()
    S, A = r64["rec"], r64["rec_abs"]                                   # S_x S_y ddepth S_q S_xx S_xy S_yy dr dg db
    sp = fr.splats.astype(np.float64)
    a, b, c, op = sp[:, 2], sp[:, 3], sp[:, 4], sp[:, 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        want = dict(xy=np.stack([-(a * S[:, 0] + b * S[:, 1]), -(b * S[:, 0] + c * S[:, 1])], 1),
                    conic=np.stack([-S[:, 4] / 2, -S[:, 5], -S[:, 6] / 2], 1),
                    opacity=np.where(op > 0, S[:, 3] / op, 0.0), rgb=S[:, 7:10], depth=S[:, 2])
        norm = dict(xy=np.stack([np.abs(a) * A[:, 0] + np.abs(b) * A[:, 1], np.abs(b) * A[:, 0] + np.abs(c) * A[:, 1]], 1),
                    conic=np.stack([A[:, 4] / 2, A[:, 5], A[:, 6] / 2], 1),
                    opacity=np.where(op > 0, A[:, 3] / op, 0.0), rgb=A[:, 7:10], depth=A[:, 2])
    assert float(np.abs(want["xy"]).max()) > 0
    for k, v in leaves.items():
        g = v.grad.numpy()
        assert np.isfinite(g).all(), (key, k)
        e = B.normalised_error(g, want[k], norm[k])
        assert float(e.max()) < FP32_AGREES, (key, k, float(e.max()))
    unblended = ~r64["blended_in"].reshape(fr.P, -1).any(1)
    assert unblended.any() or fr.P < 5
    assert not np.abs(S[unblended]).any()


@pytest.mark.parametrize("key", B.ALL_FRAMES)
def test_fp32_restatements_take_the_decisions_of_fp64_on_every_pixel_and_entry(key):
    ref = B.reference(key)
    assert ref["same_decisions"], key
    for v in ref["e32"].values():
        assert np.isfinite(v) and v < FP32_AGREES


def test_planted_threshold_pairs_sit_one_part_in_a_thousand_either_side():
    """The pairs either side of 1/255, 0.99 and 1e-4: on either side a (pixel, entry) lies between 0.5e-3 and 2e-3 (relative) from
    the threshold.  Nothing but the members planted ON a threshold (opacity 1/255: a class of their own) comes nearer than 1e-6,
    sixteen fp32 roundings — the nearest is the stack of clamped splats, (1 - 0.99f)^2 = 1e-4f (1 - 1.9e-6), whose fp32 evaluation
    is one exact subtraction and one rounded product."""
    for key, name, thr in (("c", "oG", float(B.A_MIN)), ("c", "oG", float(B.A_MAX)), ("d", "tt", float(B.T_EPS))):
        r64 = B.reference(key)["r64"]
        rels = []
        for tl in r64["tiles"]:
            if tl["n"]:
                ins = tl["inside"]
                v = tl["oG"][ins] if name == "oG" else (tl["T_before"] * (1 - tl["alpha"]))[ins]
                asked = tl["tge0"][ins] & (tl["age"][ins] if name == "tt" else True)
                rels.append(((v[asked] - thr) / thr).ravel())
        rel = np.concatenate(rels)
        rel = rel[rel != 0]
        assert ((rel > 0.5 * B.REL) & (rel < 2 * B.REL)).any() and ((-rel > 0.5 * B.REL) & (-rel < 2 * B.REL)).any(), (key, name)
        assert np.abs(rel).min() > 1e-6, (key, name, np.abs(rel).min())
    stack = (1 - float(B.A_MAX)) ** 2
    assert stack < float(B.T_EPS) and (float(B.T_EPS) - stack) / float(B.T_EPS) > 1e-6


def test_every_edge_class_occurs_in_an_in_image_quadrant():
    total = {}
    for key in ORACLE_FRAMES:
        ref = B.reference(key)
        for k, v in B.coverage(ref["frame"], ref["r64"]).items():
            total[k] = total.get(k, 0) + v
    missing = [k for k in B.REQUIRED if total.get(k, 0) <= 0]
    assert not missing, missing
    # the bit-exact frames are what they must be: one atomic per record
    for key in ("a", "b", "depth_only", "alpha_only", "translation-d", "translation-e") + tuple(f"padding-{k}" for k in (0,) + B.PAD_KS) + \
            tuple(f"phase-{k}" for k in B.PHASE_KS):
        assert B.single_atomic(B.reference(key)), key
    for key in ("c", "d", "e", "e9"):
        assert not B.single_atomic(B.reference(key)), key
    assert all(B.single_atomic(B.reference(key)) for key in B.TWIN_SINGLE_ATOMIC) and set(B.TWIN_SINGLE_ATOMIC) <= set(B.TWIN_FRAMES)
    # the padding frames shift n_contrib and nothing else
    base = B.reference("padding-0")["r64"]
    for k in B.PAD_KS:
        r = B.reference(f"padding-{k}")["r64"]
        got, was = r["n_contrib"][:8, :8], base["n_contrib"][:8, :8]              # (quadrant 0: the pattern; quadrant 3: the sibling copy)
        assert (was > 0).any() and np.array_equal(got > 0, was > 0) and (got[was > 0] >= was[was > 0] + k).all()


def test_frame_sizes_and_limits():
    sizes = {k: (B.frame(k).W, B.frame(k).H, B.frame(k).T) for k in B.BASE_FRAMES}
    # (129 x 17 is 9 x 2 tiles on 24 slots; the 9 tiles on 16 slots of a single row are frame e9, 129 x 16)
    assert sizes == {"a": (1, 1, 1), "b": (8, 8, 1), "c": (16, 16, 1), "d": (40, 25, 6), "e": (129, 17, 18), "e9": (129, 16, 9)}
    for key in B.ALL_FRAMES:
        fr = B.frame(key)
        B.check_frame(fr)
        assert max(len(fr.tile_ids(t)) for t in range(fr.T)) <= 400
        assert fr.splats_for(False)[:, 6].min() == np.inf and np.array_equal(fr.splats_for(False)[:, :6], fr.splats[:, :6])


@pytest.mark.parametrize("key", B.ALL_FRAMES)
def test_order_tables_are_permutations_plus_padding(key):
    fr = B.frame(key)
    per = (fr.T + 7) // 8
    seen = set()
    for order in ("identity", "reversed", "shuffled"):
        w = fr.ranges_words(order, seed=3)
        assert w.dtype == np.uint32 and len(w) == 2 * fr.T + 40 * per
        B.check_order_tables(w, fr.T)
        assert np.array_equal(w[:2 * fr.T].reshape(-1, 2), fr.ranges)
        seen.add(w[2 * fr.T:].tobytes())
    assert len(seen) == (3 if fr.T > 2 else len(seen))
    with pytest.raises(AssertionError):                                 # the check itself: a table with a tile twice is refused
        bad = fr.ranges_words().copy()
        bad[2 * fr.T + 8 * per] = bad[2 * fr.T + 8 * per + 1]
        B.check_order_tables(bad, fr.T)
