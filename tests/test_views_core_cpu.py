"""The K-view core of the four autograd nodes (rasterizer._views_backward) and the modules' argument check (_exactly_one_of), without a
GPU: rasterizer._backward_view is replaced with a stub that records its arguments and writes ones into the d_means2D_out it is given.
Every run is under guarded_alloc.guarded(FILL_A, devices=("cpu",)): the (K, P, 3) buffer starts from NaNs, so a slot that nobody
wrote shows."""
import types

import pytest
import torch

import guarded_alloc as GA
from scgaussian_amd import model_path as mp
from scgaussian_amd import rasterizer as R

P = 5
NAMES = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


@pytest.fixture
def calls(monkeypatch):
    """The stub in place of rasterizer._backward_view; yields the list of its calls' arguments."""
    seen = []

    def stub(state, inputs, radii, dL_dcolor, dL_ddepth, dL_dalpha, timer=None, into=None, d_means2D_out=None,
             want_dsplats=False):
        seen.append(dict(state=state, inputs=inputs, radii=radii, grads=(dL_dcolor, dL_ddepth, dL_dalpha), into=into,
                         d_means2D_out=d_means2D_out))
        if d_means2D_out is not None:
            d_means2D_out.fill_(1.0)
        if into is not None:
            return into
        out = {n: None for n in NAMES + mp.ARG_NAMES}
        out["means3D"] = torch.zeros(P, 3)
        out["means2D"] = d_means2D_out if d_means2D_out is not None else torch.full((P, 3), 7.0)
        seen[-1]["returned"] = out
        return out

    monkeypatch.setattr(R, "_backward_view", stub)
    with GA.guarded(GA.FILL_A, devices=("cpu",)):
        yield seen


def _tensor_inputs():
    return (torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 16, 3), None, torch.zeros(P, 3), torch.zeros(P, 4), None)


def _model_inputs():
    return types.SimpleNamespace(device=torch.device("cpu"), P=P)


def _tensor_ctx(K):
    inputs = _tensor_inputs()
    radii = tuple(torch.zeros(P, dtype=torch.int32) for _ in range(K))
    return types.SimpleNamespace(states=[{"view": k} for k in range(K)], inputs_present=tuple(t is not None for t in inputs),
                                 saved_tensors=tuple(t for t in inputs if t is not None) + radii,
                                 shapes=(torch.Size((P, 3)), torch.Size((K, P, 3)), torch.Size((P, 16, 3)), torch.Size((P, 1))))


def _model_ctx(K):
    return types.SimpleNamespace(states=[{"view": k} for k in range(K)], model=_model_inputs(),
                                 saved_tensors=tuple(torch.zeros(P, dtype=torch.int32) for _ in range(K)))


@pytest.mark.parametrize("make_inputs", (_tensor_inputs, _model_inputs), ids=("tensors", "model"))
def test_a_view_without_gradients_is_skipped_and_its_slot_cleared(calls, make_inputs):
    inputs = make_inputs()
    states = [{"view": k} for k in range(3)]
    radii = [torch.full((P,), k, dtype=torch.int32) for k in range(3)]
    g = [torch.zeros(3, 4, 4), None, torch.zeros(1, 4, 4), None]
    grads = (*g, None, None, None, None, None, None, g[2], None)              # view 1: all three None; view 2: depth only
    acc, d = R._views_backward(states, inputs, radii, grads, True)
    assert [c["state"] for c in calls] == [states[0], states[2]] and len(calls) == 2
    assert calls[0]["radii"] is radii[0] and calls[1]["radii"] is radii[2]
    assert calls[0]["grads"] == (g[0], g[2], None) and calls[1]["grads"] == (None, g[2], None)
    assert all(c["inputs"] is inputs for c in calls)
    assert calls[0]["into"] is None
    assert calls[1]["into"] is calls[0]["returned"] and acc is calls[0]["returned"]
    assert d.shape == (3, P, 3) and d.dtype == torch.float32 and d.is_contiguous()
    for c, k in zip(calls, (0, 2)):
        assert c["d_means2D_out"].data_ptr() == d.data_ptr() + k * P * 3 * 4 and c["d_means2D_out"].shape == (P, 3)
    assert torch.equal(d[1], torch.zeros(P, 3))
    assert torch.equal(d[0], torch.ones(P, 3)) and torch.equal(d[2], torch.ones(P, 3))


def test_no_gradient_at_all_calls_nothing_and_returns_none_everywhere(calls):
    grads = (None,) * 8
    assert R._views_backward([{}, {}], _tensor_inputs(), [None, None], grads, True) == (None, None)
    out = R._RasterizeViews.backward(_tensor_ctx(2), *grads)
    assert out == (None,) * 9
    out = mp._RasterizeModelViews.backward(_model_ctx(2), *grads)
    assert out == (None,) * (len(mp.ARG_NAMES) + 3)
    assert calls == []


def test_the_views_nodes_return_the_core_s_buffer_in_their_argument_order(calls):
    g = torch.zeros(3, 4, 4)
    out = R._RasterizeViews.backward(_tensor_ctx(2), g, None, None, None, None, None, None, None)
    assert len(out) == 9 and out[8] is None and out[0] is calls[0]["returned"]["means3D"]
    assert out[1].shape == (2, P, 3) and torch.equal(out[1][0], torch.ones(P, 3)) and torch.equal(out[1][1], torch.zeros(P, 3))
    out = mp._RasterizeModelViews.backward(_model_ctx(2), None, None, None, None, g, None, None, None)
    assert len(out) == len(mp.ARG_NAMES) + 3 and out[-2:] == (None, None)
    assert torch.equal(out[0][0], torch.zeros(P, 3)) and torch.equal(out[0][1], torch.ones(P, 3))


def test_a_single_view_node_has_no_slot_and_returns_the_view_s_own_means2d(calls):
    state, inputs, radii = {"view": 0}, _tensor_inputs(), torch.zeros(P, dtype=torch.int32)
    gc, gd = torch.zeros(3, 4, 4), torch.zeros(1, 4, 4)
    g, d = R._views_backward([state], inputs, [radii], (gc, None, gd, None), False)
    assert len(calls) == 1 and calls[0]["d_means2D_out"] is None and calls[0]["into"] is None
    assert calls[0]["state"] is state and calls[0]["radii"] is radii and calls[0]["grads"] == (gc, gd, None)
    assert g is calls[0]["returned"] and d is g["means2D"] and torch.equal(d, torch.full((P, 3), 7.0))
    # ... also when nothing reached the loss: the single-view nodes hand the call on as it is
    R._views_backward([state], inputs, [radii], (None,) * 4, False)
    assert len(calls) == 2 and calls[1]["grads"] == (None, None, None) and calls[1]["d_means2D_out"] is None
    # the two nodes: the means2D gradient is the stub's tensor, in the position of the means2D argument
    ctx = _tensor_ctx(1)
    ctx.shapes = ctx.shapes[:1] + (torch.Size((P, 3)),) + ctx.shapes[2:]
    ctx.odd_dtypes, ctx.raster_settings = None, types.SimpleNamespace(debug=False)
    out = R._RasterizeGaussians.backward(ctx, gc, None, None, None)
    assert len(out) == 9 and out[1] is calls[2]["returned"]["means2D"] and calls[2]["d_means2D_out"] is None
    out = mp._RasterizeModel.backward(_model_ctx(1), gc, None, None, None)
    assert len(out) == len(mp.ARG_NAMES) + 3 and out[0] is calls[3]["returned"]["means2D"] and calls[3]["d_means2D_out"] is None


SH_ERROR = "Please provide excatly one of either SHs or precomputed colors!"
COV_ERROR = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"


def test_exactly_one_of_raises_upstream_s_two_strings():
    t, e = torch.zeros(P, 3), torch.zeros(0)
    with GA.guarded(GA.FILL_A, devices=("cpu",)):
        for shs, colors in ((None, None), (e, None), (None, e), (e, e), (t, t)):
            with pytest.raises(Exception) as err:
                R._exactly_one_of(shs, colors, t, t, None)
            assert str(err.value) == SH_ERROR and type(err.value) is Exception
        for scales, rots, cov in ((None, None, None), (e, e, e), (t, None, None), (None, t, e), (t, t, t), (t, e, t), (None, t, t)):
            with pytest.raises(Exception) as err:
                R._exactly_one_of(t, None, scales, rots, cov)
            assert str(err.value) == COV_ERROR and type(err.value) is Exception
        # what is a render: empty tensors count as absent
        assert R._exactly_one_of(t, e, t, t, e) == (t, None, t, t, None)
        out = R._exactly_one_of(None, t, e, None, t)
        assert out[0] is None and out[1] is t and out[2] is None and out[3] is None and out[4] is t
