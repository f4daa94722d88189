"""The camera-gradient library's two compute entries under guard bands (tests/guarded_alloc.py): no 4096-byte band around a buffer is
touched, every device pointer the library is handed lies inside a guarded body (the fields of ScgModel included), and the results
with both fills and without a guard are equal — which partial sums or outputs assumed clean would break, since every body the
binding allocates (out35, partials) starts poisoned."""
import numpy as np
import pytest
import torch

import geometry_refs as G
import parity_utils as pu
from guarded_alloc import FILL_A, FILL_B, guarded, traced
from scgaussian_amd import _lib_camgrad, camera_grad
from scgaussian_amd import model_path as mp
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = 64, 48
# the device pointers of scg_camgrad_backward (8..10 the camera, 11..17 the inputs, 18 radii, 19 dsplats, 20 partials, 21 out35; 23: the
# stream) and of scg_camgrad_backward_model (7..9 the camera, 10 the model, 11 radii, 12 dsplats, 13 partials, 14 out35; 16: the stream)
TENSOR_POINTERS = {8: "view", 9: "proj", 10: "campos", 11: "means3D", 12: "opacities", 13: "shs", 15: "scales", 16: "rotations", 18: "radii",
                   19: "dsplats", 20: "partials", 21: "out35"}
MODEL_POINTERS = {7: "view", 8: "proj", 9: "campos", 11: "radii", 12: "dsplats", 13: "partials", 14: "out35"}


def _case(name):
    n = 257
    sc = syn.make_scene(n, W, H, seed=15, log_scale_mean=-3.0)
    cam = syn.orbit_camera(W, H, 8.0, -4.0, 7.0)
    model = syn.make_raw_model(sc, ray_fraction=0.6, seed=5) if name == "model" else None
    inputs = G.mode_inputs(sc, cam, 3, 1.0, "sh_sr")
    radii = G.oracle_preprocess({k: v for k, v in inputs.items()}, cam, 3, 1.0)["radii"]
    if name == "everything culled":
        radii = torch.zeros_like(radii)
    return sc, cam, model, radii, G.make_records(n, 50)


def _run(name, fill):
    sc, cam, model, radii, records = _case(name)
    st = pu.hip_settings(cam, 3, (0.0, 0.0, 0.0))
    real, calls = _lib_camgrad.load(), []
    _lib_camgrad._lib = traced(real, calls)
    entry, pointers = ("scg_camgrad_backward_model", MODEL_POINTERS) if model is not None else ("scg_camgrad_backward", TENSOR_POINTERS)

    def go(move):
        st_ = move(st)
        if model is None:
            inputs = move((sc.means3D.to(DEV), sc.opacities.to(DEV), sc.shs.to(DEV), None, sc.scales.to(DEV), sc.rotations.to(DEV), None))
        else:
            inputs = mp._ModelArgs(move(mp.tensors_of(model.to(DEV))))
        out = camera_grad.camera_backward(st_, inputs, move(radii.to(DEV)), move(records.to(DEV)))
        torch.cuda.synchronize()
        return torch.cat([o.reshape(-1) for o in out]), inputs
    try:
        if fill is None:
            return go(lambda x: x)[0].cpu().numpy()
        with guarded(fill) as reg:
            out, inputs = go(reg.rehome)
            touched = reg.check()
            assert touched == [], f"fill {fill}: {len(touched)} band(s) touched: {touched[:8]}"
            mine = [c for c in calls if c.name == entry]
            assert len(mine) == 1
            seen = dict(mine[0].pointers)
            for i, what in pointers.items():
                assert seen.get((i,)) and reg.covers(seen[(i,)]), f"{what} = {seen.get((i,))} lies in no guarded body"
            if model is not None:
                fields = [(path, v) for path, v in mine[0].pointers if path[0] == 10]
                assert len(fields) == 18
                for path, v in fields:
                    unused = (path[1] == "ray" and path[2] == "xyz") or (path[1] == "bg" and path[2] in ("zval", "rayo", "rayd"))
                    assert (not v) if unused else reg.covers(v), (path, v)
            return out.cpu().numpy()
    finally:
        _lib_camgrad._lib = real


@pytest.mark.parametrize("name", ("everything culled", "P = 257", "model"))
def test_no_band_touched_every_pointer_guarded_and_the_fills_agree(name):
    runs = {fill: _run(name, fill) for fill in (FILL_A, FILL_B, None)}
    assert np.isfinite(runs[None]).all()
    for fill in (FILL_A, FILL_B):
        assert np.array_equal(runs[fill], runs[None]), (name, fill, "the result depends on what lay in a buffer before the call")
    assert bool(runs[None].any()) == (name != "everything culled")
