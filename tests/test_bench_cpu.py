"""bench.py --dump-outputs without a GPU: the files it writes, their size bound and the fixed sample of a larger set."""
import os

import numpy as np
import pytest
import torch

import bench
from scgaussian_amd import synthetic as syn


def _last_step(workload, views, seed=0):
    """Stand-ins of what bench.py's train_step returns, on the CPU, with the shapes of `workload`."""
    w = syn.WORKLOADS[workload]
    P, W, H = w["P"], w["width"], w["height"]
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) for s in ((P, 3), (P, 16, 3), (P, 1), (P, 3), (P, 4))]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    outs = [(torch.rand(3, H, W, generator=g), torch.randint(0, 50, (P,), generator=g, dtype=torch.int32),
             torch.rand(1, H, W, generator=g), torch.rand(1, H, W, generator=g)) for _ in range(views)]
    means2D = torch.zeros((views, P, 3) if views > 1 else (P, 3))
    means2D.grad = torch.randn(means2D.shape, generator=g)
    return (outs, means2D), params


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_a_small_step_is_dumped_whole(tmp_path):
    last, params = _last_step("S1", 1)
    outs, means2D = last
    bench.dump_outputs(str(tmp_path), last, params)
    got = _load(tmp_path)
    assert set(got) == {"color", "depth", "alpha", "radii", "grad_means2D", "grad_means3D", "grad_shs", "grad_opacities",
                        "grad_scales", "grad_rotations"}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["color"], outs[0][0].numpy())
    np.testing.assert_array_equal(got["radii"], outs[0][1].float().numpy())
    np.testing.assert_array_equal(got["grad_means2D"], means2D.grad.numpy())
    np.testing.assert_array_equal(got["grad_shs"], params[1].grad.numpy())


@pytest.mark.parametrize("workload,views", [("S2", 1), ("S3", 1), ("S4", 2)])
def test_a_large_step_keeps_a_fixed_sample_within_the_budget(tmp_path, workload, views):
    last, params = _last_step(workload, views)
    outs, means2D = last
    bench.dump_outputs(str(tmp_path / "a"), last, params)
    assert _size(tmp_path / "a") <= bench.DUMP_BUDGET_BYTES
    got = _load(tmp_path / "a")
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    rows = got["gaussian_index"].astype(np.int64)
    assert len(rows) > 0 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(got["grad_shs"], params[1].grad.numpy()[rows])
    pre = "view1_" if views > 1 else ""
    np.testing.assert_array_equal(got[pre + "radii"], outs[-1][1].float().numpy()[rows])
    color = outs[-1][0].numpy()
    if "pixel_index" in got:                               # images too large for half the budget: pixels sampled as well
        px = got["pixel_index"].astype(np.int64)
        np.testing.assert_array_equal(got[pre + "color"], color.reshape(3, -1)[:, px])
    else:
        np.testing.assert_array_equal(got[pre + "color"], color)
    # the same workload samples the same rows and pixels, whatever the values
    last2, params2 = _last_step(workload, views, seed=1)
    bench.dump_outputs(str(tmp_path / "b"), last2, params2)
    again = _load(tmp_path / "b")
    for name in ("gaussian_index", "pixel_index"):
        assert (name in got) == (name in again)
        if name in got:
            np.testing.assert_array_equal(got[name], again[name])
