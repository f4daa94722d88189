"""What the camera gradients cost (no gate: a measurement).

    python tools/camgrad_timing.py [--out profiles/r27_camgrad_timing.json] [--calls 25] [--workloads S1 S2]

One process, warm, every figure the MEDIAN of `--calls` calls; host-clock figures are synchronised on both sides, kernel figures lie
between two events on the stream.  Per workload (synthetic.WORKLOADS: the benchmark's Gaussian counts and image sizes, SH degree 3):
  backward_ms           loss.backward() of one training view, camera tensors NOT requiring grad: the baseline, the parent's backward
  backward_camera_ms    the same with viewmatrix / projmatrix / campos requiring grad (the sibling node + two launches)
  geometry_backward_ms  scg_geometry_backward alone between events (the staged path's own stage): what the pass follows
  camera_pass_ms        the two launches alone between events, at degree 0 and 3, with and without SCG_CAMGRAD_NO_CAMPOS
  pose_algebra_ms       CameraPose's three matrices from delta and their backward, alone (torch; host-bound)
  pose_step_ms          render + backward to CameraPose.delta through the rasterizer
  torch_projection_ms   the baseline for the pose step — the parent offers no route to a camera gradient at all — : autograd through a
                        plain-torch projection of the same Gaussians (view transform, clip transform, pixel position, depth)
The hypothesis on record: the camera pass costs less than the geometry backward it follows.  `hypothesis_holds` states the outcome
per workload.  One process of one visit: no run-to-run spread is known."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scgaussian_amd import camera_grad, pose, rasterizer as R, synthetic as syn  # noqa: E402

DEV = "cuda"


def median_host_ms(fn, calls, before=None):
    out = []
    for i in range(calls + 2):
        arg = before() if before else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg) if before else fn()
        torch.cuda.synchronize()
        if i >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def median_event_ms(fn, calls):
    out = []
    for i in range(calls + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


class StageEvents:
    """A `timer` for rasterizer.backward_stages: events around the stage called `name`."""

    def __init__(self, name):
        self.name, self.ms = name, []

    @contextlib.contextmanager
    def __call__(self, stage):
        if stage != self.name:
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.pending = (a, b)

    def collect(self):
        torch.cuda.synchronize()
        self.ms.append(self.pending[0].elapsed_time(self.pending[1]))


def settings(cam, deg, leaves=False):
    import math
    camd = cam.to(DEV)
    t = [camd.world_view_transform.contiguous(), camd.full_proj_transform.contiguous(), camd.camera_center.contiguous()]
    if leaves:
        t = [x.clone().requires_grad_(True) for x in t]
    return R.GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                                           torch.zeros(3, device=DEV), 1.0, t[0], t[1], deg, t[2], False, False)


def measure(name, calls):
    w = syn.WORKLOADS[name]
    P, W, H = w["P"], w["width"], w["height"]
    sc = syn.make_scene(P, W, H, seed=0).to(DEV)
    cam = syn.orbit_camera(W, H, 10.0, -5.0, 7.0)
    up = [t.to(DEV) for t in syn.make_upstream_grads(W, H)]
    params = {n: getattr(sc, n).clone().requires_grad_(True) for n in ("means3D", "opacities", "shs", "scales", "rotations")}
    res = {"P": P, "width": W, "height": H}

    def forward(st):
        c, r, d, a = R.GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), **params)
        return (c * up[0]).sum() + (d * up[1]).sum() + (a * up[2]).sum()
    for key, leaves in (("backward_ms", False), ("backward_camera_ms", True), ("backward_ms_again", False)):
        st = settings(cam, 3, leaves)
        res[key] = median_host_ms(lambda loss: loss.backward(), calls, before=lambda: forward(st))

    # the geometry backward alone (the staged path's stage) and the records a camera pass reads
    st = settings(cam, 3)
    seven = (sc.means3D, sc.opacities, sc.shs, None, sc.scales, sc.rotations, None)
    ev = StageEvents("geometry_backward")
    records = radii = None
    for _ in range(calls + 2):
        fs = R.forward_stages(st, sc.means3D, sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations, prepare_backward=True)
        g = R.backward_stages(st, fs["inputs"], fs, up[0], up[1], up[2], want_dsplats=True, timer=ev)
        ev.collect()
        records, radii = g["dsplats"], fs["radii"]
    res["geometry_backward_ms"] = statistics.median(ev.ms[2:])
    res["visible"] = int((radii > 0).sum())
    out, partials = torch.empty(35, device=DEV), torch.empty((P + 255) // 256 * 27, device=DEV)
    res["camera_pass_ms"] = {}
    for deg in (0, 3):
        st_d = settings(cam, deg)
        for want in (True, False):
            res["camera_pass_ms"][f"degree {deg}, {'with' if want else 'NO_'}campos"] = median_event_ms(
                lambda: camera_grad.camera_backward(st_d, seven, radii, records, want, out=out, partials=partials), calls)
    full = res["camera_pass_ms"]["degree 3, withcampos"]
    res["hypothesis_holds"] = bool(full < res["geometry_backward_ms"])

    # the pose step
    pc = pose.CameraPose(cam.to(DEV))

    def algebra():
        (pc.world_view_transform.sum() + pc.full_proj_transform.sum() + pc.camera_center.sum()).backward()
    res["pose_algebra_ms"] = median_host_ms(algebra, calls)

    def pose_step():
        forward(settings_of(pc)).backward()

    def settings_of(c):
        import math
        return R.GaussianRasterizationSettings(c.image_height, c.image_width, math.tan(c.FoVx / 2), math.tan(c.FoVy / 2),
                                               torch.zeros(3, device=DEV), 1.0, c.world_view_transform, c.full_proj_transform, 3,
                                               c.camera_center, False, False)
    res["pose_step_ms"] = median_host_ms(pose_step, calls)
    wts = torch.randn(P, 3, device=DEV)

    def torch_projection():
        V, PM = pc.world_view_transform, pc.full_proj_transform
        pos = torch.cat([sc.means3D, torch.ones(P, 1, device=DEV)], 1)
        t, h = pos @ V, pos @ PM
        m_w = 1.0 / (h[:, 3] + 1e-7)
        px, py = ((h[:, 0] * m_w + 1.0) * W - 1.0) * 0.5, ((h[:, 1] * m_w + 1.0) * H - 1.0) * 0.5
        (px * wts[:, 0] + py * wts[:, 1] + t[:, 2] * wts[:, 2]).sum().backward()
    res["torch_projection_ms"] = median_host_ms(torch_projection, calls)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r27_camgrad_timing.json")
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--workloads", nargs="+", default=["S1", "S2"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camgrad_timing.py measures on the GPU: no device found (there is no CPU figure to report)")
    result = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "caveat": "one process of one visit",
              "workloads": {n: measure(n, a.calls) for n in a.workloads}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))
