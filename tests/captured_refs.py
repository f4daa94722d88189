"""What tests/test_gpu_captured_training.py and tests/test_captured_training_plan.py share: the run of examples/fit_captured.py at
a small size (scene, cameras, targets, perturbed start, optimizer groups), the growth constant of the planted overflow with the
capacity a capture freezes, and the two kinds of comparison (bit for bit / within the float
atomics' noise) with the table they print.

Nothing here touches the GPU at import time: the plan test runs the oracle on the CPU only."""
import math

import torch

from scgaussian_amd import _counts, synthetic as syn

P, W, H, SEED = 1_500, 120, 72, 0            # 8 x 5 tiles: a partial tile on both axes
ITERS = 12                                   # four passes over the three views
SH_DEGREE = 3

# The planted overflow: after iteration 5 the raw log-scales of both sets (ray-bound and background) grow by log(GROWTH).
# Chosen from the ORACLE's num_rendered of the perturbed start model, per camera (oracle/torch_rasterizer.py on the CPU):
#     before  ORACLE_BEFORE        a capture of such a count freezes frozen_capacity(P, R) = 12 288 instances
#     after   ORACLE_AFTER         every camera beyond that capacity by more than DRIFT
# (tests/test_captured_training_plan.py recomputes both rows and holds the two conditions on them.)
GROWTH = 10.0
ORACLE_BEFORE = (2_643, 2_513, 2_562)
ORACLE_AFTER = (17_129, 17_033, 16_983)
# The counts of the run itself are not the oracle's: five Adam steps lie between the perturbed start and the growth.  A step moves
# a parameter by at most its learning rate: log-scales by 5 x 5e-3 (2.5 % of a radius), depths by 5 x 2e-3 of 2 .. 12 — a few
# per cent of a count that is proportional to the footprints' area.  Both conditions are held with 10 % to spare.
DRIFT = 0.10


def cameras():
    return [syn.default_camera(W, H), syn.orbit_camera(W, H, 8.0, 0.0, 7.0), syn.orbit_camera(W, H, -8.0, 3.0, 7.0)]


def start_models():
    """(truth, start): the raw model of the scene and the perturbed copy examples/fit_captured.py:fit starts from, on the CPU
    (the perturbation is fit's: the same generator, the same draws in the same order, one fp32 operation each)."""
    gt = syn.make_scene(P, W, H, seed=SEED, log_scale_mean=-3.3)
    truth = syn.make_raw_model(gt)
    g = torch.Generator().manual_seed(SEED + 1)
    model = syn.make_raw_model(gt)
    with torch.no_grad():
        model.zval.mul_(1.0 + 0.03 * torch.randn(model.zval.shape, generator=g))
        model.bg_xyz.add_(0.03 * torch.randn(model.bg_xyz.shape, generator=g))
        model.features_dc.add_(0.3 * torch.randn(model.features_dc.shape, generator=g))
        model.opacity.add_(0.5 * torch.randn(model.opacity.shape, generator=g))
    return truth, model


def copy_model(model, dev):
    """A model of its own tensors on `dev` (RayBoundModel.to may hand back the same tensors on the same device)."""
    from scgaussian_amd.ply_io import RayBoundModel
    return RayBoundModel(**{k: (v.detach().clone().to(dev) if isinstance(v, torch.Tensor) else v) for k, v in model.__dict__.items()})


def grow(model, factor):
    """The scene grows: log(factor) onto the raw log-scales of both sets, in place."""
    with torch.no_grad():
        model.scaling.add_(math.log(factor))
        model.bg_scaling.add_(math.log(factor))


def activated_scene(model):
    """The model as the tensors the oracle takes (the reference's getters)."""
    with torch.no_grad():
        return syn.Scene(model.get_xyz.contiguous(), model.get_scaling.contiguous(), model.get_rotation.contiguous(),
                         model.get_opacity.contiguous(), model.get_features.contiguous())


def oracle_counts(model):
    """num_rendered of every camera by the oracle's binning (CPU)."""
    import parity_utils as pu
    sc = activated_scene(model)
    return tuple(int(pu.run_oracle(sc, cam, SH_DEGREE, (0.0, 0.0, 0.0))["aux"]["binning"]["num_rendered"]) for cam in cameras())


def frozen_capacity(n_gaussians, count):
    """The capacity a capture freezes for a camera whose renders so far counted `count` instances, by the binding's own policy
    (_counts): the model path's first render starts from first_sight_capacity, every render commits _next_capacity of the
    capacity in use, and lookup(capturing=True) takes the larger of that and the bound of 25 % more instances."""
    cap = _counts._next_capacity(_counts.first_sight_capacity(n_gaussians), count)
    return max(cap, _counts._capacity_for(int(count * 1.25) + 1))


def param_groups(model):
    """fit's learning rates, by tensor rank / role."""
    groups = []
    for p in model.parameters():
        if p.dim() == 3:
            groups.append({"params": [p], "lr": 1e-2 if p.shape[1] == 1 else 5e-4})
        elif p.shape[1] == 1:
            groups.append({"params": [p], "lr": 3e-2 if p is not model.zval else 2e-3})
        elif p.shape[1] == 4:
            groups.append({"params": [p], "lr": 1e-3})
        else:
            groups.append({"params": [p], "lr": 2e-3 if p is model.bg_xyz else 5e-3})
    return groups


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def grad_noise_bar(want, noise):
    """The bar of a gradient against an eager one: 4 x the eager step's own run-to-run spread (the blend backward's float
    atomics), with a floor of 2e-5 of the tensor's largest magnitude."""
    scale = float(want.abs().max()) + 1e-30
    return max(4.0 * float((noise - want).abs().max()), 2e-5 * scale), scale


def grad_noise_ok(got, want, noise):
    for g, w, n in zip(got, want, noise):
        tol, scale = grad_noise_bar(w, n)
        assert float((g - w).abs().max()) <= tol, (float((g - w).abs().max()), tol, scale)


class Table:
    """One line per comparison: the measured deviation beside its bar.  Failures are collected, so that a run prints the whole
    table before `assert_clean` fails it."""

    def __init__(self, mode):
        self.mode, self.failures, self.where = mode, [], ""

    def at(self, it, view, kind):
        self.where = f"{self.mode:7s} it {it:2d} view {view} {kind:8s}"

    def note(self, text):
        print(f"{self.where} | {text}")

    def _row(self, check, name, measured, bar, ok):
        print(f"{self.where} | check {check} {name:22s} {measured:>24s}   bar {bar:<12s} {'ok' if ok else 'FAILED'}")
        if not ok:
            self.failures.append(f"{self.where.strip()}: check {check} {name}: {measured.strip()} (bar {bar})")

    def bits(self, check, name, got, want):
        """got == want bit for bit (differing elements: bar 0)."""
        if got.shape != want.shape or got.dtype != want.dtype:
            self._row(check, name, f"{tuple(got.shape)} {got.dtype}", f"{tuple(want.shape)}", False)
            return False
        bad = 0 if torch.equal(got, want) else int((got != want).sum())
        self._row(check, name, f"{bad} of {got.numel()} differ", "0", bad == 0)
        return bad == 0

    def noise(self, check, name, got, want, noise):
        tol, _scale = grad_noise_bar(want, noise)
        dev = float((got - want).abs().max())
        self._row(check, name, f"{dev:.3e}", f"{tol:.3e}", dev <= tol)

    def true(self, check, name, ok, measured=""):
        self._row(check, name, measured or str(bool(ok)), "holds", bool(ok))

    def assert_clean(self):
        assert not self.failures, "\n" + "\n".join(self.failures)
