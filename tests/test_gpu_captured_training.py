"""Every replay of a captured training run held to the eager step — the composition over time that examples/fit_captured.py runs
and no other module checks: one graph_step.CapturedStep per training view over the SAME parameters, each owning the `.grad`
tensors of its own capture; the optimizer stepping in place between (mode `outside`: torch.optim.Adam, eagerly) or inside
(mode `arena`: optim.ArenaAdam + optim.densification_stats in the graph) the replays; eager renders of the same cameras in
between; an overflow recovered one replay late while the two other steps replay.

A 150-step trajectory cannot carry a tight bar (Adam with eps = 1e-15 turns a one-ulp gradient difference into a sign flip of the
update), so the run has a LOCKSTEP TWIN: a second model, optimizer and set of statistics tensors that is never captured and is put
back on the captured run's state — every parameter, exp_avg, exp_avg_sq and step, max_radii2D, xyz_gradient_accum and denom, in
place, bit for bit — before every iteration.  Each replay is compared with ONE eager step from bit-identical parameters; nothing
accumulates.  The run is fit's at P = 1 500, 120 x 72 (a partial tile on both axes), SH degree 3, 12 iterations over three views.

What each replay is held to (the number is the `check` column of the printed table):
  1  render, radii and loss equal the twin's eager step bit for bit (the forward is deterministic, the loss kernels reduce in the
     fixed order of reduce.h);
  2  every parameter gradient and viewspace_points.grad within the float atomics' noise of the twin's: 4 x the twin's own
     eager-versus-eager spread, floor 2e-5 of the tensor's largest magnitude (captured_refs.grad_noise_bar, the bar of
     tests/test_gpu_graph_step.py);
  3  whose gradient it is: after steps[v].replay() `p.grad is steps[v].grads[i]`, the three steps' gradients live in pairwise
     distinct storages, and the gradients of the two steps that did not replay are unchanged bit for bit;
  4  the optimizer used THIS replay's gradients, once: the twin's optimizer, stepped eagerly from the pre-replay snapshot on a copy
     of the gradients as they read after the replay, gives the captured run's parameters, moments and step bit for bit, and step
     equals the number of replays so far (a recapture applies no extra step).  Mode `outside` holds the same for torch's Adam
     stepping on `p.grad` after the replay;
  5  (arena) an eager optim.densification_stats on the snapshot, fed this replay's viewspace_points.grad and radii, gives the
     captured run's three statistics tensors bit for bit.

Events planted in the run:
  after iteration 3   the PSNR probe of fit (a no_grad render of the three cameras) and one eager forward + backward of camera 0
                      on the captured run's model — the same frames, hint buffers and gradient-arena pool — its gradients
                      parked away from `p.grad`;
  after iteration 5   the scene grows: log(GROWTH) = log(10) onto the raw log-scales of both sets.  The constant was chosen on
                      the CPU from the oracle's num_rendered of the start model, per camera 2 643 / 2 513 / 2 562 before and
                      17 129 / 17 033 / 16 983 after, against the 12 288 instances a capture freezes for such a count
                      (captured_refs.frozen_capacity; tests/test_captured_training_plan.py holds both conditions without a GPU).
                      From here a replay is COMPLETE iff its image equals the twin's (the eager path reads the host and retries:
                      always complete) and CLIPPED iff its count word exceeds its capacity; the two must agree on every replay, the
                      count word equals the twin's eager num_rendered, a clipped replay still has the twin's radii, is exempt from
                      1 (image, loss) and 2, and meets 3-5 all the same (its gradients were applied: the documented semantics).
                      At the end every step has overflows == clipped replays == 1 == recaptures, and its replay after the clipped
                      one is complete;
  after iteration 8   every learning rate halves (param_groups[k]["lr"] and sync_hyperparameters() on both runs: the reference's
                      update_learning_rate); check 4 goes on holding bit for bit.  The three replays that follow recapture (the
                      overflow), so the rates halve once more after iteration 11: the last replay is of a graph captured before
                      the change and reads the new rates from the device table.

Out of scope, known: CapturedStep.check() re-arms a count word from the host without knowing whether a later replay has already
written it.  This module synchronises after every replay, so it neither provokes nor settles that race; closing it needs a
device-side protocol.  Nor is anything pinned that a graph freezes by construction (camera, SH degree, background colour, P).
"""
import pytest
import torch

import captured_refs as cr
from scgaussian_amd import _cameras, _counts, losses, optim
from scgaussian_amd.graph_step import CapturedStep
from scgaussian_amd.render import PipelineParams, render

pytestmark = pytest.mark.gpu
DEV = "cuda"
PIPE = PipelineParams()
NAMES = ("zval", "features_dc", "features_rest", "opacity", "scaling", "rotation",
         "bg_xyz", "bg_features_dc", "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation")
STATS = ("max_radii2D", "xyz_gradient_accum", "denom")


class _Run:
    """One model, optimizer and set of statistics tensors with fit's step closures over them: the captured run and its twin."""

    def __init__(self, mode, start, cams, targets, bg):
        self.mode, self.cams, self.targets, self.bg = mode, cams, targets, bg
        self.model = cr.copy_model(start, DEV).requires_grad_()
        self.model.active_sh_degree = cr.SH_DEGREE
        self.params = self.model.parameters()
        assert len(self.params) == len(NAMES)
        groups = cr.param_groups(self.model)
        if mode == "arena":
            self.opt = optim.ArenaAdam(groups, eps=1e-15)
        else:
            try:
                self.opt = torch.optim.Adam(groups, eps=1e-15, fused=True)
            except (RuntimeError, TypeError):
                self.opt = torch.optim.Adam(groups, eps=1e-15)
        n = self.model.zval.shape[0] + self.model.bg_xyz.shape[0]
        self.stats = [torch.zeros(n, device=DEV), torch.zeros(n, 1, device=DEV), torch.zeros(n, 1, device=DEV)]
        # the optimizer's state exists before anything is captured or copied: one step on zero gradients creates it without moving a
        # parameter (0 / (0 + eps) = 0), then the step counters go back to zero — fit's own preparation
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.opt.step()
        for st in self.opt.state.values():
            st["step"].zero_()
        self.clear_grads()
        if mode == "arena":
            self.opt.sync_hyperparameters()

    def clear_grads(self):
        for p in self.params:
            p.grad = None

    def forward_backward(self, v):
        pkg = render(self.cams[v], self.model, PIPE, self.bg)
        loss = losses.image_loss(pkg["render"], self.targets[v], 0.2)
        loss.backward()
        return loss, pkg

    def step_fn(self, v, with_optimizer):
        def fn():
            loss, pkg = self.forward_backward(v)
            if self.mode == "arena":
                optim.densification_stats(*self.stats, pkg["viewspace_points"].grad, pkg["radii"])
                if with_optimizer:
                    self.opt.step()
            return loss, pkg["render"], pkg["radii"], pkg["viewspace_points"]
        return fn

    def state(self):
        """[(name, tensor)] of everything an iteration carries to the next: the tensors themselves."""
        out = []
        for name, p in zip(NAMES, self.params):
            st = self.opt.state[p]
            out += [(name, p), (name + ".exp_avg", st["exp_avg"]), (name + ".exp_avg_sq", st["exp_avg_sq"]), (name + ".step", st["step"])]
        return out + list(zip(STATS, self.stats))

    def halve_learning_rates(self):
        for g in self.opt.param_groups:
            g["lr"] = g["lr"] * 0.5
        if self.mode == "arena":
            self.opt.sync_hyperparameters()


def _eager(run, v):
    """One eager step of the twin from the state it holds (which it leaves as it is: no statistics, no optimizer)."""
    run.clear_grads()
    loss, pkg = run.forward_backward(v)
    torch.cuda.synchronize()
    key = (cr.W, cr.H, _cameras._camera_key(run.cams[v].world_view_transform))
    count = _counts._SPEC_STATE[torch.cuda.current_device()].cam_hint[key][1]   # the num_rendered this forward read from the host
    return dict(loss=loss.detach().clone(), render=pkg["render"].detach().clone(), radii=pkg["radii"].clone(),
                vs=pkg["viewspace_points"].grad.clone(), grads=[p.grad.clone() for p in run.params], count=int(count))


def _storages(tensors):
    return {t.untyped_storage().data_ptr() for t in tensors}


def _psnr(a, b):
    return float(-10.0 * torch.log10(((a - b) ** 2).mean()))


def _captured_run_against_its_twin(mode):
    tab = cr.Table(mode)
    truth, start = cr.start_models()
    cams = [c.to(DEV) for c in cr.cameras()]
    bg = torch.zeros(3, device=DEV)
    # the run starts where a fresh process starts: what an earlier test (the other mode of this one) learnt about these cameras'
    # capacities is dropped, so that the captures freeze the capacity of the small scene
    spec = _counts._SPEC_STATE.get(torch.cuda.current_device())
    if spec is not None:
        for c in cams:
            _counts.forget(spec, cr.P, cr.W, cr.H, _cameras._camera_key(c.world_view_transform))
    truth = truth.to(DEV)
    with torch.no_grad():
        targets = [render(c, truth, PIPE, bg)["render"].clone() for c in cams]
    run, twin = _Run(mode, start, cams, targets, bg), _Run(mode, start, cams, targets, bg)
    n_views = len(cams)
    if mode == "arena":
        for v in range(n_views):                                         # the warm-up WITHOUT the optimizer, as fit arranges it
            fn = run.step_fn(v, False)
            for _ in range(3):
                run.clear_grads()
                fn()
        steps = [CapturedStep(run.step_fn(v, True), params=run.params, warmup=0) for v in range(n_views)]
    else:
        steps = [CapturedStep(run.step_fn(v, False), params=run.params) for v in range(n_views)]
    history = [[] for _ in steps]                                        # per step: (clipped, complete) of each of its replays
    parked = None
    try:
        for it in range(cr.ITERS):
            v = it % n_views
            torch.cuda.synchronize()
            # ---- the twin goes back on the captured run's state, in place; the snapshot is what the replay started from -------
            snapshot = [(name, t.detach().clone()) for name, t in run.state()]
            with torch.no_grad():
                for (_n, dst), (_m, src) in zip(twin.state(), snapshot):
                    dst.copy_(src)
            others = {u: [g.clone() for g in steps[u].grads] for u in range(n_views) if u != v}
            want, noise = _eager(twin, v), _eager(twin, v)
            # ---- the replay -----------------------------------------------------------------------------------------------
            loss, image, radii, points = steps[v].replay()
            torch.cuda.synchronize()
            count, capacity = steps[v].words[0].value(), steps[v].capacities[0]
            clipped, complete = count > capacity, torch.equal(image, want["render"])
            history[v].append((clipped, complete))
            tab.at(it + 1, v, "clipped" if clipped else "complete")
            tab.note(f"count word {count}  capacity {capacity}  eager num_rendered {want['count']}  "
                     f"overflows {steps[v].overflows}  recaptures {steps[v].recaptures}")
            tab.true("-", "one count word", len(steps[v].words) == 1)
            tab.true("-", "count == eager count", count == want["count"], f"{count} vs {want['count']}")
            tab.true("-", "clipped iff incomplete", clipped == (not complete), f"clipped {clipped} complete {complete}")
            tab.bits(1, "radii", radii, want["radii"])
            if not clipped:
                tab.bits(1, "render", image, want["render"])
                tab.bits(1, "loss", loss.detach(), want["loss"])
                for name, p, w, n in zip(NAMES, run.params, want["grads"], noise["grads"]):
                    tab.noise(2, "d " + name, p.grad, w, n)
                tab.noise(2, "d viewspace_points", points.grad, want["vs"], noise["vs"])
            # ---- whose gradient it is --------------------------------------------------------------------------------------
            tab.true(3, "p.grad is this step's", all(p.grad is g for p, g in zip(run.params, steps[v].grads)))
            owned = [_storages(s.grads) for s in steps]
            tab.true(3, "storages distinct", all(owned[a].isdisjoint(owned[b]) for a in range(n_views) for b in range(a)))
            if parked is not None:
                tab.true(3, "parked eager grads apart", all(_storages(parked).isdisjoint(o) for o in owned))
            for u, before in others.items():
                same = all(torch.equal(g, b) for g, b in zip(steps[u].grads, before))
                tab.true(3, f"step {u}'s grads unchanged", same)
            # ---- the optimizer used this replay's gradients, once ------------------------------------------------------------
            grads = [g.clone() for g in steps[v].grads]
            if mode == "outside":
                run.opt.step()                                           # eagerly, on p.grad as the replay left it
            for p, g in zip(twin.params, grads):                         # (the twin still holds the snapshot)
                p.grad = g
            twin.opt.step()
            if mode == "arena":
                optim.densification_stats(*twin.stats, points.grad.clone(), radii.clone())
            torch.cuda.synchronize()
            for (name, got), (_n, exp) in zip(run.state(), twin.state()):
                if name in STATS and mode != "arena":
                    continue
                tab.bits(5 if name in STATS else 4, name, got.detach(), exp.detach().to(got.device))
            counters = [float(run.opt.state[p]["step"]) for p in run.params]
            tab.true(4, "step == replays so far", all(s == it + 1 for s in counters), f"{min(counters):g}..{max(counters):g} vs {it + 1}")
            # ---- the planted events --------------------------------------------------------------------------------------------
            if it + 1 == 3:
                with torch.no_grad():
                    probe = sum(_psnr(render(c, run.model, PIPE, bg)["render"], t) for c, t in zip(cams, targets)) / n_views
                kept = [p.grad for p in run.params]
                run.clear_grads()
                eager_loss, _pkg = run.forward_backward(0)
                torch.cuda.synchronize()
                parked = [p.grad for p in run.params]                    # kept to the end: their arena stays out of the pool
                for p, g in zip(run.params, kept):
                    p.grad = g
                tab.note(f"event: PSNR probe {probe:.2f} dB, eager forward + backward of view 0 (loss {float(eager_loss.detach()):.6f})")
            if it + 1 == 5:
                cr.grow(run.model, cr.GROWTH)
                tab.note(f"event: the scene grows, log-scales += log({cr.GROWTH:g})")
            if it + 1 in (8, 11):
                # (8: the three recaptures that follow are captured at the new rates; 11: the last replay is of a graph captured
                # BEFORE the change, which reads the rates from the device table)
                run.halve_learning_rates()
                twin.halve_learning_rates()
                tab.note("event: every learning rate halves")
        # ---- the overflow's accounting, per step -----------------------------------------------------------------------------
        for v, (s, h) in enumerate(zip(steps, history)):
            tab.at(cr.ITERS, v, "final")
            n_clipped = sum(c for c, _ in h)
            tab.note(f"replays {''.join('C' if c else '.' for c, _ in h)}  overflows {s.overflows}  recaptures {s.recaptures}")
            tab.true("-", "overflows == clipped == 1", s.overflows == n_clipped == 1, f"{s.overflows} / {n_clipped}")
            tab.true("-", "recaptures == overflows", s.recaptures == s.overflows, f"{s.recaptures} / {s.overflows}")
            tab.true("-", "complete after clipped", all(not h[k + 1][0] and h[k + 1][1] for k in range(len(h) - 1) if h[k][0])
                     and not h[-1][0])
            tab.true("-", "clipped image differed", all(not ok for c, ok in h if c))
    finally:
        run.clear_grads()
        twin.clear_grads()
        for s in steps:
            s.close()
    tab.assert_clean()


@pytest.mark.parametrize("mode", ["outside", "arena"])
def test_every_replay_of_a_captured_training_run_is_the_eager_step(mode):
    with torch.autograd.set_multithreading_enabled(False):               # fit's single_gpu_host_setup(), for this test only
        _captured_run_against_its_twin(mode)
