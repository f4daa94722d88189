"""CPU-only checks of scgaussian_amd.optim: the fallback to torch's Adam, what takes it, the host-side watermark policy, and the
C entry points' argument validation (no GPU is touched)."""
import copy
import ctypes as C

import pytest
import torch

import abi_text
from scgaussian_amd import _lib
from scgaussian_amd import optim as O


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(37, 1), (37, 1, 3), (37, 15, 3), (37, 1), (37, 3), (37, 4)]
    return [torch.randn(s, generator=g).requires_grad_() for s in shapes]


def _groups(ps):
    names = ["zval", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3]
    return [{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(ps, lrs, names)]


def _run(opt_cls, ps, steps, seed, **kw):
    opt = opt_cls(_groups(ps), lr=0.0, eps=1e-15, **kw)
    g = torch.Generator().manual_seed(seed)
    for it in range(steps):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ps[0].grad = None if it == 2 else ps[0].grad             # a step without the parameter's gradient
        opt.param_groups[0]["lr"] *= 0.97
        opt.step()
    return opt


def test_fallback_on_cpu_tensors_equals_torch_adam_exactly():
    a, b = _params(), _params()
    oa = _run(O.ArenaAdam, a, 12, seed=5)
    ob = _run(torch.optim.Adam, b, 12, seed=5)
    assert oa.fallback_steps == 12
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
        assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])
        assert float(oa.state[x]["step"]) == float(ob.state[y]["step"])
    # the groups keep their names and the capturable default survives the fallback
    assert [g["name"] for g in oa.param_groups] == ["zval", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert all(g["capturable"] for g in oa.param_groups)


@pytest.mark.parametrize("opts", [dict(amsgrad=True), dict(weight_decay=1e-2), dict(maximize=True)])
def test_each_unsupported_option_takes_the_fallback(opts):
    a, b = _params(1), _params(1)
    oa = _run(O.ArenaAdam, a, 4, seed=2, **opts)
    ob = _run(torch.optim.Adam, b, 4, seed=2, **opts)
    assert oa.fallback_steps == 4
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_unsupported_groups_are_recognised():
    ps = _params()
    opt = O.ArenaAdam(_groups(ps), lr=0.0, eps=1e-15)
    assert all(opt._group_supported(g) for g in opt.param_groups)
    for key, val in (("amsgrad", True), ("weight_decay", 0.1), ("maximize", True), ("differentiable", True),
                     ("lr", torch.tensor(0.1))):
        g = dict(opt.param_groups[0])
        g[key] = val
        assert not opt._group_supported(g), key
    for p in ps:
        p.grad = torch.zeros_like(p)
    assert opt._collect() is None                                # CPU tensors: torch's step


def test_state_dict_round_trip_with_torch_adam():
    a, b = _params(3), _params(3)
    ob = _run(torch.optim.Adam, b, 3, seed=1)
    oa = O.ArenaAdam(_groups(a), lr=0.0, eps=1e-15)
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert all(g["capturable"] for g in oa.param_groups)
    sd = oa.state_dict()
    assert set(sd["state"][2]) == {"step", "exp_avg", "exp_avg_sq"}
    back = torch.optim.Adam(_groups(_params(3)), lr=0.0, eps=1e-15)
    back.load_state_dict(copy.deepcopy(sd))
    assert torch.equal(back.state_dict()["state"][2]["exp_avg"], ob.state_dict()["state"][2]["exp_avg"])
    conv = O.ArenaAdam.from_optimizer(ob)
    assert [g["name"] for g in conv.param_groups] == [g["name"] for g in ob.param_groups]
    assert conv.state[b[2]]["exp_avg"] is ob.state[b[2]]["exp_avg"]          # moved, not copied


def test_install_replaces_both_optimizers():
    class M:
        pass
    m = M()
    ps = _params()
    m.optimizer = torch.optim.Adam(_groups(ps[:3]), lr=0.0, eps=1e-15)
    m.optimizer_bg = torch.optim.Adam(_groups(ps[3:]), lr=0.0, eps=1e-15)
    O.install(m)
    assert isinstance(m.optimizer, O.ArenaAdam) and isinstance(m.optimizer_bg, O.ArenaAdam)
    m2 = M()
    m2.optimizer = torch.optim.Adam(_groups(ps[:2]), lr=0.0)                  # a model without a bg set
    O.install(m2)
    assert isinstance(m2.optimizer, O.ArenaAdam) and not hasattr(m2, "optimizer_bg")


def test_force_full_policy_on_the_host():
    p = torch.zeros(8, 15, 3)
    q = torch.zeros(8, 3)
    st = {"step": torch.zeros(()), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    sq = {"step": torch.zeros(()), "exp_avg": torch.zeros_like(q), "exp_avg_sq": torch.zeros_like(q)}
    assert O._row_len(p) == 45 and O._row_len(q) == 0 and O._row_len(torch.zeros(8, 1, 3)) == 0
    slots = [(q, sq, 0), (p, st, 45)]
    pol = O.SlotPolicy()
    assert pol.force_flags(slots) == [False, True]              # nothing recorded yet: the watermark is unknown
    pol.record(slots)
    assert pol.force_flags(slots) == [False, False]             # the kernel's own writes do not bump _version
    st["exp_avg"].zero_()                                       # edited by torch in place
    assert pol.force_flags(slots) == [False, True]
    pol.record(slots)
    st["exp_avg_sq"] = torch.zeros_like(p)                      # replaced (densification's state surgery)
    assert pol.force_flags(slots) == [False, True]
    pol.record(slots)
    assert pol.force_flags([(p, st, 45), (q, sq, 0)]) == [True, False]      # another parameter in the slot
    p2 = torch.zeros(9, 15, 3)                                  # a new parameter object with new moments (prune / cat)
    st2 = {"step": st["step"], "exp_avg": torch.zeros_like(p2), "exp_avg_sq": torch.zeros_like(p2)}
    assert pol.force_flags([(q, sq, 0), (p2, st2, 45)]) == [False, True]
    pol.invalidate()
    assert pol.force_flags(slots) == [False, True]


def test_new_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("scg_adam_step", "scg_adam_workspace_bytes", "scg_densify_stats"):
        assert abi_text.header_of(name) == "scg_raster.h", name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.scg_struct_bytes(5) == C.sizeof(_lib.ScgAdamSegment) == 88
    assert lib.scg_abi_version() == 10


def test_adam_and_densify_arguments_are_rejected_with_codes():
    lib = _lib.load()
    fake = 0x1000
    ws_bytes = lib.scg_adam_workspace_bytes(6)
    assert ws_bytes >= 4 * 48 and lib.scg_adam_workspace_bytes(0) == 0 and lib.scg_adam_workspace_bytes(17) == 0
    segs = (_lib.ScgAdamSegment * 17)()
    for s in segs:
        s.param = s.grad = s.exp_avg = s.exp_avg_sq = s.step = fake
        s.numel, s.lr, s.beta1, s.beta2, s.eps = 64, 1e-3, 0.9, 0.999, 1e-15
    assert lib.scg_adam_step(None, 1, None, fake, ws_bytes, None) == -1
    assert lib.scg_adam_step(segs, 17, None, fake, ws_bytes, None) == -2 and b"nseg" in lib.scg_last_error()
    assert lib.scg_adam_step(segs, 0, None, fake, ws_bytes, None) == -2
    assert lib.scg_adam_step(segs, 2, None, None, ws_bytes, None) == -1
    assert lib.scg_adam_step(segs, 2, None, fake, 16, None) == -4
    segs[1].numel = -3
    assert lib.scg_adam_step(segs, 2, None, fake, ws_bytes, None) == -2
    segs[1].numel, segs[1].row_len = 64, 45                                 # 64 is not a whole number of rows
    assert lib.scg_adam_step(segs, 2, None, fake, ws_bytes, None) == -2
    segs[1].row_len, segs[1].exp_avg_sq = 0, None
    assert lib.scg_adam_step(segs, 2, None, fake, ws_bytes, None) == -1
    segs[1].exp_avg_sq, segs[1].flags = fake, 8
    assert lib.scg_adam_step(segs, 2, None, fake, ws_bytes, None) == -2
    segs[1].flags, segs[1].step = 0, None
    assert lib.scg_adam_step(segs, 2, None, fake, ws_bytes, None) == -1
    assert lib.scg_densify_stats(-1, fake, fake, 3, fake, fake, fake, None) == -2
    assert lib.scg_densify_stats(10, fake, fake, 1, fake, fake, fake, None) == -2
    assert lib.scg_densify_stats(10, None, fake, 3, fake, fake, fake, None) == -1
    assert lib.scg_densify_stats(0, None, None, 3, None, None, None, None) == 0       # nothing to do


def test_densification_stats_refuses_cpu_tensors():
    P = 5
    with pytest.raises(_lib.ScgError):
        O.densification_stats(torch.zeros(P), torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P, 3),
                              torch.ones(P, dtype=torch.int32))
