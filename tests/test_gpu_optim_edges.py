"""scg_adam_step alone, at its watermark and launch edges, held to the BITS of the fp32 restatement of csrc/adam_math.h
(tests/optim_refs.py: one rounding per operation, torch's order; anchored on the CPU by tests/test_optim_refs_cpu.py, which also
shows that each frame used here tells the restatement from a subtly wrong kernel).

Every comparison is np.array_equal on the uint32 view of p, m, v and the step counter after K successive restatement steps (a NaN
is compared as a NaN: IEEE 754 leaves its sign and payload open, and host and device differ there).  The kernel is called directly
through the C entry point on tensors carved out of sentinel-filled buffers, with a workspace of the test's own, except in the last
group, which goes through ArenaAdam.

  (a) plain segments: sizes around the float4 group and the 4096-element workgroup, every 4-byte alignment, back-to-back launches
  (b) arithmetic: zero, signed zero, denormal, underflowing, overflowing and non-finite gradients and moments, two eps, late steps
  (c) row segments at every watermark, against the restatement AND against a twin in which every launch is forced
  (d) gradients that move the watermark, or must not
  (e) sixteen segments in one launch, empty ones among them; the all-empty launch
  (f) the device table of learning rates
  (g) ArenaAdam's twelve groups, and a row segment that changes its slot"""
import numpy as np
import pytest
import torch

import optim_refs as OR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _held(got, want, prev, segs, k, what, lrs=None):
    """Bits of every segment's p, m, v and counter.  Where p alone differs, the message says which neighbouring fp32 coefficient
    pairs (if any) would explain the whole segment."""
    try:
        OR.assert_state_bits(got, want, what)
    except AssertionError as e:
        notes = []
        for i, (a, b) in enumerate(zip(got, want)):
            if OR.same_bits(a.m, b.m) and OR.same_bits(a.v, b.v) and not OR.same_bits(a.p, b.p):
                lr = segs[i].lr if lrs is None else lrs[i]
                notes.append((i, OR.coefficient_pairs_explaining(prev[i], segs[i], segs[i].g[k], lr, a.p)))
        raise AssertionError(f"{e}; p alone differs in segments (index, coefficient moves that explain it): {notes}") from None


def _initial(segs):
    return [OR.State(s.p, s.m, s.v, np.float32(s.step)) for s in segs]


def _run(segs, launches, forces, read_each=False, lr_table=None, use_table=False, what=""):
    """The launches on a fresh Runner: [(states, workspace)] after each launch (read_each) or after the last alone, in which case
    nothing synchronises between the launches."""
    r = OR.Runner(segs, DEV, lr_table=lr_table)
    out = []
    for k in range(launches):
        r.launch(k, force=forces[k], use_table=use_table)
        if read_each:
            out.append(r.read())
    if not read_each:
        out.append(r.read())
    assert r.sentinels_intact(), what
    return r, out


# ---------------------------------------------------------------------------------------------------------------- (a)

@pytest.mark.parametrize("off", OR.PLAIN_OFFSETS, ids=lambda o: "off" + "_".join(map(str, o)))
def test_plain_sizes_and_alignment(off):
    """numel 1 .. 8193 at one carve offset; three launches with no synchronisation between them (the ticket's reset)."""
    aligned = OR.plain_frames()
    for seg, twin in zip(OR.plain_frames(off), aligned):
        want = OR.ref_launches([seg], 3)
        r, out = _run([seg], 3, [False] * 3, what=seg.name)
        assert r.vec(0) == (tuple(off) == (0, 0, 0, 0)), seg.name          # one misaligned tensor: the scalar path
        got, ws = out[-1]
        _held(got, want[-1], want[-2], [seg], 2, seg.name)
        assert got[0].step == 3.0
        OR.assert_workspace(ws, {}, seg.name)                              # ticket back at zero, no word touched
        t = OR.ref_launches([twin], 3)[-1][0]                              # the same bits at every alignment
        assert OR.same_bits(got[0].p, t.p) and OR.same_bits(got[0].m, t.m) and OR.same_bits(got[0].v, t.v)


# ---------------------------------------------------------------------------------------------------------------- (b)

@pytest.mark.parametrize("seg", OR.arith_frames(), ids=lambda s: s.name.replace(" ", "_"))
def test_arithmetic_edges(seg):
    """4096 + 5 elements holding every combination of optim_refs.G_VALUES x M_VALUES x V_VALUES, p with +0 and -0; two launches,
    the second on the first's results (Inf and NaN moments, saturated v)."""
    want = OR.ref_launches([seg], 2)
    _r, out = _run([seg], 2, [False] * 2, read_each=True, what=seg.name)
    prev = _initial([seg])
    for k in range(2):
        _held(out[k][0], want[k], prev, [seg], k, f"{seg.name} launch {k}")
        OR.assert_workspace(out[k][1], {}, seg.name)
        prev = want[k]


# ---------------------------------------------------------------------------------------------------------------- (c)

def _watermark_case(seg):
    """One forced launch, then three without the flag (the last two feed the last live column and let it decay again): the
    restatement's bits and watermark after each; a twin with every launch forced gives the same bits (the skip is an exact
    no-op)."""
    want = OR.ref_launches([seg], 4)
    _r, out = _run([seg], 4, [True, False, False, False], read_each=True, what=seg.name)
    _t, twin = _run([seg], 4, [True] * 4, read_each=True, what=seg.name + " twin")
    prev = _initial([seg])
    for k in range(4):
        what = f"{seg.name} launch {k}"
        _held(out[k][0], want[k], prev, [seg], k, what)
        _held(twin[k][0], out[k][0], prev, [seg], k, what + " forced twin")
        for ws in (out[k][1], twin[k][1]):
            OR.assert_workspace(ws, {0: want[k][0].live}, what)
        prev = want[k]
    assert want[0][0].live == seg.w, seg.name


@pytest.mark.parametrize("rows", OR.ROW_COUNTS)
def test_row_watermarks(rows):
    """row_len 45 at w = 0 .. 45; 1 row, 91 rows (one workgroup, a tail of 3), 92 (a row across two workgroups), 273 (three)."""
    for seg in OR.row_frames(rows):
        _watermark_case(seg)


def test_row_watermarks_unaligned():
    """All four tensors 4 bytes past a 16-byte boundary: the scalar row path."""
    for seg in OR.row_frames(92, off=(4, 4, 4, 4)):
        _watermark_case(seg)


def test_row_lengths_other_than_45():
    """Rows shorter than a float4 group (1, 3), multiples of it (4, 48) and longer than a workgroup's chunk (4097)."""
    for seg in OR.other_row_frames():
        _watermark_case(seg)


# ---------------------------------------------------------------------------------------------------------------- (d)

@pytest.mark.parametrize("name", list(OR.moving_frames()))
def test_watermark_moves(name):
    """From the w = 9 state of 92 rows: a gradient at exactly column `live` of a row in the second workgroup, one in the last
    column of the last row, NaN and -Inf beyond the watermark (all processed, all raise it), -0.0 beyond it (an exact no-op)."""
    seg, moved = OR.moving_frames()[name]
    want = OR.ref_launches([seg], 3)
    assert [x[0].live for x in want[:2]] == [OR.MOVE_W, moved]
    _r, out = _run([seg], 3, [True, False, False], read_each=True, what=seg.name)
    prev = _initial([seg])
    for k in range(3):
        _held(out[k][0], want[k], prev, [seg], k, f"{seg.name} launch {k}")
        OR.assert_workspace(out[k][1], {0: want[k][0].live}, f"{seg.name} launch {k}")
        prev = want[k]


def test_forced_launch_rederives_the_watermark():
    """Moments replaced behind the kernel's back, as densification and load_state_dict do: a forced launch on zero moments and zero
    gradients lowers the watermark to 0; one on moments with a non-zero tail (a checkpoint from a higher SH degree) sets it to the
    true value, and the unforced launch after it reads that tail."""
    L, n = 45, OR.MOVE_ROWS * 45
    seg = OR.row_seg(OR.MOVE_ROWS, L, OR.MOVE_W, seed=77, launches=4)
    col = np.arange(n) % L
    seg.g[1][:] = 0
    r = OR.Runner([seg], DEV)
    step = lambda st, k: OR.State(*OR.adam_step_ref(st.p, st.m, st.v, seg.g[k], st.step, seg.lr, seg.b1, seg.b2, seg.eps),   # noqa: E731
                                  st.step + np.float32(1))
    want = step(_initial([seg])[0], 0)
    r.launch(0, force=True)
    got, ws = r.read()
    _held(got, [want], _initial([seg]), [seg], 0, "establish")
    OR.assert_workspace(ws, {0: OR.MOVE_W}, "establish")
    # zero moments, zero gradients, forced
    zeros = np.zeros(n, np.float32)
    r.write(0, "m", zeros), r.write(0, "v", zeros)
    prev = OR.State(want.p, zeros, zeros, want.step)
    want = step(prev, 1)
    r.launch(1, force=True)
    got, ws = r.read()
    _held(got, [want], [prev], [seg], 1, "zeroed")
    assert OR.same_bits(want.p, prev.p) and not want.m.any() and not want.v.any()
    OR.assert_workspace(ws, {0: 0}, "zeroed")
    # a tail up to column 30 that the gradients (columns < 9) do not feed
    rng = np.random.default_rng(5)
    m = np.where(col < 31, rng.standard_normal(n) * 1e-3, 0).astype(np.float32)
    v = np.where(col < 31, 1e-6 + 1e-6 * rng.random(n), 0).astype(np.float32)
    r.write(0, "m", m), r.write(0, "v", v)
    prev = OR.State(want.p, m, v, want.step)
    want = step(prev, 2)
    r.launch(2, force=True)
    got, ws = r.read()
    _held(got, [want], [prev], [seg], 2, "tail, forced")
    assert OR.live_after(want.m, want.v, L) == 31
    OR.assert_workspace(ws, {0: 31}, "tail, forced")
    prev, want = want, step(want, 3)
    r.launch(3, force=False)
    got, ws = r.read()
    _held(got, [want], [prev], [seg], 3, "tail, unforced")
    assert not OR.same_bits(want.m[col == 30], prev.m[col == 30])          # the tail decays: it was read
    OR.assert_workspace(ws, {0: 31}, "tail, unforced")
    assert r.sentinels_intact()


# ---------------------------------------------------------------------------------------------------------------- (e), (f)

def _row_slots(segs):
    return [i for i, s in enumerate(segs) if s.row_len]


def test_sixteen_segments_and_the_all_empty_launch():
    """One launch of 16 segments (optim_refs.sixteen_frame): every counter, the empty segments' included, advances by exactly 1 per
    launch; each row segment's watermark lands in its own slot and no other word is written."""
    segs = OR.sixteen_frame()
    slots = _row_slots(segs)
    assert slots == [2, 6] and [segs[i].numel for i in (0, 4, 10, 15)] == [0] * 4
    want = OR.ref_launches(segs, 3)
    forces = [[True] * 16, [False] * 16, [False] * 16]
    r, out = _run(segs, 3, forces, read_each=True, what="sixteen")
    assert [r.vec(i) for i in (1, 3, 11)] == [True, False, False]
    prev = _initial(segs)
    for k in range(3):
        _held(out[k][0], want[k], prev, segs, k, f"sixteen launch {k}")
        assert [float(s.step) for s in out[k][0]] == [float(np.float32(s.step)) + k + 1 for s in segs]
        OR.assert_workspace(out[k][1], {i: want[k][i].live for i in slots}, f"sixteen launch {k}")
        prev = want[k]
    assert [want[0][i].live for i in slots] == [9, 5]
    # the all-empty launch: its one workgroup only advances the counters
    empties = [OR.empty_seg(step=s, launches=2) for s in (0, 9, OR.STEP_LATE)]
    _r, out = _run(empties, 2, [False, True], what="all empty")
    got, ws = out[-1]
    assert [float(s.step) for s in got] == [2.0, 11.0, OR.STEP_LATE + 2.0]
    OR.assert_workspace(ws, {}, "all empty")


def test_lr_table():
    """lr_table = NULL and a device table holding the same doubles: the same bits.  A table that differs from seg.lr: the table's
    values are the ones used."""
    segs = OR.sixteen_frame()
    slots = _row_slots(segs)
    forces = [[True] * 16, [False] * 16]
    own = [s.lr for s in segs]
    _r, plain = _run(segs, 2, forces, what="no table")
    _r, same = _run(segs, 2, forces, lr_table=own, use_table=True, what="same table")
    OR.assert_state_bits(same[-1][0], plain[-1][0], "table of the segments' own lr")
    other = own[3:] + own[:3]
    assert all(a != b for a, b in zip(own, other)) and all(lr in OR.LRS for lr in other)
    want = OR.ref_launches(segs, 2, lrs=other)
    _r, out = _run(segs, 2, forces, lr_table=other, use_table=True, what="other table")
    _held(out[-1][0], want[-1], want[-2], segs, 1, "table that differs from seg.lr", lrs=other)
    OR.assert_workspace(out[-1][1], {i: want[-1][i].live for i in slots}, "other table")
    assert any(not OR.same_bits(a.p, b.p) for a, b in zip(out[-1][0], plain[-1][0]) if a.p.size)


# ---------------------------------------------------------------------------------------------------------------- (g)

TORCH_VS_KERNEL = {}               # name -> differing elements of (m, v, p) against torch.optim.Adam on the device: a record


def test_arena_adam_twelve_groups_and_the_slot_shift():
    """The twelve groups of tests/test_gpu_optim.py with 93 ray-bound Gaussians (features_rest crosses a workgroup boundary), six
    steps with the position-lr schedule, then a step in which zval has no gradient (features_rest moves from slot 2 to slot 1) and
    the step after it (back to slot 2): the restatement's bits, the right watermark, no step through torch.

    torch.optim.Adam runs beside it on the device; how many elements differ from the kernel in bits after six steps is printed
    and kept in profiles/README.md (a record: torch's bits are not the contract)."""
    import test_gpu_optim as TG
    from scgaussian_amd import optim as O
    base = TG._tensors(P=155)
    assert base["features_rest"].shape[0] == 92 + 1
    a, b = TG.Model(base, O.ArenaAdam), TG.Model(base, torch.optim.Adam)
    ref = {k: OR.State(v.cpu().numpy().ravel(), np.zeros(v.numel(), np.float32), np.zeros(v.numel(), np.float32), np.float32(0))
           for k, v in base.items()}
    gen = torch.Generator(device=DEV).manual_seed(21)
    names = {n: attr for attr, n, _ in TG.RAY + TG.BG}

    def one_step(it, drop=()):
        g = TG._grads(base, gen, rest_cols=9, drop=drop)
        for m in (a, b) if not drop else (a,):
            m.set_grads(g)
            m.step(it)
        torch.cuda.synchronize()
        for o in a.opts():
            for grp in o.param_groups:
                attr = names[grp["name"]]
                if g[attr] is None:
                    continue
                assert grp["lr"] in OR.LRS and grp["betas"] == OR.BETAS[0]
                st = ref[attr]
                p, m_, v = OR.adam_step_ref(st.p, st.m, st.v, g[attr].cpu().numpy().ravel(), st.step, grp["lr"], *grp["betas"],
                                            grp["eps"])
                ref[attr] = OR.State(p, m_, v, st.step + np.float32(1))

    def held(what):
        for o in a.opts():
            for grp in o.param_groups:
                attr, p = names[grp["name"]], grp["params"][0]
                st = o.state[p]
                got = OR.State(p.detach().cpu().numpy().ravel(), st["exp_avg"].cpu().numpy().ravel(),
                               st["exp_avg_sq"].cpu().numpy().ravel(), np.float32(float(st["step"])))
                OR.assert_state_bits([got], [ref[attr]], f"{what} {attr}")
        for o, k in ((a.optimizer, "features_rest"), (a.optimizer_bg, "bg_features_rest")):
            assert o.live_columns()[a.t[k]] == OR.live_after(ref[k].m, ref[k].v, 45) == 9, (what, k)
            assert o.fallback_steps == 0

    for it in range(1, 7):
        one_step(it)
    held("six steps")
    for ob in b.opts():
        for grp in ob.param_groups:
            attr, p = names[grp["name"]], grp["params"][0]
            st = ob.state[p]
            TORCH_VS_KERNEL[attr] = (p.numel(), OR.differing(st["exp_avg"].cpu().numpy(), ref[attr].m),
                                     OR.differing(st["exp_avg_sq"].cpu().numpy(), ref[attr].v),
                                     OR.differing(p.detach().cpu().numpy(), ref[attr].p))
    tot = np.array(list(TORCH_VS_KERNEL.values())).sum(axis=0)
    print("TORCH-VS-KERNEL bits after 6 steps (elements, m, v, p differing):", TORCH_VS_KERNEL)
    print("TORCH-VS-KERNEL total: %d elements, m %d, v %d, p %d" % tuple(tot))
    one_step(7, drop=("zval",))
    assert [rl for (_p, _st, rl) in a.optimizer._dev[0].last_slots].index(45) == 1
    held("zval without a gradient")
    one_step(8)
    assert [rl for (_p, _st, rl) in a.optimizer._dev[0].last_slots].index(45) == 2
    held("the step after")
    assert float(a.optimizer.state[a.t["zval"]]["step"]) == 7 and float(a.optimizer.state[a.t["features_rest"]]["step"]) == 8
