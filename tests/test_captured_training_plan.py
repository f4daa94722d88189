"""The growth constant of tests/test_gpu_captured_training.py, held on the CPU: the oracle's binning counts the instances of the
perturbed start model before and after the growth, and the binding's own capacity policy (_counts) and the library's host function
say what a capture makes of them.  No GPU: when the capacity policy changes, this test fails here instead of the planted overflow
silently no longer overflowing there."""
import captured_refs as cr
from scgaussian_amd import _counts, _lib


def test_the_planted_growth_overflows_every_captured_capacity_and_stays_on_the_tile_path():
    _truth, model = cr.start_models()
    n = model.zval.shape[0] + model.bg_xyz.shape[0]
    assert n == cr.P
    before = cr.oracle_counts(model)
    cr.grow(model, cr.GROWTH)
    after = cr.oracle_counts(model)
    print("num_rendered before", before, "after", after, "frozen capacities", [cr.frozen_capacity(n, r) for r in before])
    assert before == cr.ORACLE_BEFORE and after == cr.ORACLE_AFTER           # the numbers the constant was chosen from
    lib = _lib.load()
    for r0, r1 in zip(before, after):
        # the replays before the growth are complete: the count may drift upwards and still fit
        cap = max(cr.frozen_capacity(n, r0), cr.frozen_capacity(n, int(r0 * (1 + cr.DRIFT))))
        assert int(r0 * (1 + cr.DRIFT)) <= cap
        # (1) beyond the head room: the grown count, drifted downwards, exceeds the capacity frozen before the growth — which is
        # at least the 25 % of lookup(capturing=True) and, for a count this small, the first render's generous bound
        assert cap >= _counts._capacity_for(int(r0 * 1.25) + 1)
        assert int(r1 * (1 - cr.DRIFT)) > cap, (r0, r1, cap)
        # (2) within the tile-first binning: the capacity of the recapture (25 % above the grown count, drifted upwards) is one
        # the one-call forward accepts — a capture cannot take the staged path
        recapture = cr.frozen_capacity(n, int(r1 * (1 + cr.DRIFT)))
        assert lib.scg_binning_accepts_bound(recapture, cr.W, cr.H, _lib.BINNING_AUTO) == 1
        assert lib.scg_binning_accepts_bound(_counts._capacity_for(int(r1 * (1 + cr.DRIFT))), cr.W, cr.H, _lib.BINNING_AUTO) == 1
