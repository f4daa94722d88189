"""The binning stage ALONE (csrc/binning_tiles.hip, csrc/binning.hip, csrc/tile_sort.h) against the exact numpy reference of
tests/binning_refs.py, on frames planted at its edges: every list length at which a sort path changes (in sparse and in dense
frames, with spread, tied, bucket-limit and outlier keys), ids at the id-width steps, Gaussian counts at the slice steps,
rectangles and grids at the walk, band and tile-count steps, bounds in place of num_rendered, and launch-order hints of any
content.  Part 1 calls scg_binning directly, with SCG_BINNING_AUTO and with SCG_BINNING_GLOBAL_SORT; part 2 drives the same list
lengths through scg_forward, whose forward blend has a sort of its own and whose option bits reroute the long lists — the
reference is then built from the rects and depth keys read back from the workspace, so it does not rest on the geometry's
arithmetic.  The output is integers: everything is equality, no tile and no list entry is left out (binning_refs.compare; its
teeth are shown on the CPU by tests/test_binning_refs_cpu.py).  Which internal path a tied list takes depends on the scatter's
arrival order and cannot be observed: results are asserted, not paths."""
import numpy as np
import pytest

import binning_refs as BR
import guarded_alloc as G

pytestmark = pytest.mark.gpu

ALGOS = {"auto": BR.AUTO, "global": BR.GLOBAL_SORT}
DIRECT = [(n, a) for n in BR.LENGTH_FRAMES + BR.MEAN_FRAMES + BR.IDWIDTH_FRAMES + BR.SLICE_FRAMES + BR.GRID_FRAMES for a in ALGOS]


@pytest.mark.parametrize("name, algo", DIRECT, ids=[f"{n}-{a}" for n, a in DIRECT])
def test_scg_binning_equals_the_stable_sort_reference(name, algo):
    fr, ref = BR.frame(name), BR.reference(name)
    out = BR.run_binning(fr, ALGOS[algo])
    # the tile-first path takes grids up to 38 400 tiles; beyond, SCG_BINNING_AUTO silently takes the global sort
    assert out["accepts"] == (1 if (algo == "auto" and fr.T <= BR.TILE_PATH_MAX_TILES) else 0)
    BR.compare_run(ref, out)


@pytest.mark.parametrize("algo", ALGOS)
def test_an_empty_frame_has_empty_ranges_identity_tables_and_a_count_of_zero(algo):
    W, H, P = 75, 40, 300                                    # 5 x 3 tiles: 15 tiles on 16 slots
    T = 15
    words, nr = BR.run_empty(W, H, P, ALGOS[algo])
    nw = BR.ranges_words(T)
    assert not words[:2 * T].any() and (words[nw:] == BR.PATTERN).all()
    BR.check_order_bands(words[:nw], T)
    assert nr[0] == 0 and (nr[1:] == BR.PATTERN).all()


@pytest.mark.parametrize("which", ("R+1", "R", "R-1", "4R", "1", "tile_start", "mid_long"))
def test_a_bound_in_place_of_num_rendered_clips_and_writes_nothing_behind_it(which):
    exact = BR.reference("bounds")
    bound = BR.bounds_of(exact)[which]
    ref = BR.reference("bounds", bound)
    out = BR.run_binning(ref["frame"], BR.AUTO)
    assert out["accepts"] == 1
    BR.compare_run(ref, out)
    if bound > exact["R"]:                                   # the slots behind the counted total hold no entry: left alone
        assert (out["point_list"][exact["R"]:] == BR.PATTERN).all()
        assert (out["keys_sorted"][exact["R"]:] == np.uint64(BR.PATTERN64)).all()


_UNHINTED = {}


def _unhinted(name):
    if name not in _UNHINTED:
        _UNHINTED[name] = BR.run_binning(BR.frame(name), BR.AUTO)
        BR.compare_run(BR.reference(name), _UNHINTED[name])
    return _UNHINTED[name]


@pytest.mark.parametrize("fill", BR.HINT_FILLS)
@pytest.mark.parametrize("name", BR.HINT_FRAMES)
def test_launch_order_hints_of_any_content_change_no_result(name, fill):
    fr, ref = BR.frame(name), BR.reference(name)
    base = _unhinted(name)
    cost = BR.hint_fill(fill, fr.T, BR.TILE_COST_EDGES, seed=1)
    bcost = BR.hint_fill(fill, 4 * fr.T, BR.BWD_COST_EDGES, seed=2)
    for kw in (dict(tile_cost_in=cost), dict(bwd_cost_in=bcost), dict(tile_cost_in=cost, bwd_cost_in=bcost)):
        out = BR.run_binning(fr, BR.AUTO, **kw)
        BR.compare_run(ref, out)                             # (both order tables: permutations, every entry in its band)
        assert np.array_equal(out["point_list"], base["point_list"])
        assert np.array_equal(out["words"][:2 * fr.T], base["words"][:2 * fr.T])
        assert np.array_equal(out["keys_sorted"], base["keys_sorted"])
        if "tile_cost_in" in kw:
            BR.check_cost_order(out["words"], fr.T, cost, ref["lens"])


@pytest.mark.parametrize("name", ("lengths:equal/sparse", "lengths:bucket_ties/dense", "grid:129x128"))
def test_two_runs_of_a_frame_give_the_same_bits(name):
    fr = BR.frame(name)
    a, b = BR.run_binning(fr, BR.AUTO), BR.run_binning(fr, BR.AUTO)
    assert np.array_equal(a["point_list"], b["point_list"]) and np.array_equal(a["words"][:2 * fr.T], b["words"][:2 * fr.T])
    assert np.array_equal(a["keys_sorted"], b["keys_sorted"])


# one frame per internal path of scg_binning — every lengths frame holds lists of each sort size, work lists and global scratch
# included: equal keys (the radix / bitonic fallbacks), the dense 8-wave sort with the bucket limit reached, a large grid (bands,
# padded order slots), spread keys (the bucket sorts) — and the global 64-bit key sort
START_FRAMES = (("lengths:equal/sparse", "auto"), ("lengths:bucket_ties/dense", "auto"), ("grid:129x128", "auto"),
                ("lengths:spread/sparse", "auto"), ("lengths:equal/sparse", "global"))


@pytest.mark.parametrize("name, algo", START_FRAMES, ids=[f"{n}-{a}" for n, a in START_FRAMES])
def test_what_the_scratch_held_before_the_call_changes_no_bit(name, algo):
    """The runner's scratch starts as one fixed byte, 0x5A; the binding's comes from torch.empty.  A word of it that a kernel reads,
    or adds to, before anybody wrote it — class_counts, len_hist, a row of the slice table, the sort's counters — gives another
    list, another range or a broken order table when the scratch starts from other bytes: here from the two fills of
    tests/guarded_alloc.py (0xFF and 0x3C in every byte: guarded_alloc.fill_byte).  Every output is compared bit for bit, guards included; of the two order
    tables only what compare_run holds (permutations, every entry in its band, longer classes first): the order inside a length
    class is whatever the LDS atomics give, from run to run."""
    fr, ref = BR.frame(name), BR.reference(name)
    a, b = (BR.run_binning(fr, ALGOS[algo], scratch_byte=G.fill_byte(fill)) for fill in (G.FILL_A, G.FILL_B))
    assert a.keys() == b.keys()
    nw = BR.ranges_words(fr.T)
    for out in (a, b):
        BR.compare_run(ref, out)
        out["ranges"], out["behind_the_words"] = out["words"][:2 * fr.T], out["words"][nw:]
        del out["words"]
    for k in a:
        assert G.same_bits(a[k], b[k]), (name, algo, k)


@pytest.mark.parametrize("options", (0, BR.SKIP_RARE_SORT, BR.RARE_8WAVE | BR.SPLIT_LONG_LISTS, BR.DEBUG_SEPARATE_SORT | BR.DEBUG_SEPARATE_HIST),
                         ids=("fused", "skip_rare", "split", "separate"))
def test_what_the_workspace_held_before_scg_forward_changes_no_bit(options):
    """The same for the one-call path's workspace (every plane of the frame and the binning scratch in one allocation), on the
    scene of tied depths, sparse and dense capacity: the images, radii, rectangles, keys, the lists up to the counted total, the
    ranges and order words, the long-list counts and num_rendered."""
    sc = BR.forward_scene("ties")
    for capacity in (sc.P, sc.T * BR.DENSE_MEAN):
        a, b = (BR.run_forward(sc, capacity, options, ws_byte=G.fill_byte(fill)) for fill in (G.FILL_A, G.FILL_B))
        nw, R = BR.ranges_words(sc.T), a["num_rendered_out"]
        assert R == b["num_rendered_out"] == sc.P <= capacity
        for out in (a, b):                                       # (behind the counted total and behind the words: nobody's; the
            BR.check_order_bands(out["words"][:nw], sc.T)        #  order inside a length class: the LDS atomics')
            out["point_list"], out["words"] = out["point_list"][:R], out["words"][:2 * sc.T]
        for k in a:
            assert G.same_bits(a[k], b[k]), (options, capacity, k)


# ------------------------------------------------------------------------------------------- the same edges through scg_forward

def _recorded_forward(sc, capacity, options):
    """BR.run_forward with the entry point wrapped: the option word scg_forward actually received."""
    from scgaussian_amd import _lib
    lib = _lib.load()
    real, seen = lib.scg_forward, []

    def recording(*a):
        seen.append(int(a[18]))
        return real(*a)

    lib.scg_forward = recording
    try:
        out = BR.run_forward(sc, capacity, options)
    finally:
        lib.scg_forward = real
    assert seen == [options], (seen, options)
    return out


def _reference_from_workspace(sc, out, capacity):
    """The reference built from the rects and depth keys the geometry stage left in the workspace; they are the planted ones."""
    fr = BR.Frame(sc.name, BR.FWD_W, BR.FWD_H, out["rects"], out["depth_keys"])
    ref = BR.reference_of(fr, capacity)
    assert np.array_equal(ref["lens"], sc.lens) and np.array_equal(out["depth_keys"], sc.key)      # lengths and tie groups as planted
    x, y, w, h = fr.unpacked()
    assert (w == 1).all() and (h == 1).all() and np.array_equal(y * fr.gx + x, sc.tile)
    return ref


def _check_long_counts(ref, out, capacity):
    if out["sorts_in_blend"]:                                # (the separate sort kernel's launch records nothing)
        limit = 3584 if capacity // ref["frame"].T >= BR.DENSE_MEAN else 1536
        n = ref["hi"] - ref["lo"]
        assert out["long_lists"].tolist() == [int((n > limit).sum()), int((n > 16384).sum())]


@pytest.mark.parametrize("dense", (False, True), ids=("sparse", "dense"))
@pytest.mark.parametrize("kind", BR.FWD_PATTERNS)
def test_scg_forward_sorts_the_same_lists_whatever_the_options(kind, dense):
    sc = BR.forward_scene(kind)
    capacity = sc.T * BR.DENSE_MEAN if dense else sc.P       # the capacity decides which kernels run
    assert (capacity // sc.T >= BR.DENSE_MEAN) == dense and capacity >= sc.P
    ref = None
    for options in BR.FWD_OPTIONS:
        out = _recorded_forward(sc, capacity, options)
        assert out["sorts_in_blend"] == (0 if options & BR.DEBUG_SEPARATE_SORT else 1)
        if ref is None:
            ref = _reference_from_workspace(sc, out, capacity)
        else:
            assert np.array_equal(out["rects"], ref["frame"].rects) and np.array_equal(out["depth_keys"], ref["frame"].keys)
        BR.compare_forward(ref, out)
        _check_long_counts(ref, out, capacity)


def test_scg_forward_with_the_split_route_and_a_capacity_that_cuts_a_long_list():
    sc = BR.forward_scene("spread")
    exact = BR.reference_of(BR.Frame(sc.name, BR.FWD_W, BR.FWD_H, np.stack([(sc.tile % sc.gx) | ((sc.tile // sc.gx) << 16),
                                                                          np.full(sc.P, 1 | (1 << 16))], 1), sc.key))
    t = int(np.nonzero(exact["lens"] == 8193)[0][0])
    capacity = int(exact["start"][t]) + 5001                 # inside a list longer than 4 096 (and no multiple of 64: padding follows)
    assert capacity % 64 and exact["start"][t] + 4096 < capacity < exact["end"][t]
    options = BR.RARE_8WAVE | BR.SPLIT_LONG_LISTS
    out = _recorded_forward(sc, capacity, options)
    ref = _reference_from_workspace(sc, out, capacity)
    assert ref["R"] == exact["R"] > capacity
    BR.compare_forward(ref, out)
    _check_long_counts(ref, out, capacity)
