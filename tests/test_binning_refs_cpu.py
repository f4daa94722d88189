"""tests/binning_refs.py without a GPU: the numpy reference against the oracle's bin_and_sort and against a brute-force sort of
tuples; every planted frame really has the property it is named for (list lengths, tie groups, live ids, grids, R // tiles —
computed from the frame); the comparator rejects every subtle corruption of a correct output, so the GPU tests would fail on a
subtly wrong kernel; and the oracle's preprocess confirms that every Gaussian planted for the one-call frames touches exactly the
tile it was planted on."""
import numpy as np
import pytest

import binning_refs as BR


def _random_frame(seed, gx, gy, P, culled=0.3, few_keys=False):
    rng = np.random.default_rng(seed)
    w, h = rng.integers(1, gx + 1, P), rng.integers(1, gy + 1, P)
    x, y = rng.integers(0, gx - w + 1), rng.integers(0, gy - h + 1)
    keys = rng.choice(BR.spread(5, 1.0, 9.0), P) if few_keys else rng.integers(BR.KEY_LO, BR.KEY_HI + 1, P)
    dead = rng.random(P) < culled
    dead[0] = False
    rects = np.stack([x | (y << 16), w | (h << 16)], 1)
    rects[dead] = 0
    keys = np.where(dead, BR.CULLED, keys)
    return BR.Frame(f"random-{seed}", 16 * gx - 3, 16 * gy - 7, rects, keys)


@pytest.mark.parametrize("seed, gx, gy, P, few", [(1, 5, 4, 300, False), (2, 9, 7, 1000, True), (3, 1, 1, 50, True), (4, 17, 3, 700, False)])
def test_reference_agrees_with_the_oracles_bin_and_sort(seed, gx, gy, P, few):
    import torch
    from oracle import torch_rasterizer as orc
    fr = _random_frame(seed, gx, gy, P, few_keys=few)
    ref = BR.reference_of(fr)
    x, y, w, h = fr.unpacked()
    pre = dict(grid=(fr.gx, fr.gy), tiles_touched=torch.from_numpy(w * h),
               rect=torch.from_numpy(np.stack([x, y, x + w, y + h], 1).astype(np.int32)),
               depth=torch.from_numpy(fr.keys.view(np.float32).copy()))
    assert np.array_equal(pre["depth"].numpy().view(np.uint32), fr.keys)       # (culled keys are NaN bit patterns: kept as bits)
    o = orc.bin_and_sort(pre, fr.W, fr.H)
    assert o["num_rendered"] == ref["R"]
    assert np.array_equal(o["point_list"], ref["ids"])
    assert np.array_equal(o["ranges"], ref["ranges"])
    assert np.array_equal(o["keys_sorted"], ref["keys_sorted"])


@pytest.mark.parametrize("seed", range(4))
def test_reference_agrees_with_a_brute_force_sort_of_tuples(seed):
    fr = _random_frame(10 + seed, 4, 3, 60, few_keys=seed % 2 == 0)
    x, y, w, h = (a.tolist() for a in fr.unpacked())
    inst = sorted((ty * fr.gx + tx, int(fr.keys[i]), i) for i in range(fr.P) for ty in range(y[i], y[i] + h[i])
                  for tx in range(x[i], x[i] + w[i]))
    R = len(inst)
    for bound in (None, R + 3, R, R - 1, R // 2, 1):
        ref = BR.reference_of(fr, bound)
        assert ref["R"] == R and [int(i) for i in ref["ids"]] == [i for _, _, i in inst]
        assert [int(k) for k in ref["keys_sorted"]] == [(t << 32) | k for t, k, _ in inst]
        cap = R if bound is None else bound
        for t in range(fr.T):
            pos = [p for p, (tt, _, _) in enumerate(inst) if tt == t]
            s, e = (pos[0], pos[-1] + 1) if pos else (0, 0)
            lo, hi = min(s, cap), min(e, cap)
            assert tuple(ref["ranges"][t]) == ((lo, hi) if hi > lo else (0, 0))


# ------------------------------------------------------------------------------------------------ the planted properties

@pytest.mark.parametrize("name", BR.LENGTH_FRAMES)
def test_length_frames_hold_every_length_and_their_key_pattern(name):
    fr = BR.frame(name)
    tile, key, _ = BR.expand(fr)
    lens = np.bincount(tile, minlength=fr.T)
    planted = fr.tags["planted"]
    assert sorted(planted.values()) == sorted(BR.LENGTHS) and len(planted) == len(BR.LENGTHS)
    assert all(lens[t] == n for t, n in planted.items()) and lens.sum() == sum(BR.LENGTHS)
    mean = int(lens.sum()) // fr.T
    assert (mean >= BR.DENSE_MEAN) if fr.tags["dense"] else (mean < BR.DENSE_MEAN)
    kind = fr.tags["kind"]
    for t, n in planted.items():
        g = BR.tie_groups(key[tile == t]) if n else np.zeros(1, int)
        if kind == "spread" or n < 3:
            assert kind in ("equal", "few") or g[0] <= 1
        if kind == "equal" and n:
            assert g[0] == n
        if kind == "few" and n > 200:
            assert 20 <= len(g) <= 37
        if kind in ("bucket_ties", "long_ties") and n >= 100 and not (kind == "long_ties" and n > 8192):
            assert list(g[:3]) == [BR.BUCKET_MAX + 1, BR.BUCKET_MAX, 1]
        if kind == "long_ties" and n > 8192:
            assert list(g[:3]) == [BR.LONG_BUCKET_MAX + 1, BR.LONG_BUCKET_MAX, 1]
            k = np.sort(key[tile == t])
            for size in (BR.LONG_BUCKET_MAX, BR.LONG_BUCKET_MAX + 1):            # in sorted order the group straddles a multiple of 1 024
                v = [u for u, c in zip(*np.unique(k, return_counts=True)) if c == size][0]
                first = int(np.searchsorted(k, v))
                assert first // 1024 != (first + size - 1) // 1024 and first % 1024 != 0
        if kind == "outliers" and n >= 3:
            k = np.sort(key[tile == t])
            assert k[0] == BR.KEY_LO and k[-1] == BR.KEY_HI and (n < 4 or int(k[-2]) - int(k[1]) == 3 * (n - 3))


def test_mean_edge_frames_sit_either_side_of_the_dense_mean():
    for name, mean in zip(BR.MEAN_FRAMES, (BR.DENSE_MEAN - 1, BR.DENSE_MEAN)):
        fr = BR.frame(name)
        lens = np.bincount(BR.expand(fr)[0], minlength=fr.T)
        assert fr.T == 64 and int(lens.sum()) // fr.T == mean
        assert all(lens[t] == n for t, n in fr.tags["planted"].items())
        assert {2048, 2049, 4096, 4097, 8192, 8193} <= set(lens.tolist())


@pytest.mark.parametrize("name", BR.IDWIDTH_FRAMES)
def test_id_width_frames_tie_the_ids_at_the_byte_steps(name):
    fr = BR.frame(name)
    P = int(name.split(":")[1])
    assert fr.P == P
    tile, key, gid = BR.expand(fr)
    live = np.unique(gid)
    assert len(live) < 60                                                     # almost everything is culled
    t = fr.tags["tied_tile"]
    k = key[tile == t]
    v, c = np.unique(k, return_counts=True)
    tied = set(gid[(tile == t) & (key == v[c.argmax()])].tolist())
    assert len(tied) > BR.BUCKET_MAX and tied == set(fr.tags["tied"])
    assert P - 1 in tied and all(i in tied for i in (255, 256, 65535, 65536) if i < P)
    id_bits = 8
    while (1 << id_bits) < P:
        id_bits += 8
    assert id_bits == {256: 8, 257: 16, 65536: 16, 65537: 24}[P] and max(tied) >> (id_bits - 8) > 0


@pytest.mark.parametrize("name", BR.SLICE_FRAMES)
def test_slice_frames_leave_whole_slices_empty(name):
    fr = BR.frame(name)
    tile, _, gid = BR.expand(fr)
    R, live = len(tile), np.unique(gid)
    n = BR.slice_count(fr.P, R)
    if name.startswith("large"):
        want = int(name.split(":")[1])
        assert R == want and fr.P == 300 and n == (256 if want >= BR.LARGE_FRAME else 128)
        return
    P = int(name.split(":")[1])
    assert fr.P == P and live[0] == 0 and live[-1] == P - 1 and list(live) == fr.tags["live_ids"]
    assert n == (256 if P >= BR.LARGE_SCENE else 128)
    slot = live * (16 * n) // P                                                # the wave slice of tile_walk.h that owns an id
    assert len(np.unique(slot // 16)) <= min(n, len(live)) and (P < 2047 or len(np.unique(slot // 16)) < n // 8)
    if P > 16:
        assert np.diff(live).max() > P // 4                                   # a long culled run


@pytest.mark.parametrize("name", BR.GRID_FRAMES)
def test_grid_frames_hold_the_rectangles_that_fit(name):
    fr = BR.frame(name)
    arg = name.split(":")[1]
    gx, gy = (BR.BIG_GRIDS[arg][:2] if arg in BR.BIG_GRIDS else map(int, arg.split("x")))
    assert (fr.gx, fr.gy) == (gx, gy) and fr.W % 16 and fr.H % 16
    shapes = set(fr.tags["shapes"])
    sizes = {(w, h) for _, _, w, h in shapes}
    for c in ((0, 0, 1, 1), (gx - 1, 0, 1, 1), (0, gy - 1, 1, 1), (gx - 1, gy - 1, 1, 1), (0, 0, gx, gy)):
        assert c in shapes
    for (w, h) in ((6, 8), (48, 1), (7, 7), (49, 1), (3, BR.COOP // 3 + 1), (7, BR.COOP // 7 + 1), (240, 1)):
        assert ((w, h) in sizes) == (w <= gx and h <= gy), (w, h)
    rows = sorted(set(gy * b // 8 for b in range(1, 8)) - {0})
    for r in rows:                                                             # a rectangle across every band boundary
        assert any(y < r < y + h for _, y, _, h in shapes), r
    lens = np.bincount(BR.expand(fr)[0], minlength=fr.T)
    assert (lens >= 2).all()                                                  # the two full-image rectangles
    for t in fr.tags["long_tiles"]:
        assert lens[t] >= 102
    if arg in BR.BIG_GRIDS:
        per_band = (gy // 8) * gx
        within = {t % per_band for t in fr.tags["long_tiles"]}
        assert {255, 256} <= within or arg.startswith("24")
        if arg == "128x128":
            assert per_band == 2048 and 2047 in within
        if arg == "129x128":
            assert per_band == 2064 and any(w >= 2048 for w in within)
        if arg == "240x160":
            assert fr.T == BR.TILE_PATH_MAX_TILES
        if arg == "241x160":
            assert fr.T > BR.TILE_PATH_MAX_TILES


def test_grid_frames_cover_the_tile_counts_and_band_shapes():
    grids = [tuple(map(int, n.split(":")[1].split("x"))) for n in BR.GRID_FRAMES if n.split(":")[1] not in BR.BIG_GRIDS]
    assert {1, 7, 8, 9, 63, 64, 65} <= {gx * gy for gx, gy in grids}
    assert {1, 2, 7} <= {gy for _, gy in grids} and 1 in {gx for gx, _ in grids}


def test_bound_frame_has_long_lists_and_its_bounds_fall_where_they_should():
    fr = BR.frame("bounds")
    ref = BR.reference("bounds")
    assert all(ref["lens"][t] == n for t, n in fr.tags["planted"].items()) and ref["R"] == sum(fr.tags["planted"].values())
    b = BR.bounds_of(ref)
    R = ref["R"]
    assert (b["R+1"], b["R"], b["R-1"], b["4R"], b["1"]) == (R + 1, R, R - 1, 4 * R, 1)
    assert b["tile_start"] in ref["start"][ref["lens"] > 0].tolist()
    cut = np.nonzero((ref["start"] < b["mid_long"]) & (ref["end"] > b["mid_long"]))[0]
    assert len(cut) == 1 and ref["lens"][cut[0]] > 8192
    assert R // fr.T < BR.DENSE_MEAN <= 4 * R // fr.T                          # the bound 4 R makes the frame a dense one


# ------------------------------------------------------------------------------------------------- the comparator's teeth

def _corruptions(ref):
    """name -> buffers that differ from a correct output in one subtle way."""
    R, T, cap = ref["R"], ref["frame"].T, ref["cap"]
    out = {}

    def new():
        return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in BR.perfect_output(ref).items()}

    n = min(R, cap)
    whole = np.repeat(ref["end"] <= cap, ref["lens"])[:n]
    pair = whole[:-1] & whole[1:] & (ref["tile"][1:n] == ref["tile"][:n - 1])    # neighbours in one list below the bound
    same_key = ref["key"][1:n] == ref["key"][:n - 1]
    tied, neigh = np.nonzero(pair & same_key)[0], np.nonzero(pair & ~same_key)[0]
    o = new()
    i = int(tied[len(tied) // 2])
    o["point_list"][[i, i + 1]] = o["point_list"][[i + 1, i]]
    out["two tied ids swapped"] = o
    o = new()
    i = int(neigh[len(neigh) // 2])
    o["point_list"][[i, i + 1]] = o["point_list"][[i + 1, i]]
    if cap >= R:
        o["keys_sorted"][[i, i + 1]] = o["keys_sorted"][[i + 1, i]]            # (consistently: the list alone must give it away)
        o2 = new()
        o2["keys_sorted"][[i, i + 1]] = o2["keys_sorted"][[i + 1, i]]
        out["two sorted keys swapped"] = o2
    out["two entries of neighbouring depth swapped"] = o
    t = int(np.nonzero(ref["ranges"][:, 1] > ref["ranges"][:, 0])[0][1])
    for w, nm in ((0, "start"), (1, "end")):
        o = new()
        o["words"][2 * t + w] += 1
        out[f"a range's {nm} moved by one"] = o
    o = new()
    o["point_list"][cap] ^= 1
    out["a guard word behind point_list touched"] = o
    o = new()
    o["words"][BR.ranges_words(T) + 3] = 0
    out["a guard word behind the ranges words touched"] = o
    o = new()
    o["keys_sorted"][cap + BR.GUARD - 1] = 0
    out["a guard word behind keys_sorted touched"] = o
    o = new()
    o["num_rendered_out"] = min(R, cap) if cap < R else R - 1
    out["a wrong num_rendered_out"] = o
    o = new()
    o["words"][2 * T + 1] = o["words"][2 * T]
    out["an order table with a repeated tile"] = o
    o = new()
    per = (T + 7) // 8
    if T > 8:
        a, b = 2 * T, 2 * T + per                                              # first slots of bands 0 and 1
        o["words"][[a, b]] = o["words"][[b, a]]
        out["a tile in another band's slots"] = o
    cut = np.nonzero((ref["start"] < cap) & (ref["end"] > cap))[0]
    if len(cut):
        lo, hi = int(ref["lo"][cut[0]]), int(ref["hi"][cut[0]])
        o = new()
        o["point_list"][lo + 1] = o["point_list"][lo]
        out["an entry duplicated over another in the clipped tile"] = o
        o = new()
        o["point_list"][[lo, lo + 1]] = o["point_list"][[lo + 1, lo]]
        out["two entries of the clipped tile out of order"] = o
        o = new()
        other = ref["ids"][:int(ref["start"][cut[0]])]
        o["point_list"][lo] = other[0] if len(other) else ref["frame"].P - 1
        out["an entry of another tile in the clipped tile"] = o
    return out


def _accepts(ref, o):
    BR.compare(ref, o["point_list"], o["words"], o["keys_sorted"], o["num_rendered_out"])


@pytest.mark.parametrize("name, bound", [("lengths:bucket_ties/sparse", None), ("grid:13x5", None), ("bounds", None),
                                         ("bounds", "R+1"), ("bounds", "mid_long"), ("bounds", "R-1")])
def test_comparator_accepts_the_reference_and_rejects_every_corruption(name, bound):
    b = None if bound is None else BR.bounds_of(BR.reference("bounds"))[bound]
    ref = BR.reference(name, b)
    _accepts(ref, BR.perfect_output(ref))
    cases = _corruptions(ref)
    must = {"two tied ids swapped", "two entries of neighbouring depth swapped", "a range's start moved by one",
            "a guard word behind point_list touched", "a wrong num_rendered_out", "an order table with a repeated tile"}
    if ref["cap"] < ref["R"]:
        must |= {"an entry duplicated over another in the clipped tile"}
    assert must <= set(cases)
    for what, o in cases.items():
        with pytest.raises(AssertionError):
            _accepts(ref, o)
            pytest.fail(f"the comparator accepted: {what}", pytrace=False)


def test_cost_order_rule_accepts_class_order_and_rejects_a_reversed_band():
    T = 64
    lens = np.full(T, 5)
    cost = np.arange(T, dtype=np.uint32) * 9                                   # 0 .. 567: below, inside and above the classes
    per = T // 8
    words = np.zeros(BR.ranges_words(T), np.uint32)
    order = np.concatenate([np.arange(b * per, (b + 1) * per)[::-1] for b in range(8)])       # decreasing cost inside a band
    words[2 * T: 3 * T] = order
    BR.check_cost_order(words, T, cost, lens)
    words[2 * T: 3 * T] = np.arange(T)                                         # increasing
    with pytest.raises(AssertionError):
        BR.check_cost_order(words, T, cost, lens)


# ------------------------------------------------------------------------------------------------------- the one-call frames

@pytest.mark.parametrize("kind", BR.FWD_PATTERNS)
def test_every_gaussian_planted_for_the_one_call_frames_touches_its_tile_alone(kind):
    sc = BR.forward_scene(kind)
    assert sorted(sc.lens[sc.lens > 0].tolist()) == sorted(BR.FWD_LENGTHS) and sc.T == 192
    assert sc.P // sc.T < BR.DENSE_MEAN                                       # a capacity of R is sparse, 192 x 1 100 >= R is dense
    assert sc.T * BR.DENSE_MEAN >= sc.P
    rect, depth, visible = BR.oracle_rects(sc)
    assert visible.all()
    assert np.array_equal(depth.view(np.uint32), sc.key)                       # view depth = the planted z, to the bit
    assert ((rect[:, 2] - rect[:, 0] == 1) & (rect[:, 3] - rect[:, 1] == 1)).all()
    assert np.array_equal(rect[:, 1] * sc.gx + rect[:, 0], sc.tile)
    for t in np.nonzero(sc.lens)[0]:
        g = BR.tie_groups(sc.key[sc.tile == t])
        n = int(sc.lens[t])
        if kind == "spread":
            assert g[0] == 1
            if n == 20000:
                z = np.sort(sc.key[sc.tile == t].view(np.float32))
                assert z[2] < 0.5 < 1.0 <= z[3] and z[-4] <= 100.0 < 800 < z[-3]
        elif kind == "equal":
            assert g[0] == n
        else:
            assert list(g[:3]) == ([BR.LONG_BUCKET_MAX + 1, BR.LONG_BUCKET_MAX, 1] if n > 8192 else [BR.BUCKET_MAX + 1, BR.BUCKET_MAX, 1])
