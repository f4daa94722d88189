"""The LPIPS metric on the GPU (scgaussian_amd/lpips.py, csrc/lpips.hip) against the fp64 restatement of tests/lpips_refs.py: the
layer alone (scg_lp_conv3x3) at its tile, pool and rounding edges, then the whole call.

Bar, everywhere: max(4 e_ref, 1 fp32 ulp of the tensor's largest magnitude) in the max norm per tensor, no exclusion set.  e_ref is
the larger of two fp32 evaluations' deviations from fp64 on the same input: torch's fp32 convolution and the sequential fp32 chain.
For the layer it is computed here (the shapes are tiny); for the end-to-end scenes it is read from tests/golden/ref_lpips.npz, and
only the fp64 run (well under a second) is repeated.  Every comparison prints the kernel's deviation beside e_ref and the bar.

The head is symmetric in its two images bit for bit (the header says why), so swapping them is asserted bitwise."""
import numpy as np
import pytest
import torch

import eval_refs as ER
import lpips_refs as LR
from scgaussian_amd import _lib_lp, evaluate, lpips

pytestmark = pytest.mark.gpu
DEV = "cuda"
TM = _lib_lp.LP_TILE_M
PAIRS = sorted(set(lpips.CHANNELS))
FX = np.load(LR.GOLDEN)
WEIGHTS = LR.make_weights()
_CACHE = {}


def metric():
    if "lp" not in _CACHE:
        _CACHE["lp"] = lpips.Lpips.from_state_dicts(*LR.state_dicts(WEIGHTS), device=DEV)
    return _CACHE["lp"]


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


# ---- the layer alone ----------------------------------------------------------------------------------------------------------
def layer_inputs(cin, cout, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin, h, w), generator=g)
    if cin == 3:
        x = torch.rand((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.05
    return x, wt, b


def run_layer(x, wt, b, relu, pool=False, zscore=False):
    out = lpips.conv3x3(x.to(DEV), wt.to(DEV), b.to(DEV), relu=relu, pool=pool, zscore=zscore)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_layer(x, wt, b, pool, zscore, what):
    """Both ReLU settings of one layer call against fp64: the pre-activation's three evaluations are computed once, the ReLU is
    applied to each (it follows the sum in the rule), so e_ref is each setting's own."""
    pre = [LR.layer(x, wt, b, False, pool, zscore, dt, cv) for dt, cv in ((torch.float64, LR._conv_torch), (torch.float32, LR._conv_torch),
                                                                          (torch.float32, LR._conv_chain32))]
    for relu in (False, True):
        wide, a32, c32 = [np.maximum(p, 0) if relu else p for p in pre]
        e_ref = max(np.abs(a32 - wide).max(), np.abs(c32 - wide).max())
        got = run_layer(x, wt, b, relu, pool, zscore)
        assert got.shape == wide.shape and got.dtype == np.float32
        dev = np.abs(got.astype(np.float64) - wide).max()
        print(what, "relu" if relu else "linear", "deviation", dev, "e_ref", e_ref, "bar", LR.bar(e_ref, wide))
        assert dev <= LR.bar(e_ref, wide), (what, relu, dev, e_ref)
        if relu:
            assert not np.signbit(got[got == 0]).any() and (got >= 0).all()


@pytest.mark.parametrize("spatial", [(1, 1), (1, 2), (2, 1), (3, 3), (5, 7), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_layer_pairs_and_sizes(pair, spatial):
    (cin, cout), (h, w) = pair, spatial
    x, wt, b = layer_inputs(cin, cout, 2, h, w, seed=cin + cout + 7 * h + w)
    check_layer(x, wt, b, False, cin == 3, f"({cin},{cout}) {h}x{w}")
    if cin == 3:
        check_layer(x, wt, b, False, False, f"({cin},{cout}) {h}x{w} raw")


@pytest.mark.parametrize("spatial", [(2, 2), (2, 3), (3, 2), (3, 3), (5, 7), (6, 8), (16, 16), (17, 15)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", [(64, 128), (128, 256), (256, 512), (512, 512), (64, 64)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_layer_with_pool_at_even_and_odd_sizes(pair, spatial):
    (cin, cout), (h, w) = pair, spatial
    x, wt, b = layer_inputs(cin, cout, 2, h, w, seed=3 * cin + cout + 5 * h + w)
    check_layer(x, wt, b, True, False, f"({cin},{cout}) pooled {h}x{w}")


@pytest.mark.parametrize("pixels", [TM - 1, TM, TM + 1, 2 * TM + 1])
@pytest.mark.parametrize("pair", [(3, 64), (64, 64), (64, 128)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_layer_pixel_counts_around_the_tile(pair, pixels):
    cin, cout = pair
    x, wt, b = layer_inputs(cin, cout, 1, 1, pixels, seed=pixels + cin)
    check_layer(x, wt, b, False, cin == 3, f"({cin},{cout}) 1x{pixels}")
    if cin != 3:                                              # the pooled size is the pixel count; an odd row and column are dropped
        x, wt, b = layer_inputs(cin, cout, 1, 3, 2 * pixels + 1, seed=pixels + cin + 1)
        check_layer(x, wt, b, True, False, f"({cin},{cout}) pooled to 1x{pixels}")


@pytest.mark.parametrize("case", [(64, 128, 64, 128, False), (64, 128, 64, 129, False), (64, 128, 128, 259, True), (128, 256, 33, 127, False),
                                  (128, 256, 32, 128, False), (128, 256, 67, 255, True)], ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}{'p' if c[4] else ''}")
def test_layer_on_either_side_of_the_small_grid_threshold(case):
    """A layer with at most SMALL_GRID workgroups of 128 x 128 runs with 128 x 64 ones, so every small shape above goes that way.
    These are the smallest shapes beyond the threshold, and the largest ones on it: 64 -> 128 at 2 x 64 x 128 pixels has 128
    workgroups, at 2 x 64 x 129 it has 129; 128 -> 256 at 2 x 32 x 128 has 64 x 2, at 2 x 33 x 127 it has 66 x 2.  Pooled twins
    of the beyond side.  The bits do not depend on the tile: the same input runs as n = 1 halves (fewer workgroups, the narrow
    tile) and must give the halves of the n = 2 result."""
    cin, cout, h, w, pool = case
    x, wt, b = layer_inputs(cin, cout, 2, h, w, seed=h + w)
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    wide = -(-2 * ho * wo // TM) * (cout // 128) > _lib_lp.LP_SMALL_GRID
    assert wide == ((h, w) not in ((64, 128), (32, 128)))
    check_layer(x, wt, b, pool, False, f"({cin},{cout}) {h}x{w} {'wide' if wide else 'narrow'} tile")
    both = run_layer(x, wt, b, True, pool)
    halves = np.concatenate([run_layer(x[i:i + 1], wt, b, True, pool) for i in range(2)])
    assert -(-ho * wo // TM) * (cout // 128) <= _lib_lp.LP_SMALL_GRID          # a half alone runs with the narrow tile
    assert np.array_equal(both.view(np.uint32), halves.view(np.uint32))


@pytest.mark.parametrize("pair", [(3, 64), (64, 64), (256, 512)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_layer_planted_cases(pair):
    cin, cout = pair
    x, wt, b = layer_inputs(cin, cout, 2, 5, 7, seed=11)
    # a zero weight tensor: exactly relu(bias), and the bias itself without the ReLU
    got = run_layer(x, torch.zeros_like(wt), b, True)
    want = np.broadcast_to(np.maximum(b.numpy(), 0)[None, :, None, None], got.shape)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert np.array_equal(run_layer(x, torch.zeros_like(wt), b, False), np.broadcast_to(b.numpy()[None, :, None, None], got.shape))
    # pre-activations exactly zero (an exact cancellation, a zero bias on zero weights) or negative stay +0
    one = torch.zeros_like(x)
    one[:, 0, 2, 3] = 1.0
    w1 = torch.zeros_like(wt)
    w1[:, 0, 1, 1] = torch.linspace(-1.0, 1.0, cout)
    got = run_layer(one, w1, -w1[:, 0, 1, 1].clone(), True)          # centre: w - w = 0; elsewhere: relu(-w)
    assert (got[:, :, 2, 3] == 0).all() and not np.signbit(got).any()
    assert np.array_equal(got[0, :, 0, 0], np.maximum(-w1[:, 0, 1, 1].numpy(), 0))
    assert not run_layer(x, torch.zeros_like(wt), torch.zeros_like(b), True).view(np.uint32).any()          # +0 has no bit set
    # one nonzero input element: every output is one product plus the bias, bit for bit
    a = np.float32(0.7310586)
    one = torch.zeros_like(x)
    one[1, cin - 1, 2, 3] = float(a)
    got = run_layer(one, wt, b, False)
    want = np.broadcast_to(b.numpy()[None, :, None, None], got.shape).copy()
    for ky in range(3):
        for kx in range(3):
            y, xx = 2 - (ky - 1), 3 - (kx - 1)
            want[1, :, y, xx] = (a * wt[:, cin - 1, ky, kx].numpy()).astype(np.float32) + b.numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a denormal input, and a denormal weight: the products come through unflushed
    tiny = np.float32(3e-39)
    for xin, wv in ((float(tiny), 0.5), (0.5, float(tiny))):
        one = torch.zeros_like(x)
        one[0, 0, 2, 3] = xin
        w1 = torch.zeros_like(wt)
        w1[:, 0, 1, 1] = wv
        got = run_layer(one, w1, torch.zeros_like(b), False)
        want = np.float32(xin) * np.float32(wv)
        assert 0 < want < np.finfo(np.float32).tiny and (got[0, :, 2, 3] == want).all() and np.count_nonzero(got) == cout


# ---- end to end -------------------------------------------------------------------------------------------------------------
def run_metric(x, y, lp=None):
    lp = lp or metric()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    value = lp(xd, yd)
    terms = lp.terms.clone()
    fx, fy = lp.features(xd, yd)
    torch.cuda.synchronize()
    assert value.shape == (1, 1, 1, 1) and value.dtype == torch.float32 and value.is_cuda
    out = {"value": value.reshape(()).cpu().numpy(), "terms": terms.cpu().numpy()}
    for l in range(5):
        out[f"fx{l}"], out[f"fy{l}"] = fx[l][0].cpu().numpy(), fy[l][0].cpu().numpy()
    assert np.array_equal(bits(lp.terms), bits(terms))          # the features call ran the same network on the same pair
    return out


def compare(got, r64, e_ref, what):
    worst = []
    for k, wide in LR.tensors_of(r64).items():
        assert got[k].shape == wide.shape and got[k].dtype == np.float32, k
        dev = float(np.abs(got[k].astype(np.float64) - wide).max())
        print(what, k, "deviation", dev, "e_ref", e_ref[k], "bar", LR.bar(e_ref[k], wide))
        if not dev <= LR.bar(e_ref[k], wide):
            worst.append((k, dev, e_ref[k], LR.bar(e_ref[k], wide)))
    assert not worst, (what, worst)


@pytest.mark.parametrize("scene", LR.SCENES, ids=lambda s: LR.tag(s[0], s[1]))
def test_value_terms_and_features_against_the_fixture(scene):
    """16 x 16 ... 48 x 80, and the two shapes whose pixel counts straddle a multiple of the tile: 25 x 41 at the first resolution
    (2 H W = 16 TM + 2), 21 x 53 at the third (2 (H / 4)(W / 4) = TM + 2)."""
    H, W, seed = scene
    t = LR.tag(H, W)
    x, y = LR.make_images(H, W, seed)
    r64 = LR.rule(x, y, WEIGHTS)
    assert abs(float(r64["value"]) - float(FX[f"{t}_value"])) <= 1e-11 * float(r64["value"])          # the fixture's scene
    e_ref = dict(zip(FX[f"{t}_names"], np.maximum(FX[f"{t}_dev_torch32"], FX[f"{t}_dev_chain32"])))
    compare(run_metric(x, y), r64, e_ref, t)


def test_straddling_shapes_are_what_they_claim():
    assert (2 * 25 * 41) % TM == 2 and (2 * (21 // 4) * (53 // 4)) % TM == 2 and (25, 41, 9) in LR.SCENES and (21, 53, 10) in LR.SCENES


def test_equal_images_give_exactly_zero_and_a_swap_the_same_bits():
    lp = metric()
    x, y = LR.make_images(17, 19, 4)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    for other in (xd, xd.clone()):                      # x is y, x == y
        v = lp(xd, other)
        assert not bits(v).any() and not bits(lp.terms).any()
    a = lp(xd, yd)
    ta = lp.terms.clone()
    b = lp(yd[None], xd[None])                          # (1,3,H,W) as well
    assert float(a) > 1e-3 and np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ta), bits(lp.terms))
    fa, fb = lp.features(xd, yd)
    ga, gb = lp.features(yd, xd)
    assert all(torch.equal(p, q) for p, q in zip(fa + fb, gb + ga))
    assert all(torch.equal(p, q) for p, q in zip(lp.features(xd), fa))


def test_constant_images_against_fp64():
    """Every pixel's neighbourhood differs only by the border: the zero padding in the z domain decides all of it."""
    H, W = 16, 17
    x = np.broadcast_to(np.array([0.2, 0.5, 0.9], np.float32)[:, None, None], (3, H, W)).copy()
    y = np.broadcast_to(np.array([0.25, 0.45, 0.8], np.float32)[:, None, None], (3, H, W)).copy()
    r64 = LR.rule(x, y, WEIGHTS)
    e_ref = {k: max(a, b) for (k, a), b in zip(LR.deviations(r64, LR.rule(x, y, WEIGHTS, torch.float32)).items(),
                                               LR.deviations(r64, LR.chain32(x, y, WEIGHTS)).values())}
    assert float(r64["value"]) > 1e-4
    compare(run_metric(x, y), r64, e_ref, "constant")


def test_zeroed_layers_silence_the_later_taps_exactly():
    """conv4_3 and conv5_3 zeroed, weights and bias: taps 3 and 4 are all zero and contribute exactly 0 through the 1e-10; the
    taps in front keep their bits.  conv4_3 alone: tap 3 is all zero; tap 4 is the later biases' constant, the same bits for both
    images, so its term is exactly 0 as well."""
    x, y = LR.make_images(16, 17, 2)
    base = run_metric(x, y)
    zero = lambda p: (torch.zeros_like(p[0]), torch.zeros_like(p[1]))          # noqa: E731
    for layers, dead in (((9, 12), (3, 4)), ((9,), (3,))):
        convs = [zero(p) if i in layers else p for i, p in enumerate(WEIGHTS[0])]
        got = run_metric(x, y, lpips.Lpips(convs, WEIGHTS[1], device=DEV))
        assert not got["terms"][3:].view(np.uint32).any(), layers
        assert all(not np.ascontiguousarray(got[f"f{s}{l}"]).view(np.uint32).any() for s in "xy" for l in dead), layers
        assert np.array_equal(got["terms"][:3].view(np.uint32), base["terms"][:3].view(np.uint32))
        assert all(np.array_equal(got[f"fx{l}"], base[f"fx{l}"]) for l in range(3))
        assert abs(float(got["value"]) - float(base["terms"][:3].astype(np.float64).sum())) <= 2 * LR.ulp(got["value"])
        if dead == (3,):
            assert got["fx4"].any() and np.array_equal(got["fx4"], got["fy4"])


def test_a_nan_or_infinite_pixel_gives_nan():
    lp = metric()
    x, y = LR.make_images(17, 16, 3)
    for bad, where in ((np.nan, (1, 5, 6)), (np.inf, (0, 16, 15)), (-np.inf, (2, 0, 0))):
        xb = x.copy()
        xb[where] = bad
        assert torch.isnan(lp(torch.from_numpy(xb).to(DEV), torch.from_numpy(y).to(DEV))).all(), (bad, where)
        assert torch.isnan(lp(torch.from_numpy(y).to(DEV), torch.from_numpy(xb).to(DEV))).all(), (bad, where)


def test_refusals():
    lp = metric()
    for shape in ((3, 15, 16), (3, 16, 15), (4, 16, 16), (16, 16)):
        with pytest.raises(ValueError):
            lp(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError, match="one shape"):
        lp(torch.zeros((3, 16, 16), device=DEV), torch.zeros((3, 16, 17), device=DEV))
    vgg, lin = LR.state_dicts(WEIGHTS)
    with pytest.raises(ValueError, match=r"features\.28\.weight"):
        lpips.Lpips.from_state_dicts({k: v for k, v in vgg.items() if k != "features.28.weight"}, lin, device=DEV)
    with pytest.raises(ValueError, match=r"lin4"):
        lpips.Lpips.from_state_dicts(vgg, {**lin, "lin4.model.1.weight": torch.zeros(1, 256, 1, 1)}, device=DEV)
    lib = _lib_lp.load()
    assert lib.scg_lp_forward(15, 16, 16, 16, 16, 16, 16, None, 16, 1 << 40, None) == -2          # refused before any launch


def test_both_key_spellings_and_two_runs_give_the_same_bits():
    x, y = LR.make_images(31, 33, 5)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    other = lpips.Lpips.from_state_dicts(*LR.state_dicts(WEIGHTS, vgg_prefix="", published=False), device=DEV)
    a, b, c = metric()(xd, yd).clone(), metric()(xd, yd).clone(), other(xd, yd)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)) and np.array_equal(bits(metric().terms), bits(other.terms))
    f1, f2 = metric().features(xd), metric().features(xd)
    assert all(torch.equal(p, q) for p, q in zip(f1, f2))
    a = metric()(xd, yd).clone()                          # the head alone on the taps this call left: the same bits
    ta = metric().terms.clone()
    h = metric().head(31, 33)
    assert np.array_equal(bits(a), bits(h)) and np.array_equal(bits(ta), bits(metric().terms)) and bits(a).any()


def test_a_call_in_a_graph_replayed_on_rewritten_images_equals_eager():
    lp = metric()
    (x1, y1), (x2, y2) = LR.make_images(17, 19, 4), LR.make_images(17, 19, 40)
    xd, yd = torch.from_numpy(x1).to(DEV), torch.from_numpy(y1).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lp(xd, yd)                                      # warm: the scratch of this size exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        value = lp(xd, yd)
        terms = lp.terms
    xd.copy_(torch.from_numpy(x2))
    yd.copy_(torch.from_numpy(y2))
    graph.replay()
    torch.cuda.synchronize()
    replayed = (value.clone(), terms.clone())
    eager = lp(torch.from_numpy(x2).to(DEV), torch.from_numpy(y2).to(DEV))
    assert np.array_equal(bits(replayed[0]), bits(eager)) and np.array_equal(bits(replayed[1]), bits(lp.terms))
    assert float(eager) != float(lp(torch.from_numpy(x1).to(DEV), torch.from_numpy(y1).to(DEV)))


def _count_reads(monkeypatch):
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda orig, name: lambda self, *a, **k: (reads.append(name) if self.is_cuda else None,
                                                                                         orig(self, *a, **k))[1])(orig, name))
    return reads


def test_no_host_read_during_a_call(monkeypatch):
    lp = metric()
    x, y = LR.make_images(16, 16, 1)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    lp(xd, yd)
    torch.cuda.synchronize()
    reads = _count_reads(monkeypatch)
    v = lp(xd, yd)
    lp.features(xd, yd)
    assert reads == [] and v.is_cuda
    assert v.cpu().shape == (1, 1, 1, 1) and reads == ["cpu"]          # the counter counts


def test_eval_set_reports_lpips_and_avg_with_one_host_read(monkeypatch):
    lp = metric()
    shapes = [(17, 19), (16, 33), (21, 18)]
    views = [ER.images(H, W, seed=60 + i) for i, (H, W) in enumerate(shapes)]
    names = [f"{i:05d}.png" for i in range(3)]
    es = evaluate.EvalSet(3, lpips_fn=lp)
    reads = _count_reads(monkeypatch)
    outs = [es.add(names[i], r.to(DEV), g.to(DEV), d.to(DEV)) for i, (r, g, d) in enumerate(views)]
    assert reads == []
    full, per_view = es.results()
    assert reads == ["cpu"]                              # the set's one host read
    monkeypatch.undo()
    assert set(full) == set(per_view) == {"SSIM", "PSNR", "LPIPS", "AVG"} and list(per_view["LPIPS"]) == names
    want = [float(lp(o["renders_masked"], o["gt_masked"])) for o in outs]          # the masked images, one view at a time
    assert [per_view["LPIPS"][k] for k in names] == want and len(set(want)) == 3 and all(0 < v < 10 for v in want)
    for k, l in zip(names, want):                        # metrics.py:91
        p, s = torch.tensor(per_view["PSNR"][k]), torch.tensor(per_view["SSIM"][k])
        avg = torch.exp(torch.log(torch.tensor([10 ** (-p / 10), torch.sqrt(1 - s), l])).mean()).item()
        assert per_view["AVG"][k] == pytest.approx(avg, rel=1e-6)
    assert full["LPIPS"] == torch.tensor(want).mean().item()
    assert full["AVG"] == torch.tensor(want).mean().item()          # metrics.py:107 as it stands: the mean of the LPIPS values
