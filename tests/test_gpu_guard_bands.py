"""Guard bands around every buffer the HIP libraries are handed (tests/guarded_alloc.py), one table of cases over the compute
entries of every header under include/.

The parity tests show that the bytes INSIDE the outputs are right.  The caching allocator rounds every allocation up and carves it
from large blocks, so a vector tail that lands a few bytes past a buffer, or a workspace-size function that reports a few bytes too
little, changes nothing those tests look at.  Here every case runs three times — under fill A, under fill B, unguarded — and holds:

  1. no band of any allocation is touched, under A and under B;
  2. every device pointer the binding passes to a library lies inside a guarded body of the current run (a case's `excused` names
     the exceptions, by entry and parameter as the header spells it: queue handles, pinned host words, and inputs the wrapper
     itself derives with torch arithmetic or uploads — never an output or a scratch buffer in device memory);
  3. every output / scratch parameter of the header was seen non-NULL at least once (a case's `not_passed` names the optional ones
     it leaves out, `fields` the outputs inside struct arguments);
  4. the public results of the three runs are bit-identical — except where float atomics sum them, held to the module's own bar.

A difference between A and B means bytes outside an input reached a result: a finding of the same rank as a touched band.  No case
plants an out-of-range value; every call is one the wrappers make today at sizes the suite already uses.

Index reads, audited by reading the kernels before the first guarded run (the wider-integer fills are the valid indices 1 and 2 all
the same; none needed a fix): the segment tables of seed.hip and matchpoint.hip are copied to LDS with s < nseg and searched inside
[0, nseg - 1], a segment's view is used only when 0 <= view < V, and a winner index only when 0 <= wi < N; mono.hip reads its group,
segment and view tables at blockIdx (the launch dimensions are their lengths) and checks segment, partner and view before use;
pngpack.hip checks a chunk's image index against the image count; resample.hip clamps the column index to wout - 1 and a bound to
[0, win - 1]; the geocheck pair table is written by scg_geocheck_setup itself; scg_sort_pairs and scg_inclusive_scan_u32 take
their integers as values, never as addresses; scg_densify_stats compares radii with 0.
"""
import contextlib
import glob
import math
import os
import re
import time

import numpy as np
import pytest
import torch

import abi_text
from guarded_alloc import FILL_A, FILL_B, guarded, traced
from scgaussian_amd import _lib_lp, _lib_mp, _lib_vw, ply as _ply_module

pytestmark = pytest.mark.gpu
DEV = "cuda"
MP_T, PLY_T, VW_T, LP_TM = _lib_mp.MP_TILE_RECORDS, _ply_module.TILE_ROWS, _lib_vw.VW_TILE, _lib_lp.LP_TILE_M      # the kernels' tiles
HEADERS = sorted(glob.glob(os.path.join(abi_text.INCLUDE, "**", "*.h"), recursive=True))


# ---- the headers' text: parameter names, and which pointers are written -------------------------------------------------------------

def _header_functions():
    """{entry: [(parameter name, is a pointer, is const)]} of every SCG_API prototype under include/."""
    out = {}
    for path in HEADERS:
        with open(path) as fh:
            code = abi_text.strip_comments(fh.read())
        for m in re.finditer(r"SCG_API\s+[^;(]+?\b(scg_[a-z0-9_]+)\s*\(([^()]*)\)", code):
            params = []
            for p in (q.strip() for q in m.group(2).split(",")):
                if p and p != "void":
                    params.append((re.search(r"(\w+)\s*$", p).group(1), "*" in p, "const" in p))
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = params
    return out


FUNCTIONS = _header_functions()
HANDLES = {"stream", "event", "stage_events"}                     # queue / event handles and the host struct of event handles


def written_parameters(entry):
    """The output and scratch parameters of an entry: its non-const pointers that are no handle."""
    return [n for n, ptr, const in FUNCTIONS[entry] if ptr and not const and n not in HANDLES]


def _name_of(entry, path):
    """(argument index, field, ...) of a traced pointer -> `param` or `param.field.sub`, the parameter as the header spells it."""
    return ".".join([FUNCTIONS[entry][path[0]][0]] + [str(p) for p in path[1:]])


# ---- the binding's libraries, traced ---------------------------------------------------------------------------------------------

def _lib_modules():
    from scgaussian_amd import _lib, _lib_img, _lib_io, _lib_lp, _lib_mp, _lib_png, _lib_vw
    return (_lib, _lib_io, _lib_img, _lib_mp, _lib_vw, _lib_lp, _lib_png)


@contextlib.contextmanager
def tracing():
    """Every library handle of the binding replaced by traced(handle) sharing one list of calls; restored on exit."""
    calls, saved = [], []
    try:
        for mod in _lib_modules():
            real = mod.load()
            saved.append((mod, real))
            mod._lib = traced(real, calls)
        yield calls
    finally:
        for mod, real in saved:
            mod._lib = real


def _clear_caches():
    """The binding's process-global caches hold device buffers of earlier tests: emptied here, in place (other modules hold the same
    dictionaries by name), so that every buffer of a case is allocated inside its own guarded run (condition 2 fails otherwise)."""
    from scgaussian_amd import _counts, _grads, model_path, rasterizer
    rasterizer._FRAME_CACHE.clear()
    rasterizer._CAM_HINTS.clear()
    _grads._ARENA_POOLS.clear()
    _grads._LAYOUTS.clear()
    model_path._ACCEPTS.clear()
    _counts._SPEC_STATE.clear()


# ---- a case --------------------------------------------------------------------------------------------------------------------------

class Case:
    """run(home) builds the inputs with the module's generator, moves them with home() (Registry.rehome under a guard, the identity
    without), calls the public entry once and returns {name: tensor or number}.
    entries: the library entries the case must reach.  excused: {entry: {parameter: why}} — pointers that need not lie in a body.
    not_passed: {entry: {parameter}} — optional outputs this case leaves NULL.  fields: {entry: [dotted struct fields]} that must be
    seen non-NULL (outputs inside struct arguments, which carry no const; STRUCT_OUTPUT_ENTRIES names the entries for which a case
    must list them).  close: result name -> f(a, b, what) for the results that float atomics sum, None for the others, which are
    compared bit for bit."""

    def __init__(self, id, run, entries, excused=None, not_passed=None, fields=None, close=None):
        self.id, self.run, self.entries = id, run, tuple(entries)
        self.excused, self.not_passed, self.fields = excused or {}, not_passed or {}, fields or {}
        self.close = (lambda name: None) if close is None else close


def _to_host(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().contiguous()
    if isinstance(obj, dict):
        return {k: _to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_to_host(v) for v in obj]
    return obj


def _run_once(case, fill):
    _clear_caches()
    with tracing() as calls:
        if fill is None:
            out = case.run(lambda x: x)
            torch.cuda.synchronize()
            return _to_host(out), calls, None
        with guarded(fill) as reg:
            out = case.run(reg.rehome)
            torch.cuda.synchronize()
            out = _to_host(out)
    return out, calls, reg


def _same_bits(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and \
            torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same_bits(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


SEEN = set()                                                      # every entry a case of this file reached (the coverage test)
TIMES = {}
# the entries that write device memory through the pointer fields of a struct argument (the headers' comments say which fields):
# the header's text gives those fields no const to tell them by, so every case that reaches one lists them by hand
STRUCT_OUTPUT_ENTRIES = ("scg_densify_scatter", "scg_seed_scatter", "scg_mono_images", "scg_mono_matches", "scg_mono_pairs",
                         "scg_ply_unpack", "scg_backward_model", "scg_forward", "scg_forward_model", "scg_backward")


def check_case(case):
    t0 = time.perf_counter()
    runs = {}
    for fill in (FILL_A, FILL_B, None):
        out, calls, reg = _run_once(case, fill)
        runs[fill] = out
        names = {c.name for c in calls}
        SEEN.update(names)
        missing = [e for e in case.entries if e not in names]
        assert not missing, f"{case.id}: the case never called {missing} (it called {sorted(names)})"
        if reg is None:
            continue
        # 1. no band touched
        touched = reg.check()
        assert touched == [], f"{case.id} under fill {fill}: {len(touched)} band(s) touched: {touched[:8]}"
        # 2. every device pointer inside a guarded body of this run
        stray, seen = [], {}
        for c in calls:
            if c.name not in FUNCTIONS:
                continue
            for path, value in c.pointers:
                name = _name_of(c.name, path)
                if not value:
                    continue                                      # NULL: condition 3 holds the outputs to be passed
                seen.setdefault(c.name, set()).add(name)
                top = name.split(".")[0]
                if top in HANDLES or name in case.excused.get(c.name, {}) or top in case.excused.get(c.name, {}):
                    continue
                if not reg.covers(value):
                    stray.append(f"{c.name}({name}) = {value:#x}")
        assert not stray, f"{case.id} under fill {fill}: pointers outside every guarded body: {sorted(set(stray))}"
        # 3. the outputs and scratch buffers the header names were passed
        for entry in names & set(FUNCTIONS):
            want = [n for n in written_parameters(entry) if n not in case.not_passed.get(entry, ())]
            want = [n for n in want if not _is_struct_parameter(entry, n)] + list(case.fields.get(entry, ()))
            absent = [n for n in want if n not in seen.get(entry, set())]
            assert not absent, f"{case.id}: {entry} never received a non-NULL {absent}"
            assert entry not in STRUCT_OUTPUT_ENTRIES or case.fields.get(entry), \
                f"{case.id}: {entry} writes through the fields of a struct argument; the case must list them in `fields`"
        for entry, excused in case.excused.items():               # no excuse for an output or a scratch buffer in device memory:
            for name, why in excused.items():                     # a struct field carries no const, so only host memory is excused there
                host = why.startswith(("pinned host", "host"))
                assert host or ("." not in name and name not in written_parameters(entry)), (case.id, entry, name, "excuses an output")
                assert name not in {f for f in case.fields.get(entry, ())}, (case.id, entry, name, "is excused and required")
    # 4. the same results under A, under B and unguarded
    for other in (FILL_B, None):
        a, b = runs[FILL_A], runs[other]
        assert a.keys() == b.keys()
        for k in a:
            what = f"{case.id}: result {k!r} under fill A and {'under fill B' if other else 'unguarded'}"
            compare = case.close(k)
            if compare is not None:
                compare(a[k], b[k], what)
            else:
                assert _same_bits(a[k], b[k]), what + " differ"
    TIMES[case.id] = time.perf_counter() - t0


def _is_struct_parameter(entry, name):
    """Parameters the binding declares as a typed pointer (a host struct, table or word of the call) and not as a plain address:
    their device pointers, if any, are the struct's fields."""
    import ctypes
    for mod in _lib_modules():
        if entry in mod.SYMBOLS:
            argtypes = mod.SYMBOLS[entry][1]
            index = [n for n, _, _ in FUNCTIONS[entry]].index(name)
            return argtypes[index] is not ctypes.c_void_p
    raise KeyError(entry)


# ---- helpers shared by the cases -----------------------------------------------------------------------------------------------------

def _rel(tol):
    def close(a, b, what):
        a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
        scale = max(float(b.abs().max()) if b.numel() else 0.0, 1e-30)
        err = float((a - b).abs().max()) / scale if b.numel() else 0.0
        print(f"GUARD {what}: {err:.3e} of the largest entry (bar {tol:g})")
        assert math.isfinite(err) and err <= tol, (what, err, tol)
    return close


def _scalar(x):
    return torch.tensor(x, dtype=torch.float32, device=DEV)       # (a patched name: guarded under a guard)


# ---- image loss (scg_loss.h) -----------------------------------------------------------------------------------------------------

def _image_loss(shape, lam):
    def run(home):
        import test_image_loss as T
        from scgaussian_amd import losses
        x, y = T._content("random", shape, seed=sum(shape))
        xd, yd = home(x.to(DEV).requires_grad_(True)), home(y.to(DEV))
        loss = losses.image_loss(xd, yd, lam)
        loss.backward(_scalar(-2.5))
        with torch.no_grad():
            plain = losses.image_loss(home(x.to(DEV)), yd, lam)
        return dict(loss=loss, grad=xd.grad, plain=plain)
    return Case(f"image_loss_combined-{'x'.join(map(str, shape))}-lam{lam}", run,
                ["scg_image_loss_forward_combined", "scg_image_loss_backward_combined"])


def _image_loss_pair(shape):
    def run(home):
        import test_image_loss as T
        from scgaussian_amd import losses
        x, y = T._content("hdr", shape, seed=sum(shape) + 1)
        xd, yd = home(x.to(DEV).requires_grad_(True)), home(y.to(DEV))
        l1, ss = losses.l1_and_ssim(xd, yd)
        torch.autograd.backward([l1, ss], [_scalar(0.8), _scalar(-0.2)])
        return dict(l1=l1, ssim=ss, grad=xd.grad)
    return Case(f"image_loss_pair-{'x'.join(map(str, shape))}", run, ["scg_image_loss_forward", "scg_image_loss_backward"],
                excused={"scg_image_loss_backward": {"weights": "two words the wrapper forms with torch.stack(...) * (1 / n)"}})


# ---- match loss (scg_matchloss.h) --------------------------------------------------------------------------------------------------

def _match_loss(M):
    def run(home):
        import test_match_loss as T
        from scgaussian_amd.match_loss import match_loss_from_depth
        cam0, cams = T._cams(T.MW, T.MH)
        depth = T._depth(T.MW, T.MH, 1000 + M)
        uvs = [T._random_uv0(T.MW, T.MH, M, 31 * M + k) for k in range(2)]
        uvs[0][M - 1] = torch.tensor([140.25, 90.5])
        pairs = [T._pair_from_uv0(cam0, c, depth, uvs[k], 77 * M + k) for k, c in enumerate(cams)]
        d = home(depth.clone().to(DEV)[None].requires_grad_(True))
        out = match_loss_from_depth(d, [home(T._to_cuda(p)) for p in pairs], float(T.MW), float(T.MH))
        out.backward(_scalar(0.3))
        return dict(loss=out, grad=d.grad)
    # the loss word and the gradient image are summed over matches and pairs by float atomics: the module's own bars
    return Case(f"match_loss-M{M}", run, ["scg_match_loss_pair"], close={"loss": _rel(1e-6), "grad": _rel(1e-4)}.get)


# ---- kNN (scg_knn.h) ----------------------------------------------------------------------------------------------------------------

def _knn(n):
    def run(home):
        import loss_refs as lr
        from simple_knn._C import distCUDA2
        return dict(dist2=distCUDA2(home(torch.from_numpy(lr.aniso_cloud(n, 7 * n + 1)).to(DEV))))
    return Case(f"knn-{n}", run, ["scg_knn3_mean_dist2_ws"])


# ---- the standalone integer primitives (scg_raster.h) ------------------------------------------------------------------------------

def _sort(n):
    def run(home):
        from scgaussian_amd import _lib
        lib = _lib.load()
        rng = np.random.default_rng(n * 131)
        keys = rng.integers(0, 2 ** 62, size=n, dtype=np.int64) & ((1 << 41) - 1)
        k_in, v_in = home(torch.from_numpy(keys).to(DEV)), torch.arange(n, dtype=torch.int32, device=DEV)
        k_out, v_out = torch.empty_like(k_in), torch.empty_like(v_in)
        scratch = torch.empty(lib.scg_sort_scratch_bytes(n), dtype=torch.uint8, device=DEV)
        _lib.check(lib.scg_sort_pairs(k_in.data_ptr(), v_in.data_ptr(), k_out.data_ptr(), v_out.data_ptr(), n, 41,
                                      scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream), "sort")
        torch.cuda.synchronize()
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(k_out.cpu().numpy(), keys[order]) and np.array_equal(v_out.cpu().numpy(), order.astype(np.int32))
        return dict(keys=k_out, vals=v_out)
    return Case(f"sort_pairs-{n}", run, ["scg_sort_pairs"])


def _scan(n):
    def run(home):
        from scgaussian_amd import _lib
        lib = _lib.load()
        x = np.random.default_rng(n).integers(0, 300, size=n, dtype=np.int32)
        t_in = home(torch.from_numpy(x).to(DEV))
        t_out = torch.empty_like(t_in)
        total = torch.zeros(1, dtype=torch.int32, device=DEV)
        scratch = torch.empty(lib.scg_scan_scratch_bytes(n), dtype=torch.uint8, device=DEV)
        _lib.check(lib.scg_inclusive_scan_u32(t_in.data_ptr(), t_out.data_ptr(), n, total.data_ptr(), scratch.data_ptr(),
                                              scratch.numel(), torch.cuda.current_stream().cuda_stream), "scan")
        torch.cuda.synchronize()
        assert np.array_equal(t_out.cpu().numpy(), np.cumsum(x).astype(np.int32)) and int(total) == int(x.sum())
        return dict(out=t_out, total=total)
    return Case(f"inclusive_scan-{n}", run, ["scg_inclusive_scan_u32"])


# ---- DTU (scg_loss.h) ---------------------------------------------------------------------------------------------------------------

def _dtu(n):
    def run(home):
        import dtu_refs as DR
        import test_gpu_dtu as T
        from scgaussian_amd import dtu
        H, W = T.SIZES[n]
        g = torch.Generator().manual_seed(n)
        view = dtu.DtuView(home(DR.dark_run_image(H, W, seed=n, dark_share=0.8).to(DEV)))
        alpha = home(torch.rand(1, H, W, generator=g).to(DEV).requires_grad_(True))
        term = dtu.alpha_term(alpha, view)
        term.backward(_scalar(0.7))
        img, gt = (home((torch.rand(3, H, W, generator=g) * 1.8 - 0.4).to(DEV)) for _ in range(2))
        m = torch.randn(H, W, generator=g)
        m[m.abs() < 0.3] = 0.0
        l1, psnr, mse = dtu.eval_metrics_all(img, gt, home(m.to(DEV)))
        return dict(mask=view.mask, gt=view.gt, count=view.count, term=term, grad=alpha.grad, l1=l1, psnr=psnr, mse=mse)
    return Case(f"dtu-{n}", run, ["scg_dtu_bg_mask", "scg_masked_mean_forward", "scg_masked_mean_backward", "scg_eval_metrics"])


# ---- the evaluation view (scg_eval.h) -------------------------------------------------------------------------------------------------

def _eval_view(masked):
    def run(home):
        import eval_refs as ER
        import test_gpu_eval as T
        from scgaussian_amd import evaluate
        H, W = T.TH + 1, T.TW + 1
        render, gt, depth = ER.images(H, W, seed=100 * H + W, outside=True)
        mask = home(T._mask(H, W, 7 * H + W).to(DEV)) if masked else None
        out = evaluate.evaluate_view(home(render.to(DEV)), home(gt.to(DEV)), home(depth.to(DEV)), mask)
        return {k: v for k, v in out.items() if v is not None}
    return Case(f"eval_view-{'masked' if masked else 'plain'}", run, ["scg_eval_depth_range", "scg_eval_view", "scg_image_loss_forward"],
                not_passed={"scg_image_loss_forward": {"dmaps"}, "scg_eval_view": set() if masked else {"mask_u8"}})


# ---- geocheck (scg_geocheck.h) -------------------------------------------------------------------------------------------------------

def _geocheck(n, H, W):
    def run(home):
        import test_gpu_geocheck as T
        from scgaussian_amd import geo_check as gc
        intrs, exts, depths = T._close_scene(n, H, W, seed=100 + 7 * H + W)
        chk = gc.GeoCheck(n, H, W, num_src=2, device=torch.device(DEV, 0))
        chk.setup(home(torch.from_numpy(intrs).to(DEV)), home(torch.from_numpy(exts).to(DEV)))      # fp64: used as they are
        fd, fm = chk.run(home(torch.from_numpy(depths).to(DEV)), view_thresh=0)
        return dict(filtered=fd, masks=fm, votes=chk.votes, pairs=chk.pairs)
    return Case(f"geocheck-{n}x{H}x{W}", run, ["scg_geocheck_setup", "scg_geocheck"])


# ---- depth colour maps (scg_viz.h) ---------------------------------------------------------------------------------------------------

def _viz(H, W):
    def run(home):
        from scgaussian_amd import video
        rng = np.random.default_rng(H * 2000 + W)
        x = home(torch.from_numpy(rng.random((H, W), dtype=np.float32) * 5 + 1).to(DEV))
        render = home(torch.from_numpy(rng.random((3, H, W), dtype=np.float32) * 1.4 - 0.2).to(DEV))
        viz = home(video.DepthColorizer(H, W))                    # (its table is uploaded with .to(device): moved too)
        r = viz.depth_range(x)
        outs = {k: torch.empty((H, W) if k == "depth_u8" else (H, W, 3), dtype=torch.uint8, device=DEV)
                for k in ("depth_color", "depth_color_bgr", "depth_u8", "render_u8", "frame_bgr")}
        viz.frame(x, r, render=render, **outs)
        stats = viz.stats(x).clone()
        return dict(outs, range=r, stats=stats, nan=viz._nan)
    return Case(f"viz-{H}x{W}", run, ["scg_eval_depth_range", "scg_viz_select", "scg_viz_frame"])


# ---- densify, reset-opacity, densification statistics (scg_raster.h) -------------------------------------------------------------

def _model_results(m):
    import densify_refs as D
    out = {a: getattr(m, a) for a in [r[0] for r in D.RAY + D.BG] + [f[0] for f in D.FIXED + D.STATS]}
    for opt, tag in ((m.optimizer, "ray"), (m.optimizer_bg, "bg")):
        for g in opt.param_groups:
            st = opt.state.get(g["params"][0])
            if st:
                out[f"{tag}.{g['name']}.exp_avg"], out[f"{tag}.{g['name']}.exp_avg_sq"] = st["exp_avg"], st["exp_avg_sq"]
    return out


def _densify(nr, nb):
    def run(home):
        import test_gpu_densify as T
        from scgaussian_amd import densify
        t, states, noise = T.make_inputs(nr, nb, 100 + nr, "mixed")
        m = home(T.build(t, states, DEV, torch.optim.Adam))       # the model, both optimizers and their moments, moved together
        densify.install(m)
        m.densify_and_prune(T.MAX_GRAD, T.MIN_OPACITY, T.EXTENT, 20, noise=home(noise.to(DEV)))
        mid = {k: v.detach().clone() for k, v in _model_results(m).items()}
        m.reset_opacity()
        return dict(after_densify=mid, after_reset=_model_results(m))
    bg = ["args.out." + f for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")] if nb else []
    return Case(f"densify-{nr}+{nb}", run, ["scg_densify_classify", "scg_densify_scatter", "scg_reset_opacity"],
                fields={"scg_densify_scatter": bg + ["args.accum", "args.denom", "args.max_radii2D", "args.ray_scaling"]},
                not_passed={"scg_reset_opacity": set() if nb else {"bg_opacity", "bg_exp_avg", "bg_exp_avg_sq"}})


def _densify_stats(P):
    def run(home):
        from scgaussian_amd import optim
        g = torch.Generator().manual_seed(P)
        radii = home((torch.randint(0, 9, (P,), generator=g, dtype=torch.int32) * (torch.rand(P, generator=g) < 0.7)).to(DEV))
        grad = home(torch.randn(P, 3, generator=g).to(DEV))       # row stride 3: the third column is not the kernel's
        max_radii, accum, denom = (home(torch.rand(P, *tail, generator=g).to(DEV)) for tail in ((), (1,), (1,)))
        optim.densification_stats(max_radii, accum, denom, grad, radii)
        return dict(max_radii2D=max_radii, accum=accum, denom=denom)
    return Case(f"densify_stats-{P}", run, ["scg_densify_stats"])


# ---- seeding (scg_raster.h) --------------------------------------------------------------------------------------------------------

def _seed(N):
    def run(home):
        import test_gpu_seed as T
        from scgaussian_amd import seed
        parts = min(N, 6)
        arena = T.random_arena(N, T.split(N, parts, N), [s % 3 for s in range(parts)], 3, seed_=N)
        keep = torch.arange(N) % 3 != 1                           # two of three matches pass the threshold, the first among them
        arena["min_loss"] = torch.where(keep, 0.01, 0.5).to(DEV)
        arena = {k: home(v) if torch.is_tensor(v) else v for k, v in arena.items()}
        inputs = home(T.inputs_of(arena))                         # (its device segment table is uploaded with .to(device): moved too)
        out = seed.seed_arrays(inputs, arena["min_loss"])
        assert 0 < out["n"] <= N
        return out
    outs = ["args." + f for f in ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "opacity_out",
                                  "max_radii2D")]
    return Case(f"seed-{N}", run, ["scg_seed_classify", "scg_seed_scatter", "scg_knn3_mean_dist2_ws", "scg_seed_finish"],
                fields={"scg_seed_scatter": outs}, excused={"scg_seed_scatter": {"args.segments": "host copy of the segment table"}})


# ---- scene setup (scg_mono.h) ------------------------------------------------------------------------------------------------------

MONO_OUTPUTS = ["a." + n for n in ("image_color", "uv", "color", "blender_mask", "rays_o", "rays_d", "cam_rays_d", "cam_z", "z", "uv_t",
                                   "valid", "wgt", "counts")]


def _mono(which):
    def run(home):
        import mono_refs as MR
        import test_gpu_mono as T
        from scgaussian_amd import mono
        if which == "two_views":                                  # the edge file's smallest scene: two 16 x 16 views, one match
            ramp = (np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256).astype(np.uint8)
            cams = [MR.camera("a", ramp, np.eye(3), (0, 0, 0), 1.0, 1.0, (1, 2)),
                    MR.camera("b", ramp[::-1].copy(), np.eye(3), (0, 0, 0), 1.0, 1.0, (1, 2))]
            md, u = {"a": {"b": np.array([[0.5, 0.5]])}, "b": {"a": np.array([[0.5, 0.5]])}}, np.zeros(2, dtype=np.float32)
        else:
            cams, md, u = T.edge_scene()
        setup = mono.MonoSetup.build(cams, md, DEV, u)
        return {k: getattr(setup, k) for k in T.OUT}
    return Case(f"mono-{which}", run, ["scg_mono_images", "scg_mono_matches", "scg_mono_pairs"],
                fields={e: MONO_OUTPUTS for e in ("scg_mono_images", "scg_mono_matches", "scg_mono_pairs")})


# ---- the init stage's snapshot (mp/scg_matchpoint.h) ---------------------------------------------------------------------------------

def _matchpoint(N):
    def run(home):
        import matchpoint_refs as MR
        import test_gpu_matchpoint as T
        from scgaussian_amd import matchpoint
        arena = MR.random_arena([N], [0], [(5, 6)], seed=N)
        inputs = home(T.inputs_of(arena, home(T.tensors(arena))))  # (the two device tables are uploaded by the constructor: moved too)
        snap = matchpoint.pack(inputs)
        return dict(buffer=snap.buffer)
    return Case(f"matchpoint-{N}", run, ["scg_mp_pack"],
                excused={"scg_mp_pack": {"args.segments": "host copy of the segment table", "args.views": "host copy of the view table"}})


# ---- scene save and load (io/scg_ply.h) ----------------------------------------------------------------------------------------------

def _ply(nr, nb):
    def run(home):
        import tempfile
        import ply_refs as R
        import test_gpu_ply as T
        from scgaussian_amd import ply, ply_io
        m = T._np_model(nr, nb)
        model = home(T._ray_bound(m))
        packed = ply.pack(model)
        out = dict(buffer=packed.buffer)
        cam = home(torch.tensor([0.3, -0.2, 4.0], dtype=torch.float32, device=DEV))
        with tempfile.TemporaryDirectory() as folder:
            for deg in range(4):                                  # every degree of the colour view
                ply.save_color_pcd(model, cam, os.path.join(folder, f"deg{deg}"), sh_degree=deg)
                with open(os.path.join(folder, f"deg{deg}", "point_cloud_color.ply"), "rb") as fh:
                    out[f"color{deg}"] = fh.read()
            path = os.path.join(folder, "point_cloud.ply")
            packed.write(path)
            loaded = ply_io.RayBoundModel(**{k: torch.zeros((1,) + R.TAILS[k]) for k in R.RAY_KEYS})
            took = ply.load_ply(loaded, path)
            assert took == ({"ray": True, "bg": True} if nb else {"ray": True})
        for k in R.RAY_KEYS + R.BG_KEYS:
            out["loaded_" + k] = getattr(loaded, k)
        return out
    return Case(f"ply-{nr}+{nb}", run, ["scg_ply_pack", "scg_ply_pack_color_view", "scg_ply_unpack"],
                excused={"scg_ply_unpack": {"upload": "the file's bytes, uploaded by the wrapper with .to(device) from pinned memory"}},
                fields={"scg_ply_unpack": (["model.ray.zval", "model.ray.features_rest"] if nr else []) + (["model.bg.xyz"] if nb else [])})


# ---- the bicubic resize (img/scg_resample.h) ------------------------------------------------------------------------------------------

def _resize(win, hin, wout, hout, c, shift=1):
    def run(home):
        import test_gpu_resize as T
        from scgaussian_amd import images
        src, want, fl = T._case("random", win, hin, c, (wout, hout))
        flat = torch.from_numpy(np.array(src)).reshape(-1)
        buf = torch.zeros(flat.numel() + shift, dtype=torch.uint8, device=DEV)
        buf[shift:] = flat.to(DEV)
        view = buf[shift:].view(src.shape)                        # the device source at an odd address
        channels = 1 if src.ndim == 2 else src.shape[2]
        plan = images.plan_of((win, hin), (wout, hout), channels)
        dev = view.device
        plan._device_tables[dev] = home(torch.from_numpy(np.array(plan.tables)).to(dev))      # the plan's cached upload, in a body
        try:
            out_float = torch.full((channels, hout, wout), -1.0, dtype=torch.float32, device=DEV)
            got = images.resize_u8(view, (wout, hout), out_float=out_float)
            torch.cuda.synchronize()
        finally:
            plan._device_tables.pop(dev, None)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(out_float.cpu().numpy().view(np.uint32), fl.view(np.uint32))
        return dict(out=got, out_float=out_float)
    return Case(f"resize-{win}x{hin}-to-{wout}x{hout}-{'L' if c == 0 else 'RGB'}", run, ["scg_resample_u8"])


# ---- virtual-view warp and smoothness (vw/scg_virtualwarp.h) -----------------------------------------------------------------------------

def _warp(H, W, nv):
    def run(home):
        import test_gpu_virtualwarp as T
        import virtualwarp_refs as VR
        from scgaussian_amd import virtual
        scene = VR.make_scene(H, W, nv, T.SEEDS[(H, W, nv)])
        t = home(VR.tensors(scene, device=DEV))
        warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
        warp.set_pose(scene["vir_c2w"])
        img, depth = t["virtual_img"].requires_grad_(True), t["virtual_depth"].requires_grad_(True)
        loss = warp.loss(img, depth, t["vir_mask"])
        loss.backward(_scalar(0.75))
        return dict(loss=loss, loss_map=warp.loss_map, winner=warp.winner, in_bounds=warp.in_bounds, d_img=img.grad, d_depth=depth.grad)
    return Case(f"vw_warp-{H}x{W}x{nv}", run, ["scg_vw_warp_forward", "scg_vw_warp_backward"])


def _smooth(H, W, form):
    def run(home):
        from scgaussian_amd import virtual
        rng = np.random.default_rng(H * 1000 + W)
        depth = (3 + rng.uniform(-1, 1, (H, W))).astype(np.float32)
        guide = {"none": None, "hw": rng.uniform(0, 1, (H, W)), "chw": rng.uniform(0, 1, (3, H, W))}[form]
        d = home(torch.from_numpy(depth).to(DEV).requires_grad_(True))
        g = None if guide is None else home(torch.from_numpy(guide.astype(np.float32)).to(DEV))
        loss = virtual.smooth_loss(d, g)
        grad = torch.autograd.grad(loss, d, _scalar(0.5))[0]
        return dict(loss=loss, grad=grad)
    return Case(f"vw_smooth-{H}x{W}-{form}", run, ["scg_vw_smooth_forward", "scg_vw_smooth_backward"])


# ---- LPIPS (lp/scg_lpips.h) ------------------------------------------------------------------------------------------------------------

def _lp_layer(cin, cout, h, w, pool):
    def run(home):
        import test_gpu_lpips as T
        from scgaussian_amd import lpips
        x, wt, b = T.layer_inputs(cin, cout, 1, h, w, seed=h + w + cin)
        # channels-last in memory, so that the wrapper's own re-layout is the identity and the kernel reads these very buffers
        xd, wd = (home(t.permute(0, 2, 3, 1).contiguous().to(DEV)).permute(0, 3, 1, 2) for t in (x, wt))
        out = lpips.conv3x3(xd, wd, home(b.to(DEV)), relu=True, pool=pool, zscore=cin == 3)
        return dict(out=out)
    return Case(f"lp_conv3x3-{cin}-{cout}-{h}x{w}{'-pooled' if pool else ''}", run, ["scg_lp_conv3x3"])


def _lp_metric(H, W):
    def run(home):
        import lpips_refs as LR
        import test_gpu_lpips as T
        from scgaussian_amd import lpips
        lp = home(lpips.Lpips.from_state_dicts(*LR.state_dicts(T.WEIGHTS), device=DEV))      # (the weights are re-laid with torch.cat)
        x, y = LR.make_images(H, W, seed=H + W)
        xd, yd = home(torch.from_numpy(x).to(DEV)), home(torch.from_numpy(y).to(DEV))
        value = lp(xd, yd)
        terms = lp.terms.clone()
        fx, fy = lp.features(xd, yd)
        head = lp.head(H, W)
        return dict(value=value, terms=terms, head=head, head_terms=lp.terms, fx=list(fx), fy=list(fy))
    return Case(f"lp_forward-{H}x{W}", run, ["scg_lp_forward", "scg_lp_head"], not_passed={"scg_lp_head": {"features"}})


# ---- PNG (png/scg_png.h) ----------------------------------------------------------------------------------------------------------------

def _png(gray):
    def run(home):
        import test_gpu_png as T
        from scgaussian_amd import png
        rng = np.random.default_rng(2)
        wrap = np.array([[0, 255, 0, 255, 1], [255, 0, 255, 0, 254], [0, 0, 255, 255, 128]], dtype=np.uint8)
        # the smallest images of the module's own test, none with a row of a multiple of 16 bytes, one and three channels
        arrays = [np.zeros((1, 1), np.uint8), np.full((1, 1, 3), 255, np.uint8), T.noise(rng, 1, 37), T.noise(rng, 37, 1),
                  T.noise(rng, 1, 9, 3), T.noise(rng, 9, 1, 3), wrap, np.stack([wrap, wrap[::-1], 255 - wrap], axis=2),
                  T.smooth(31, 45, 3), T.smooth(31, 45, 1), T.noise(rng, 5, 7, 1)]
        imgs = [home(T._t(a)) for a in arrays]
        plan = home(png.PngPlan([t.shape for t in imgs], DEV, png.UP, gray, own_inputs=False))      # (its chunk table is uploaded)
        files = plan.encode(imgs).files()
        T.check_files(files, arrays, png.UP, gray, "guarded")
        return dict(files=files)                                  # (the buffer's gaps between the streams belong to nobody)
    return Case(f"png-{'rgb' if gray else 'gray'}", run, ["scg_png_encode"],
                excused={"scg_png_encode": {"args.images_host": "host copy of the image table"}})


# ---- the rasterizer: the staged geometry stage, the one-call entries, the model path (scg_raster.h) ------------------------------

PINNED = "pinned host words (the camera's long-list counts, the forward's partial sums of num_rendered)"
FRAME_HOST = {"frame.long_lists_out": PINNED, "frame.num_rendered_out": PINNED}
FRAME_ENTRIES = ("scg_geometry_forward", "scg_binning", "scg_blend_forward", "scg_blend_backward", "scg_geometry_backward", "scg_forward",
                 "scg_backward", "scg_forward_model", "scg_backward_model")
RASTER_EXCUSED = {e: dict(FRAME_HOST) for e in FRAME_ENTRIES}
for _e in ("scg_forward", "scg_forward_model"):
    RASTER_EXCUSED[_e]["partial_sums"] = PINNED
RASTER_EXCUSED["scg_wait_num_rendered"] = {"partial_sums_host": PINNED}
W_RASTER, H_RASTER = 75, 40                                       # no multiple of the tile either way


def _atomics(a, b, what):
    """Gradients the blend backward sums with float atomics (and what the geometry backward makes of them): the suite's own bar,
    its finiteness check included — fill A is a NaN, and a float read past an input must not be able to hide behind one."""
    import parity_utils as pu
    pu.assert_close(a, b, what)


def _atomics_where_written(a, b, what):
    """The same bar for the `tail_` results, whose outputs start as NaN and keep it wherever SCG_BACKWARD_SH_TAIL_ZERO tells the
    kernel not to write: the unwritten elements must be the SAME elements in both runs, and only they are left out."""
    import parity_utils as pu
    assert torch.equal(a.isnan(), b.isnan()), what + ": the elements left unwritten (NaN) differ"
    pu.assert_close(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0), what)


def _raster_comparator(name):
    """The comparison of a raster or model-path result by its name (None: bit for bit)."""
    if name.startswith("tail_"):
        return _atomics_where_written
    return _atomics if name.startswith(("staged_", "added_", "grad_")) else None


def _absent_gradients(mode):
    col, cov = mode.split("_")
    out = {"dL_dcolors_precomp"} if col == "sh" else {"dL_dshs"}
    return out | ({"dL_dcov3D_precomp"} if cov == "sr" else {"dL_dscales", "dL_drotations"})


def _raster(mode, deg, P):
    def run(home):
        import parity_utils as pu
        import test_gpu_geometry_edges as TG
        from scgaussian_amd import _lib
        from scgaussian_amd import rasterizer as R
        from scgaussian_amd import synthetic as syn
        W, H = W_RASTER, H_RASTER
        sc = syn.make_scene(P, W, H, seed=P, log_scale_mean=-3.0)
        cam = syn.orbit_camera(W, H, 8.0, 4.0, 7.0)
        st = home(pu.hip_settings(cam, deg, (0.2, 0.4, 0.6)))
        leaves = {k: home(v.detach().to(DEV).contiguous().requires_grad_(True)) for k, v in pu.run_oracle_inputs(sc, cam, deg, 1.0, mode).items()}
        ups = [home(g.to(DEV)) for g in syn.make_upstream_grads(W, H, seed=P + 50)]
        ins = {k: v.detach() for k, v in leaves.items() if k != "means2D"}
        out = {}
        # the staged path: scg_geometry_forward, then the backward stages writing, adding (ACCUMULATE) and with the SH tails left
        fs = R.forward_stages(st, ins["means3D"], ins["opacities"], shs=ins.get("shs"), colors_precomp=ins.get("colors_precomp"),
                              scales=ins.get("scales"), rotations=ins.get("rotations"), cov3D_precomp=ins.get("cov3D_precomp"),
                              prepare_backward=True)
        out.update(color=fs["color"], depth=fs["depth"], alpha=fs["alpha"], radii=fs["radii"], splats=fs["splats"], rects=fs["rects"],
                   depth_keys=fs["depth_keys"], clamped=fs["clamped"])
        g1 = R.backward_stages(st, fs["inputs"], fs, *ups, want_dsplats=True)
        records = g1.pop("dsplats")
        for k, v in g1.items():
            if isinstance(v, torch.Tensor):
                out["staged_" + k] = v.clone()
        g2 = R.backward_stages(st, fs["inputs"], fs, *ups, into=g1)
        for k, v in g2.items():
            if isinstance(v, torch.Tensor):
                out["added_" + k] = v.clone()
        tail = TG._call_backward(st, ins, mode, fs["radii"], fs["clamped"], records, flags=_lib.BACKWARD_SH_TAIL_ZERO)
        for k, v in tail.items():
            out["tail_" + k] = v
        # the one-call path (the staged forward above established the shape's capacity)
        rast = R.GaussianRasterizer(st)
        kw = {k: v for k, v in leaves.items() if k not in ("means3D", "means2D", "opacities")}
        for _ in range(2):                                        # (the second forward has the first one's per-tile costs as its hint)
            c, radii, d, a = rast(means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacities"], **kw)
        torch.autograd.backward([c, d, a], ups)
        out.update(one_color=c, one_depth=d, one_alpha=a, one_radii=radii)
        for k, v in leaves.items():
            out["grad_" + k] = v.grad
        return out
    absent = _absent_gradients(mode)
    return Case(f"raster-{mode}-d{deg}-P{P}", run,
                ["scg_geometry_forward", "scg_geometry_backward", "scg_forward", "scg_backward"], excused=RASTER_EXCUSED,
                not_passed={"scg_geometry_backward": absent, "scg_backward": absent, "scg_binning": {"keys_sorted"}},
                fields={"scg_forward": ["frame.tile_cost_out"], "scg_backward": ["frame.bwd_cost_out"]}, close=_raster_comparator)


def _model_path(nr, nb, deg):
    def run(home):
        from scgaussian_amd import model_path as mp
        from scgaussian_amd import render as rmod
        from scgaussian_amd import synthetic as syn
        W, H, P = W_RASTER, H_RASTER, nr + nb
        sc = syn.make_scene(P, W, H, seed=2 + P, log_scale_mean=-3.0)
        model = syn.make_raw_model(sc, ray_fraction=nr / P, seed=5)
        md = home(model.to(DEV))
        md.requires_grad_()
        md.active_sh_degree = deg
        assert (md.zval.shape[0], md.bg_xyz.shape[0]) == (nr, nb)
        act = mp.activate(**mp.tensors_of(md))
        cam = home(syn.orbit_camera(W, H, -4.0, 2.0, 7.0).to(DEV))
        bg = torch.tensor((0.1, 0.2, 0.3), device=DEV)
        ups = [home(g.to(DEV)) for g in syn.make_upstream_grads(W, H, seed=5)]
        assert rmod.model_fast_path_available(md, rmod.PipelineParams())
        for _ in range(2):
            res = rmod.render(cam, md, rmod.PipelineParams(), bg)
        torch.autograd.backward([res["render"], res["rendered_depth"], res["rendered_alpha"]], ups)
        out = dict(render=res["render"], depth=res["rendered_depth"], alpha=res["rendered_alpha"], radii=res["radii"], act=list(act),
                   grad_means2D=res["viewspace_points"].grad)
        for n in ("zval", "features_dc", "features_rest", "opacity", "scaling", "rotation", "bg_xyz", "bg_features_dc",
                  "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation"):
            if getattr(md, n).shape[0]:
                out["grad_" + n] = getattr(md, n).grad
        return out
    fields = (["grads.ray." + f for f in ("zval", "features_dc", "features_rest", "opacity", "scaling", "rotation")] if nr else []) + \
        (["grads.bg." + f for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")] if nb else [])
    return Case(f"model_path-{nr}+{nb}-d{deg}", run, ["scg_model_activate", "scg_forward_model", "scg_backward_model"],
                excused=RASTER_EXCUSED, close=_raster_comparator,
                fields={"scg_backward_model": fields + ["frame.bwd_cost_out"], "scg_forward_model": ["frame.tile_cost_out"]})


CASES = (
    [_image_loss(s, lam) for s, lam in (((3, 1, 1), 0.2), ((3, 5, 7), 0.2), ((3, 33, 65), 1.0))]
    + [_image_loss_pair(s) for s in ((3, 1, 1), (3, 33, 65))]
    + [_match_loss(M) for M in (1, 37)]
    + [_knn(n) for n in (1, 4, 65, 257)]
    + [_sort(n) for n in (1, 255, 257)] + [_scan(n) for n in (1, 255, 257)]
    + [_dtu(n) for n in (1, 63)]
    + [_eval_view(False), _eval_view(True)]
    + [_geocheck(3, 1, 1)]
    + [_viz(H, W) for H, W in ((1, 1), (1, 3), (5, 7), (17, 65), (1, 1025))]
    + [_densify(nr, nb) for nr, nb in ((1, 0), (33, 32), (129, 128))] + [_densify_stats(P) for P in (1, 257)]
    + [_seed(N) for N in (1, 65, 257)]
    + [_mono("two_views"), _mono("edge_scene")]
    + [_matchpoint(N) for N in (1, 5, MP_T + 1)]
    + [_ply(nr, nb) for nr, nb in ((1, 0), (0, 1), (PLY_T + 1, 3))]
    + [_resize(*a, c) for a in ((1, 7, 3, 5), (5, 7, 3, 5), (17, 7, 6, 5), (7, 5, 20, 9), (1, 1, 3, 2)) for c in (0, 3)]
    + [_warp(3, 3, 3), _warp(VW_T + 1, VW_T - 1, 3), _warp(7, 9, 1)] + [_smooth(2, 2, "chw"), _smooth(1, 1, "none")]
    + [_lp_layer(3, 64, 1, LP_TM + 1, False), _lp_layer(64, 128, 3, 2 * LP_TM + 3, True)] + [_lp_metric(16, 16), _lp_metric(17, 16)]
    + [_png(True), _png(False)]
    + [_raster("sh_sr", 0, 1), _raster("sh_sr", 3, 63), _raster("col_cov", 3, 65), _raster("sh_sr", 0, 257), _raster("sh_sr", 3, 257),
       _raster("col_cov", 3, 257)]
    + [_model_path(1, 0, 0), _model_path(0, 1, 3), _model_path(61, 59, 3), _model_path(64, 65, 0)]
)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_guard_bands(case):
    check_case(case)


def test_the_helper_sees_device_memory():
    """tests/test_guarded_alloc_cpu.py holds the helper's teeth on CPU tensors; the same three statements once on the device: a write
    one element past a body and one before it are found, a tensor made by an unpatched name lies in no body."""
    for fill in (FILL_A, FILL_B):
        with guarded(fill) as reg:
            t = torch.zeros(5, dtype=torch.float32, device=DEV)
            u = torch.empty((3, 2), dtype=torch.uint8, device=DEV)
            idx = torch.arange(4, dtype=torch.int32, device=DEV)
            assert all(reg.covers(x.data_ptr()) for x in (t, u, idx)) and not reg.covers(torch.randn(4, device=DEV).data_ptr())
            assert reg.check() == []
            torch.as_strided(t, (1,), (1,), t.storage_offset() + 5).fill_(7.5)
            torch.as_strided(idx, (1,), (1,), idx.storage_offset() - 1).fill_(9)
            torch.cuda.synchronize()
        hits = {h.shape: h for h in reg.check()}
        assert set(hits) == {(5,), (4,)}
        assert (hits[(5,)].side, hits[(5,)].offset, hits[(5,)].found) == ("back", 0, 7.5)
        assert (hits[(4,)].side, hits[(4,)].offset, hits[(4,)].found) == ("front", -4, 9)


# ---- coverage: every compute entry of every header is reached by a case above, or named here with its reason --------------------------

# families whose own edge tests already place guard values around their buffers
ALREADY_GUARDED = {
    "scg_binning": "tests/test_gpu_binning_edges.py", "scg_blend_forward": "tests/test_gpu_blend_edges.py",
    "scg_blend_backward": "tests/test_gpu_blend_edges.py", "scg_init_stage_run": "tests/test_gpu_init_stage_edges.py",
    "scg_adam_step": "tests/test_gpu_optim_edges.py",
}
# pure size, layout, version and error queries (no device memory is touched), and the event helpers (host handles only)
QUERIES = {
    "scg_last_error", "scg_abi_version", "scg_struct_bytes", "scg_ranges_words", "scg_geometry_scratch_bytes", "scg_binning_scratch_bytes",
    "scg_binning_accepts_bound", "scg_sort_scratch_bytes", "scg_scan_scratch_bytes", "scg_workspace_layout", "scg_forward_sorts_in_blend",
    "scg_wait_num_rendered", "scg_event_create", "scg_event_destroy", "scg_event_elapsed_ms", "scg_adam_workspace_bytes",
    "scg_densify_workspace_bytes", "scg_seed_workspace_bytes", "scg_init_stage_partials_bytes", "scg_knn3_scratch_bytes",
    "scg_image_loss_dmaps_bytes", "scg_image_loss_scratch_bytes", "scg_dtu_bg_mask_segment_rows", "scg_masked_mean_scratch_bytes",
    "scg_eval_metrics_scratch_bytes", "scg_eval_depth_range_scratch_bytes", "scg_eval_view_tile", "scg_geocheck_workspace_bytes",
    "scg_geocheck_tile", "scg_viz_select_block", "scg_viz_select_scratch_bytes", "scg_mono_struct_bytes", "scg_mono_block",
    "scg_img_last_error", "scg_img_abi_version", "scg_resample_pitch", "scg_resample_mid_bytes", "scg_io_last_error", "scg_io_abi_version",
    "scg_ply_layout_bytes", "scg_ply_layout", "scg_lp_last_error", "scg_lp_abi_version", "scg_lp_scratch_bytes", "scg_lp_feature_floats",
    "scg_mp_last_error", "scg_mp_abi_version", "scg_mp_struct_bytes", "scg_mp_layout", "scg_mp_workspace_bytes", "scg_png_last_error",
    "scg_png_abi_version", "scg_png_struct_bytes", "scg_png_layout", "scg_vw_last_error", "scg_vw_abi_version", "scg_vw_warp_scratch_bytes",
    "scg_vw_smooth_scratch_bytes",
}


def test_every_compute_entry_of_every_header_has_a_case():
    """Runs behind the cases (SEEN is what their traced calls reached; a case that has not run in this process is run here).  The
    table's own claims are held first: the three sets tile the headers' functions, and every entry a case names exists."""
    declared = set(FUNCTIONS)
    assert QUERIES <= declared and set(ALREADY_GUARDED) <= declared and not QUERIES & set(ALREADY_GUARDED)
    compute = declared - QUERIES - set(ALREADY_GUARDED)
    claimed = {e for c in CASES for e in c.entries}
    assert claimed <= declared
    assert compute - claimed == set(), f"compute entries without a case: {sorted(compute - claimed)}"
    for case in CASES:                                            # (selected alone, or with -k: the cases that have not run yet run here)
        if case.id not in TIMES:
            check_case(case)
    assert compute - SEEN == set(), f"compute entries no case reached: {sorted(compute - SEEN)}"
    print(f"GUARD {len(CASES)} cases, {sum(TIMES.values()):.2f} s in the cases; slowest: {sorted(TIMES.items(), key=lambda kv: -kv[1])[:5]}")
