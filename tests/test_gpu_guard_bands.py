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
  4. the public results of the three runs are bit-identical — except where float atomics sum them, held to the module's own bar;
  5. under A and under B the body of every torch.empty / torch.empty_like request of the binding (outputs, scratch, workspaces,
     arenas, the pinned staging buffers) starts from the fill instead of what the allocator last held there (guarded_alloc:
     "Poison"), the third run stays unpoisoned as the baseline, and condition 4 is the detector: a scratch float read before
     anything wrote it is a NaN under A and 0.0115 under B, an output element nobody wrote has different bits under A and B, a
     counter assumed to start at 0 starts at 0xFFFFFFFF and at 0x3C3C3C3C (1 and 2 in an int16/32/64 tensor).

A difference between A and B means bytes outside an input reached a result: a finding of the same rank as a touched band.  No case
plants an out-of-range value; every call is one the wrappers make today at sizes the suite already uses — the second half of the
table at the paths that write least (everything culled, one tile, nothing kept, nothing selected, nothing in bounds, all NaN, the
smallest image), where a "nothing to do" return would leave an output as it was.  Where the module's own test knows the exact
answer of such a path (zeros, the background, NaN), the case asserts it inside run() as well.

Index reads, audited by reading the kernels before the first guarded run (the wider-integer fills are the valid indices 1 and 2 all
the same; none needed a fix): the segment tables of seed.hip and matchpoint.hip are copied to LDS with s < nseg and searched inside
[0, nseg - 1], a segment's view is used only when 0 <= view < V, and a winner index only when 0 <= wi < N; mono.hip reads its group,
segment and view tables at blockIdx (the launch dimensions are their lengths) and checks segment, partner and view before use;
pngpack.hip checks a chunk's image index against the image count; jpegpack.hip takes a segment record only when its image lies in
[0, images) and its row in [0, the image's segments) and names this very workgroup (segment_of), clamps every pixel index to the
image, and reads a header template at the offset the entry point checked against the templates' size; resample.hip clamps the column index to wout - 1 and a bound to
[0, win - 1]; the geocheck pair table is written by scg_geocheck_setup itself; scg_sort_pairs and scg_inclusive_scan_u32 take
their integers as values, never as addresses; scg_densify_stats compares radii with 0; jpegunpack.hip: a batched workgroup finds
its image by a search of the prefix table inside [0, n - 1] and goes on only when first[image] <= its index < first[image] + the
image's own group count; a record of the device table is followed only when frame_from accepts its frame and the header block, the
segment, the pixels and each of the ten workspace regions lie, offset and size, inside upload_bytes, out_bytes and workspace_bytes as
the call was passed them (view_of_image), every index into the header block is masked (look[peek >> 8], vals[.. & 255], table id & 1,
quant id & 3), a stream read stops at the segment's bytes and a coefficient is stored only for a block below the frame's count;
camgrad.hip reads radii, inputs and records at min(i, P - 1), compares radii with 0 and splits i at model.ray.count, which the entry
point held to P.

Scratch words, audited by reading before the first poisoned run — per family: the words a kernel reads or updates atomically, and
who wrote or cleared them earlier in the same call (K: the kernel itself or an earlier launch of the call; M: a hipMemsetAsync on
the call's stream; W: the wrapper).  No dependence on an unwritten word was found and no product code changed; that "none" rests
on this reading and on the cases below, not on a proof.
  binning_tiles.hip   class_counts[4] and len_hist[1024]: K, cleared by workgroup 0 of tile_hist_kernel or geometry_hist_kernel
                      (one launch before the first atomic on them); table[B][Tn]: K, every one of the B workgroups stores its whole
                      row, also one that owns no Gaussian; tile_total / tile_part / tile_class / tile_start: K, table_colscan_kernel
                      and the eight publishing workgroups write every tile; mid_tiles / big_tiles / segments: read up to the counts
                      in class_counts only; seg_count is class_counts[2]; the scatter's cursors are LDS; spill: written by the
                      list's own workgroup before it is read; ranges / order / order_q: K, every slot (padding slots n_tiles)
  binning.hip         counts[256][blocks] and totals[256]: K (sort_hist_kernel stores every word, sort_rowscan_kernel the totals);
                      the scan's block sums: K; ranges on the global-sort and the empty path: M, the two order tables K
  geometry.hip        next_chunk and the block sums of geometry_hist_kernel are LDS, cleared behind a barrier; block_sums /
                      partial_sums: K, one store per 256-Gaussian block (armed by the host on the one-call path); splats, rects,
                      depth_keys, clamped, radii: K, flush_stage writes culled Gaussians too
  blend.hip           cost_out: K (publish_tile_starts stores 0 per tile before the forward's atomicMax; the hint buffers come from
                      torch.zeros); bcost_out: K, stored per (tile, quadrant), 0 on an empty walk; dsplats: K (the forward blend's
                      zero_fill, every record, before any tile test) or M (not prezeroed); final_T / n_contrib: K, every pixel
                      inside the image; the record planes of the fused forward are LDS
  the rasterizer's workspace (scg_forward / scg_backward, _launch_forward's `ws`, forward_stages' two _Arena.buf): the planes
                      above carved from one allocation; the padding between them and point_list beyond the counted total are
                      never read; the gradient arena (_grads.py): K, every row of every segment (zeros for a culled Gaussian;
                      the SH tail when the arena carries no promise yet), its <= 3 padding floats per segment belong to nobody
  matchloss.hip       loss, grad_depth: W (one torch.zeros for both)
  optim.hip           ws: W, zero by contract (torch.zeros once, the kernel returns every word to 0 or to the watermark)
  initstage.hip       partials: K, rows [0, n_steps) x every workgroup, flushed before the kernel ends; loss_state / grad: K
  dtumask.hip         count: M; the partial sums of the masked mean and of the metrics: K, one word per workgroup, all read
  evalview.hip        sk[2]: M; the range's partial (min, max): K; mask_u8 is not written without a mask and not returned
  depthviz.hip        all kSelWords words (three histograms, max of ~key, NaN count): M
  loss.hip, knn.hip   partials / partial (splits, n, 3): K, every word the fold reads
  geocheck.hip        workspace, votes, masks, filtered: W (torch.zeros); the kernel skips a record whose source is no view
  compact.h, densify.hip, seed.hip: counts: K, one store per workgroup, carry_scan reads groups words; head: K (scan kernel);
                      fate / keep: K for i < P; winner: K, seed_classify_kernel / mp_clear_kernel store -1 in every pixel before
                      the atomicMax launches; the new statistics rows: K, zeroed whole by the scatter
  matchpoint.hip      partial (min, max): K per resolve workgroup; the gaps behind the four regions of the buffer: K (mp_clear)
  virtualwarp.hip     y, dyd: K, every (view, channel, pixel) whether in bounds or not; coef, loss_map, winner: K per pixel;
                      partial: K per tile; the smoothness partials (2, groups): K
  lpips.hip           taps, the two activation buffers, partial [tap][pb]: K, each layer writes what the next one reads
  resample.hip        mid: K, whole dwords of every row; the bytes of a row's pitch behind its last dword are never read
  pngpack.hip         lengths, info, base, ioff, table: K for every chunk and image; the image table is uploaded by _bind before
                      the first launch; the gaps between the streams in `out` belong to nobody and reach no file
  jpegpack.hip        base[s]: K, the count kernel's one store per segment (0 for a record that names nothing), base[segments] and
                      the exclusive offsets by the scan kernel; ioff, table: K, the scan kernel writes every image's row and the
                      last one before the encode kernel reads flag, offset and base[s], base[s + 1]; the window, the code tables and
                      the DC history are LDS, cleared behind a barrier; the image table is uploaded by _bind, the segment and header
                      tables by the plan; a flagged file's capacity and the gaps between the files in `out` belong to nobody
  jpegunpack.hip      the status words and the change counters (all images' in the batch): M, one clear; the coefficient buffers: M,
                      the second clear; entry, exit: K, sync launch 0 stores every subsequence's before a later launch or the
                      count reads them; bnd: K, every workgroup stores its word in every launch, launch k + 1 reads what launch k
                      stored and launch 0 reads none; cnt, dcs: K, the count stores every subsequence's before the scan and the
                      write read them; the planes: K, the idct stores every block of the padded planes before the colour kernel
                      reads inside them; out: K, every byte of H W components; the alignment gaps between regions and between
                      the batch's images belong to nobody
  camgrad.hip         partials: K, every workgroup stores its 27 words (a wave without a visible Gaussian adds zeros) before the
                      one finishing workgroup reads [0, blocks) x 27; out35: K, all 35 words, the twelve dead ones as 0, also at
                      P = 0 and with everything culled
  plypack.hip, mono.hip: no scratch; every byte of the buffer / arena region an entry owns is written by it; the tables the mono
                      kernels index are uploaded from the host copy
"""
import contextlib
import functools
import glob
import math
import os
import re
import time

import numpy as np
import pytest
import torch

import abi_text
from guarded_alloc import FILL_A, FILL_B, guarded, same_bits as _same_bits, traced
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
    from scgaussian_amd import _lib, _lib_camgrad, _lib_img, _lib_io, _lib_jpegdec, _lib_jpg, _lib_lp, _lib_mp, _lib_png, _lib_vw
    return (_lib, _lib_io, _lib_img, _lib_mp, _lib_vw, _lib_lp, _lib_png, _lib_jpg, _lib_jpegdec, _lib_camgrad)


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
    from scgaussian_amd import _counts, _grads, jpeg_decode, model_path, rasterizer
    rasterizer._FRAME_CACHE.clear()
    rasterizer._CAM_HINTS.clear()
    _grads._ARENA_POOLS.clear()
    _grads._LAYOUTS.clear()
    model_path._ACCEPTS.clear()
    _counts._SPEC_STATE.clear()
    jpeg_decode._PLANS.clear()                                    # (images.py keeps no decode plan of its own: it calls jpeg_decode)
    jpeg_decode._BATCH_BUFFERS.clear()


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


def _image_loss_pair(shape, same=False):
    def run(home):
        import test_image_loss as T
        from scgaussian_amd import losses
        x, y = T._content("hdr", shape, seed=sum(shape) + 1)
        if same:
            y = x.clone()                                         # identical images: no pixel has anything to add to the L1 sum
        xd, yd = home(x.to(DEV).requires_grad_(True)), home(y.to(DEV))
        l1, ss = losses.l1_and_ssim(xd, yd)
        torch.autograd.backward([l1, ss], [_scalar(0.8), _scalar(-0.2)])
        if same:
            assert float(l1.detach()) == 0.0 and bool(torch.isfinite(xd.grad).all()) and math.isfinite(float(ss.detach()))
        return dict(l1=l1, ssim=ss, grad=xd.grad)
    return Case(f"image_loss_pair-{'x'.join(map(str, shape))}{'-identical' if same else ''}", run,
                ["scg_image_loss_forward", "scg_image_loss_backward"],
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


def _match_loss_outside(M):
    """Every match projects outside the second view (the scene of test_match_loss_with_no_counting_match_is_exactly_zero): no
    match counts, nothing is added to the loss word or to the gradient image."""
    def run(home):
        import test_match_loss as T
        from scgaussian_amd.match_loss import match_loss_from_depth
        cam0, cams = T._cams(T.MW, T.MH)
        depth = T._depth(T.MW, T.MH, 5)
        w2c1 = cams[0].world_view_transform.t().contiguous().clone()
        w2c1[0, 3] += 1000.0
        p = T._pair_from_uv0(cam0, cams[0], depth, T._random_uv0(T.MW, T.MH, M, 3), 4, w2c1=w2c1)
        p["mask0"], p["mask1"] = torch.ones(M), torch.ones(M)
        d = home(depth.clone().to(DEV)[None].requires_grad_(True))
        out = match_loss_from_depth(d, [home(T._to_cuda(p))], float(T.MW), float(T.MH))
        out.backward(_scalar(0.3))
        assert float(out.detach()) == 0.0 and not bool(d.grad.any())
        return dict(loss=out, grad=d.grad)
    return Case(f"match_loss-M{M}-all-outside", run, ["scg_match_loss_pair"])


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


def _dtu_empty(n):
    """A ground truth without a dark pixel: the mask is empty, the count 0, the alpha term the mean of nothing (NaN, gradient 0);
    and metrics over an empty selection (NaN)."""
    def run(home):
        import test_gpu_dtu as T
        from scgaussian_amd import dtu
        H, W = T.SIZES[n]
        g = torch.Generator().manual_seed(n)
        bright = torch.rand(3, H, W, generator=g) * 0.4 + 0.5
        view = dtu.DtuView(home(bright.to(DEV)))
        alpha = home(torch.rand(1, H, W, generator=g).to(DEV).requires_grad_(True))
        term = dtu.alpha_term(alpha, view)
        term.backward(_scalar(0.7))
        img, gt = (home((torch.rand(3, H, W, generator=g) * 1.8 - 0.4).to(DEV)) for _ in range(2))
        l1, psnr, mse = dtu.eval_metrics_all(img, gt, home(torch.zeros(H, W).to(DEV)))
        assert int(view.count) == 0 and not bool(view.mask.any()) and torch.equal(view.gt.cpu(), bright)
        assert math.isnan(float(term.detach())) and not bool(alpha.grad.any())
        assert math.isnan(float(l1)) and math.isnan(float(psnr)) and bool(torch.isnan(mse).all())
        return dict(mask=view.mask, gt=view.gt, count=view.count, term=term, grad=alpha.grad, l1=l1, psnr=psnr, mse=mse)
    return Case(f"dtu-{n}-empty", run, ["scg_dtu_bg_mask", "scg_masked_mean_forward", "scg_masked_mean_backward", "scg_eval_metrics"])


# ---- the evaluation view (scg_eval.h) -------------------------------------------------------------------------------------------------

def _eval_view(masked, nan_depth=False):
    def run(home):
        import eval_refs as ER
        import test_gpu_eval as T
        from scgaussian_amd import evaluate
        H, W = T.TH + 1, T.TW + 1
        render, gt, depth = ER.images(H, W, seed=100 * H + W, outside=True)
        if nan_depth:
            depth = torch.full_like(depth, float("nan"))          # no finite depth: the range is (NaN, NaN)
        mask = home(T._mask(H, W, 7 * H + W).to(DEV)) if masked else None
        out = evaluate.evaluate_view(home(render.to(DEV)), home(gt.to(DEV)), home(depth.to(DEV)), mask)
        return {k: v for k, v in out.items() if v is not None}
    return Case(f"eval_view-{'masked' if masked else 'plain'}{'-nan-depth' if nan_depth else ''}", run,
                ["scg_eval_depth_range", "scg_eval_view", "scg_image_loss_forward"],
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


def _geocheck_singular(n, H, W):
    """View 2 has a focal length of 0 (no inverse): it finds no source and is nobody's source — no votes
    (test_singular_intrinsic_gives_no_votes_and_no_fault)."""
    def run(home):
        import test_gpu_geocheck as T
        from scgaussian_amd import geo_check as gc
        intrs, exts, depths = T._close_scene(n, H, W, seed=100 + 7 * H + W)
        intrs = intrs.copy()
        intrs[2] = np.array([[0.0, 0, W / 2], [0, 0.0, H / 2], [0, 0, 1]])
        chk = gc.GeoCheck(n, H, W, num_src=2, device=torch.device(DEV, 0))
        chk.setup(home(torch.from_numpy(intrs).to(DEV)), home(torch.from_numpy(exts).to(DEV)))
        fd, fm = chk.run(home(torch.from_numpy(depths).to(DEV)), view_thresh=0)
        assert not bool(chk.votes[2].any()) and not bool(fm[2].any())
        return dict(filtered=fd, masks=fm, votes=chk.votes, pairs=chk.pairs)
    return Case(f"geocheck-{n}x{H}x{W}-singular", run, ["scg_geocheck_setup", "scg_geocheck"])


# ---- depth colour maps (scg_viz.h) ---------------------------------------------------------------------------------------------------

def _viz(H, W, all_nan=False):
    def run(home):
        from scgaussian_amd import video
        rng = np.random.default_rng(H * 2000 + W)
        plane = rng.random((H, W), dtype=np.float32) * 5 + 1
        if all_nan:
            plane[:] = np.nan                                     # every key is the NaN key: one bin, H * W NaNs counted
        x = home(torch.from_numpy(plane).to(DEV))
        render = home(torch.from_numpy(rng.random((3, H, W), dtype=np.float32) * 1.4 - 0.2).to(DEV))
        viz = home(video.DepthColorizer(H, W))                    # (its table is uploaded with .to(device): moved too)
        r = viz.depth_range(x)
        outs = {k: torch.empty((H, W) if k == "depth_u8" else (H, W, 3), dtype=torch.uint8, device=DEV)
                for k in ("depth_color", "depth_color_bgr", "depth_u8", "render_u8", "frame_bgr")}
        viz.frame(x, r, render=render, **outs)
        stats = viz.stats(x).clone()
        if all_nan:                                               # matplotlib's "bad" colour everywhere, numpy's NaN percentiles
            assert int(viz._nan) == H * W and bool(torch.isnan(stats[:2]).all())
            assert not bool(outs["depth_color"].any()) and not bool(outs["depth_color_bgr"].any())
        return dict(outs, range=r, stats=stats, nan=viz._nan)
    return Case(f"viz-{H}x{W}{'-all-nan' if all_nan else ''}", run, ["scg_eval_depth_range", "scg_viz_select", "scg_viz_frame"])


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


def _densify(nr, nb, mode="mixed"):
    """mode (test_gpu_densify.make_inputs): "none" — no gradient is hot, nothing is cloned, split or pruned, the background set is
    copied as it is; "prune_all" — every background row is pruned and none is created: no new row at all."""
    def run(home):
        import test_gpu_densify as T
        from scgaussian_amd import densify
        t, states, noise = T.make_inputs(nr, nb, 100 + nr, mode)
        m = home(T.build(t, states, DEV, torch.optim.Adam))       # the model, both optimizers and their moments, moved together
        before = m.bg_xyz.detach().clone()
        densify.install(m)
        m.densify_and_prune(T.MAX_GRAD, T.MIN_OPACITY, T.EXTENT, 20, noise=home(noise.to(DEV)))
        mid = {k: v.detach().clone() for k, v in _model_results(m).items()}
        if mode == "none":
            assert torch.equal(m.bg_xyz.detach(), before)
        if mode == "prune_all":
            assert m.bg_xyz.shape == (0, 3) and m.xyz_gradient_accum.shape == (nr, 1)
        if mode != "mixed":                                       # the statistics of every row that is left start from zero
            assert not bool(m.xyz_gradient_accum.any()) and not bool(m.denom.any()) and not bool(m.max_radii2D.any())
        m.reset_opacity()
        return dict(after_densify=mid, after_reset=_model_results(m))
    left = nb and mode != "prune_all"
    bg = ["args.out." + f for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")] if left else []
    return Case(f"densify-{nr}+{nb}" + ("" if mode == "mixed" else "-" + mode), run,
                ["scg_densify_classify", "scg_densify_scatter", "scg_reset_opacity"],
                fields={"scg_densify_scatter": bg + ["args.accum", "args.denom", "args.max_radii2D", "args.ray_scaling"]},
                not_passed={"scg_reset_opacity": set() if left else {"bg_opacity", "bg_exp_avg", "bg_exp_avg_sq"}})


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


def _seed_edges():
    """Two calls of the scenes of tests/test_gpu_seed.py: no match under the threshold (nothing is scattered, no kNN launch, every
    pixel of the sparse depth is 0) and a view no segment belongs to (its planes are zero whatever the other views receive)."""
    def run(home):
        import test_gpu_seed as T
        from scgaussian_amd import seed
        out = {}
        for name, V, seg_view, loss in (("none_kept", 3, [0, 1, 2, 0], 0.5), ("untouched_view", 4, [0, 3, 0, 1], 0.01)):
            arena = T.random_arena(32, [8, 8, 8, 8], seg_view, V, H=12, W=16, seed_=5)
            arena["min_loss"] = torch.full((32,), loss).to(DEV)
            arena = {k: home(v) if torch.is_tensor(v) else v for k, v in arena.items()}
            got = seed.seed_arrays(home(T.inputs_of(arena)), arena["min_loss"])
            if name == "none_kept":
                assert got["n"] == 0 and not bool(got["masks"].any()) and not bool(got["sparse_depths"].any())
            else:
                assert got["n"] == 32 and not bool(got["masks"][2].any()) and not bool(got["sparse_depths"][2].any())
                assert bool(got["masks"].any())
            out[name] = got
        return out
    outs = ["args." + f for f in ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "opacity_out",
                                  "max_radii2D")]
    return Case("seed-none-kept-and-untouched-view", run,
                ["scg_seed_classify", "scg_seed_scatter", "scg_knn3_mean_dist2_ws", "scg_seed_finish"],
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

def _matchpoint(N, empty_view=False):
    def run(home):
        import matchpoint_refs as MR
        import test_gpu_matchpoint as T
        from scgaussian_amd import matchpoint
        if empty_view:                                            # three views, the middle one without a match: a plane of zeros
            arena = MR.random_arena([N, N + 2], [0, 2], [(5, 6), (3, 7), (4, 5)], seed=N)
        else:
            arena = MR.random_arena([N], [0], [(5, 6)], seed=N)
        inputs = home(T.inputs_of(arena, home(T.tensors(arena))))  # (the two device tables are uploaded by the constructor: moved too)
        snap = matchpoint.pack(inputs)
        return dict(buffer=snap.buffer)
    return Case(f"matchpoint-{N}{'-empty-view' if empty_view else ''}", run, ["scg_mp_pack"],
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
            for name in sorted(os.listdir(folder)):               # the files themselves: point_cloud(.ply, _bg.ply, _color.ply)
                if name.endswith(".ply"):
                    with open(os.path.join(folder, name), "rb") as fh:
                        out["file_" + name] = fh.read()
            assert ("file_point_cloud_bg.ply" in out) == bool(nb)
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

def _resize(win, hin, wout, hout, c, shift=1, float_from="full"):
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
            if float_from == "full":
                out_float = torch.full((channels, hout, wout), -1.0, dtype=torch.float32, device=DEV)
            else:                                                 # undefined content, as the binding's own callers hand it over
                out_float = torch.empty((channels, hout, wout), dtype=torch.float32, device=DEV)
            got = images.resize_u8(view, (wout, hout), out_float=out_float)
            torch.cuda.synchronize()
        finally:
            plan._device_tables.pop(dev, None)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(out_float.cpu().numpy().view(np.uint32), fl.view(np.uint32))
        return dict(out=got, out_float=out_float)
    # (the width unchanged: no horizontal pass, no intermediate image)
    return Case(f"resize-{win}x{hin}-to-{wout}x{hout}-{'L' if c == 0 else 'RGB'}{'' if float_from == 'full' else '-' + float_from}", run,
                ["scg_resample_u8"], not_passed={"scg_resample_u8": {"mid"} if win == wout else set()})


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


def _warp_blind(kind):
    """The two scenes of test_a_frame_no_view_sees_is_exactly_zero: every source view 100 units aside (nothing in bounds), and a
    mask that is false everywhere: no winner, a loss of exactly 0 and gradients of exactly 0 in every pixel."""
    def run(home):
        import virtualwarp_refs as VR
        from scgaussian_amd import virtual
        sc = VR.make_scene(VW_T + 1, VW_T + 3, 3, 5)
        if kind == "unseen":
            sc["w2cs"][:, 0, 3] += 100.0
        else:
            sc["vir_mask"][:] = False
        t = home(VR.tensors(sc, device=DEV))
        warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
        warp.set_pose(sc["vir_c2w"])
        img, depth = t["virtual_img"].requires_grad_(True), t["virtual_depth"].requires_grad_(True)
        loss = warp.loss(img, depth, t["vir_mask"])
        loss.backward(_scalar(0.75))
        assert float(loss.detach()) == 0.0 and bool((warp.winner == -1).all()) and not bool(warp.loss_map.any())
        assert not bool(img.grad.any()) and not bool(depth.grad.any()) and bool(warp.in_bounds.any()) == (kind != "unseen")
        return dict(loss=loss, loss_map=warp.loss_map, winner=warp.winner, in_bounds=warp.in_bounds, d_img=img.grad, d_depth=depth.grad)
    return Case(f"vw_warp-{kind}", run, ["scg_vw_warp_forward", "scg_vw_warp_backward"])


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


def _lp_metric(H, W, equal=False):
    def run(home):
        import lpips_refs as LR
        import test_gpu_lpips as T
        from scgaussian_amd import lpips
        lp = home(lpips.Lpips.from_state_dicts(*LR.state_dicts(T.WEIGHTS), device=DEV))      # (the weights are re-laid with torch.cat)
        x, y = LR.make_images(H, W, seed=H + W)
        if equal:
            y = x.copy()                                          # every difference of normalised features is exactly 0
        xd, yd = home(torch.from_numpy(x).to(DEV)), home(torch.from_numpy(y).to(DEV))
        value = lp(xd, yd)
        terms = lp.terms.clone()
        if equal:
            assert float(value) == 0.0 and not bool(terms.any())
        fx, fy = lp.features(xd, yd)
        head = lp.head(H, W)
        return dict(value=value, terms=terms, head=head, head_terms=lp.terms, fx=list(fx), fy=list(fy))
    return Case(f"lp_forward-{H}x{W}{'-equal' if equal else ''}", run, ["scg_lp_forward", "scg_lp_head"],
                not_passed={"scg_lp_head": {"features"}})


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


def _png_edges(gray):
    """1 x 1 alone (one chunk of two bytes), an all-zero image (the longest runs: a handful of tokens per chunk), and an odd-sized
    image of more than one chunk whose last chunk is short; the files are the restatement's byte for byte."""
    def run(home):
        import test_gpu_png as T
        from scgaussian_amd import png
        rng = np.random.default_rng(3)
        arrays = [np.full((1, 1), 7, np.uint8), np.zeros((37, 45, 3), np.uint8), np.zeros((1, 1, 3), np.uint8),
                  T.noise(rng, 131, 251), T.smooth(87, 127, 3)]      # 131 x 252 = 33 012 and 87 x 382 = 33 234 bytes: 32 768 + a rest
        out = {}
        for name, part in (("one_pixel", arrays[:1]), ("batch", arrays[1:])):
            imgs = [home(T._t(a)) for a in part]
            plan = home(png.PngPlan([t.shape for t in imgs], DEV, png.UP, gray, own_inputs=False))
            files = plan.encode(imgs).files()
            T.check_files(files, part, png.UP, gray, "poisoned " + name)
            out[name] = files
        return out
    return Case(f"png-edges-{'rgb' if gray else 'gray'}", run, ["scg_png_encode"],
                excused={"scg_png_encode": {"args.images_host": "host copy of the image table"}})


# ---- JPEG (jpg/scg_jpeg.h) -------------------------------------------------------------------------------------------------------------

JPEG_EXCUSED = {"scg_jpeg_encode": {"args.images_host": "host copy of the image table"}}


def _jpeg_batch(T):
    """The smallest images of the module's own tests: one block, sizes that are no multiple of the MCU either way, one component."""
    rng = np.random.default_rng(6)
    return [T.noise(rng, 1, 1), T.noise(rng, 7, 9), T.noise(rng, 9, 9), T.smooth(24, 8), T.noise(rng, 5, 7, 1), T.smooth(31, 45),
            T.noise(rng, 8, 24)]


def _jpeg(sub):
    def run(home):
        import test_gpu_jpeg as T
        from scgaussian_amd import jpeg
        arrays = _jpeg_batch(T)
        imgs = [home(T._t(a)) for a in arrays]
        plan = jpeg.JpegPlan([t.shape for t in imgs], DEV, 90, sub, own_inputs=False)
        packed = plan.encode(imgs)
        files = packed.files()                                    # (1 x 1 and its like do not fit header + 3 H W: encoded once more)
        T.check_files(files, arrays, 90, sub, what="guarded")
        return dict(files=files, table=packed.table_host.copy())  # (the buffer's gaps between the files belong to nobody)
    return Case(f"jpeg-{sub}", run, ["scg_jpeg_encode"], excused=JPEG_EXCUSED)


def _jpeg_shortfall():
    """The same batch with exactly the bytes every file needs, the third one byte short: without the retry no byte of that file is
    written and the others are the restatement's; with it all seven are."""
    def run(home):
        import jpeg_refs
        import test_gpu_jpeg as T
        from scgaussian_amd import jpeg
        arrays = _jpeg_batch(T)
        imgs = [home(T._t(a)) for a in arrays]
        caps = [len(jpeg_refs.encode(a, 90, "4:2:0")) for a in arrays]
        caps[2] -= 1
        plan = jpeg.JpegPlan([t.shape for t in imgs], DEV, 90, "4:2:0", capacities=caps, own_inputs=False)
        packed = plan.encode(imgs).to_host(retry=False)
        files = packed.files()
        assert files[2] == b"" and packed.overflowed == [2] and not packed.retried
        T.check_files(files[:2] + files[3:], arrays[:2] + arrays[3:], what="one byte short")
        again = plan.encode(imgs)
        whole = again.files()
        assert again.retried and again.overflowed == []
        T.check_files(whole, arrays, what="encoded again")
        return dict(files=files, table=packed.table_host.copy(), whole=whole, whole_table=again.table_host.copy())
    return Case("jpeg-shortfall", run, ["scg_jpeg_encode"], excused=JPEG_EXCUSED)


def _jpeg_edges():
    """1 x 1 alone; a 4:2:0 row of 43 MCUs x 6 = 258 blocks (two rounds of 256) whose file lies inside one 16 KiB window; two noise
    rows at quality 100, 4:2:0 and 4:4:4, whose single segment crosses the window and flushes a full one.  The sizes are the
    restatement's, on the CPU.  The default capacity (header + 3 H W) holds the two 4:2:0 rows; 1 x 1 and the 4:4:4 row (noise at
    quality 100 takes more than three bytes per pixel: 34 315 > 629 + 24 576) are flagged and encoded once more."""
    def run(home):
        import test_gpu_jpeg as T
        from scgaussian_amd import jpeg
        rng = np.random.default_rng(6)
        wide100, wide90, flat100 = T.noise(rng, 16, 1024), T.noise(rng, 16, 688), T.noise(rng, 8, 1024)
        out = {}
        for name, a, quality, sub, size in (("one_pixel", T.noise(rng, 1, 1), 90, "4:2:0", None), ("two_rounds", wide90, 90, "4:2:0", 10543),
                                            ("window_420", wide100, 100, "4:2:0", 32992), ("window_444", flat100, 100, "4:4:4", 34315)):
            img = home(T._t(a))
            packed = jpeg.JpegPlan([img.shape], DEV, quality, sub, own_inputs=False).encode([img])
            files = packed.files()
            T.check_files(files, [a], quality, sub, what="poisoned " + name)
            assert size is None or len(files[0]) == size, (name, len(files[0]))
            assert packed.retried == (name in ("one_pixel", "window_444")), name
            out[name] = files
        return out
    return Case("jpeg-edges", run, ["scg_jpeg_encode"], excused=JPEG_EXCUSED)


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


BG_RASTER = (0.2, 0.4, 0.6)
ONE_TILE = (1, 1)                                                 # the tile the "one_tile" scenes put every Gaussian into


def _sparse_scene(kind, P, seed):
    """(scene, camera) of the table's frame.  "random": the frame the older cases render.  "culled": the same Gaussians behind a
    camera that looks the other way — every radius is 0, no tile has a list, the image is the background.  "one_tile": small
    Gaussians whose centres lie in the middle of tile ONE_TILE — every other tile's list is empty."""
    from scgaussian_amd import synthetic as syn
    W, H = W_RASTER, H_RASTER
    if kind == "random":
        return syn.make_scene(P, W, H, seed=seed, log_scale_mean=-3.0), syn.orbit_camera(W, H, 8.0, 4.0, 7.0)
    if kind == "culled":
        return syn.make_scene(P, W, H, seed=seed, log_scale_mean=-3.0), syn.orbit_camera(W, H, 180.0, 0.0, 7.0, target=(0.0, 0.0, -7.0))
    assert kind == "one_tile"
    sc = syn.make_scene(P, W, H, seed=seed, log_scale_mean=-5.5)
    g = torch.Generator().manual_seed(seed + 1)
    px, py = (16.0 * t + 5.0 + 6.0 * torch.rand(P, generator=g) for t in ONE_TILE)      # 5 .. 11 pixels inside the tile
    tany = math.tan(math.radians(50.0) / 2)
    z = sc.means3D[:, 2]
    sc.means3D[:, 0] = ((2 * px + 1) / W - 1) * (tany * W / H) * z
    sc.means3D[:, 1] = ((2 * py + 1) / H - 1) * tany * z
    return sc, syn.default_camera(W, H)


def _assert_sparse(kind, color, depth, alpha, radii):
    """What the module's own tests know of these frames: the background wherever no tile has a list."""
    bg = torch.tensor(BG_RASTER, device=color.device)[:, None, None]
    if kind == "culled":
        assert not bool(radii.any()) and torch.equal(color, bg.expand_as(color)) and not bool(depth.any()) and not bool(alpha.any())
    if kind == "one_tile":
        outside = torch.ones(color.shape[-2:], dtype=torch.bool, device=color.device)
        outside[16 * ONE_TILE[1]:16 * ONE_TILE[1] + 16, 16 * ONE_TILE[0]:16 * ONE_TILE[0] + 16] = False
        assert bool((radii > 0).all()) and bool((radii <= 5).all()), radii.max()
        assert torch.equal(color[:, outside], bg[:, 0].expand(3, int(outside.sum()))) and not bool(alpha[:, outside].any())
        assert bool(alpha[:, ~outside].any())


def _raster(mode, deg, P, scene="random"):
    def run(home):
        import parity_utils as pu
        import test_gpu_geometry_edges as TG
        from scgaussian_amd import _lib
        from scgaussian_amd import rasterizer as R
        from scgaussian_amd import synthetic as syn
        W, H = W_RASTER, H_RASTER
        sc, cam = _sparse_scene(scene, P, P)
        st = home(pu.hip_settings(cam, deg, BG_RASTER))
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
        _assert_sparse(scene, fs["color"], fs["depth"], fs["alpha"], fs["radii"])
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
        _assert_sparse(scene, c, d, a, radii)
        out.update(one_color=c, one_depth=d, one_alpha=a, one_radii=radii)
        for k, v in leaves.items():
            out["grad_" + k] = v.grad
            if scene == "culled":                                 # every gradient row is written, and a culled Gaussian's is zero
                assert v.grad is not None and not bool(v.grad.any()), k
                assert not bool(out["staged_" + k].any()) and not bool(out["added_" + k].any()), k
        if scene == "culled":
            # no Gaussian at all, where the binding takes it (the staged forward; the operator itself refuses empty inputs):
            # nothing is launched on the Gaussians, the image is the background
            none = {k: v[:0] for k, v in ins.items()}
            f0 = R.forward_stages(st, none["means3D"], none["opacities"], shs=none.get("shs"), colors_precomp=none.get("colors_precomp"),
                                  scales=none.get("scales"), rotations=none.get("rotations"), cov3D_precomp=none.get("cov3D_precomp"))
            _assert_sparse(scene, f0["color"], f0["depth"], f0["alpha"], f0["radii"])
            out.update(none_color=f0["color"], none_depth=f0["depth"], none_alpha=f0["alpha"])
        return out
    absent = _absent_gradients(mode)
    return Case(f"raster-{mode}-d{deg}-P{P}" + ("" if scene == "random" else "-" + scene), run,
                ["scg_geometry_forward", "scg_geometry_backward", "scg_forward", "scg_backward"], excused=RASTER_EXCUSED,
                not_passed={"scg_geometry_backward": absent, "scg_backward": absent, "scg_binning": {"keys_sorted"}},
                fields={"scg_forward": ["frame.tile_cost_out"], "scg_backward": ["frame.bwd_cost_out"]}, close=_raster_comparator)


def _model_path(nr, nb, deg, scene="random"):
    def run(home):
        from scgaussian_amd import model_path as mp
        from scgaussian_amd import render as rmod
        from scgaussian_amd import synthetic as syn
        W, H, P = W_RASTER, H_RASTER, nr + nb
        sc, cam_cpu = _sparse_scene(scene, P, 2 + P)
        model = syn.make_raw_model(sc, ray_fraction=nr / P, seed=5)
        md = home(model.to(DEV))
        md.requires_grad_()
        md.active_sh_degree = deg
        assert (md.zval.shape[0], md.bg_xyz.shape[0]) == (nr, nb)
        act = mp.activate(**mp.tensors_of(md))
        cam = home((syn.orbit_camera(W, H, -4.0, 2.0, 7.0) if scene == "random" else cam_cpu).to(DEV))
        bg = torch.tensor((0.1, 0.2, 0.3) if scene == "random" else BG_RASTER, device=DEV)
        ups = [home(g.to(DEV)) for g in syn.make_upstream_grads(W, H, seed=5)]
        assert rmod.model_fast_path_available(md, rmod.PipelineParams())
        for _ in range(2):
            res = rmod.render(cam, md, rmod.PipelineParams(), bg)
        torch.autograd.backward([res["render"], res["rendered_depth"], res["rendered_alpha"]], ups)
        _assert_sparse(scene, res["render"], res["rendered_depth"], res["rendered_alpha"], res["radii"])
        out = dict(render=res["render"], depth=res["rendered_depth"], alpha=res["rendered_alpha"], radii=res["radii"], act=list(act),
                   grad_means2D=res["viewspace_points"].grad)
        for n in ("zval", "features_dc", "features_rest", "opacity", "scaling", "rotation", "bg_xyz", "bg_features_dc",
                  "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation"):
            if getattr(md, n).shape[0]:
                out["grad_" + n] = getattr(md, n).grad
                if scene == "culled":                             # every row of every raw-parameter gradient is written: zeros
                    assert getattr(md, n).grad is not None and not bool(getattr(md, n).grad.any()), n
        return out
    fields = (["grads.ray." + f for f in ("zval", "features_dc", "features_rest", "opacity", "scaling", "rotation")] if nr else []) + \
        (["grads.bg." + f for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")] if nb else [])
    return Case(f"model_path-{nr}+{nb}-d{deg}" + ("" if scene == "random" else "-" + scene), run,
                ["scg_model_activate", "scg_forward_model", "scg_backward_model"],
                excused=RASTER_EXCUSED, close=_raster_comparator,
                fields={"scg_backward_model": fields + ["frame.bwd_cost_out"], "scg_forward_model": ["frame.tile_cost_out"]})


# ---- the JPEG decoder (jpegdec/scg_jpegdec.h) --------------------------------------------------------------------------------------

UPLOADED = "the file's bytes and its header block, uploaded by the wrapper with .to(device) from pinned memory"
JPEGDEC_LONG = (88, 96)                                           # noise at quality 100, 4:4:4: a segment of two workgroups


@functools.lru_cache(maxsize=None)
def _jpegdec_small():
    """[(name, file, the restatement's pixels)]: the smallest sizes of test_gpu_jpegdec.SIZES at each sampling, one component, a
    restart interval, and a segment of one subsequence and a byte.  Computed once."""
    import jpegdec_refs as R
    files = [(f"{H}x{W}-{sampling}", R.pillow_file(R.image(H, W, 3, "noise"), 90, sampling))
             for (H, W) in ((1, 1), (7, 9), (17, 33), (3, 50)) for sampling in R.SAMPLINGS]
    files.append(("7x9-one-component", R.pillow_file(R.image(7, 9, 1, "noise"), 90)))
    files.append(("17x33-restart", R.pillow_file(R.image(17, 33, 3, "noise"), 90, "4:2:0", restart_blocks=1)))
    files.append(("subsequence+1", R.segment_of_length(R.SUBSEQ + 1)))
    assert b"\xff\xd0" in files[-2][1] and R.segment_bytes(files[-1][1]) == R.SUBSEQ + 1
    return [(name, data, R.decode(data)) for name, data in files]


@functools.lru_cache(maxsize=None)
def _jpegdec_long():
    import jpegdec_refs as R
    data = R.pillow_file(R.image(*JPEGDEC_LONG, 3, "noise"), 100, "4:4:4")
    assert R.segment_bytes(data) >= R.SUBSEQ * R.THREADS + 1 and b"\xff\xd0" not in data      # more than one workgroup, no marker
    return "long", data, R.decode(data)


def _jpegdec_single():
    def run(home):
        from scgaussian_amd import jpeg_decode
        out = {}
        for name, data, want in _jpegdec_small() + [_jpegdec_long()]:
            got = jpeg_decode.decode(data, DEV)
            last = dict(jpeg_decode.LAST)
            assert last["route"] == "device" and last["status"] == 0, (name, last)      # (never through Pillow on the host)
            assert np.array_equal(got.cpu().numpy(), want), name
            if name == "long":                                    # hand-over words across workgroups, more than one sync launch
                assert last["launched"] > 1 and 1 < last["rounds"] <= last["launched"], last
            out[name] = got
        return out
    return Case("jpegdec-single", run, ["scg_jpegdec_decode"],
                excused={"scg_jpegdec_decode": {"header_dev": UPLOADED, "segment_dev": UPLOADED}})


def _jpegdec_batch():
    """The small files in one list: several share a header block (one quality, the standard tables), two have one shape, and a
    progressive file in the middle is refused by parse() and decoded alone afterwards; then the list again in two chunks."""
    def run(home):
        import jpegdec_refs as R
        from scgaussian_amd import jpeg_decode
        small = _jpegdec_small()
        twin = R.pillow_file(R.image(7, 9, 3, "noise", seed=1), 90, "4:4:4")
        refused = R.pillow_file(R.image(24, 40, 3, "noise"), 90, "4:2:0", progressive=True)
        assert jpeg_decode.parse(refused) is None and small[3][0] == "7x9-4:4:4"
        files = [d for _n, d, _w in small[:4]] + [twin] + [d for _n, d, _w in small[4:8]] + [refused] + [d for _n, d, _w in small[8:]]
        want = [w for _n, _d, w in small[:4]] + [R.pillow_pixels(twin)] + [w for _n, _d, w in small[4:8]] + [R.pillow_pixels(refused)] + \
            [w for _n, _d, w in small[8:]]
        at = files.index(refused)
        accepted = [f for f in files if f is not refused]
        whole = jpeg_decode.BatchStage([jpeg_decode.parse(f) for f in accepted], accepted).plan().workspace_bytes
        out = {}
        for tag, kw, chunks in (("one", {}, 1), ("two", dict(max_workspace_bytes=whole - 1), 2)):
            got = jpeg_decode.decode_batch(files, DEV, **kw)
            last = dict(jpeg_decode.LAST)
            assert last["chunks"] == chunks and last["headers"] < chunks * len(accepted), last
            assert [r for i, r in enumerate(last["route"]) if i != at] == ["device"] * len(accepted), last
            assert last["route"][at] == "single host" and last["status"][at] is None, last
            for i, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g.cpu().numpy(), w), (tag, i)
            if chunks == 1:                                       # images of one shape side by side: 189 bytes padded to 192
                assert got[3].untyped_storage().data_ptr() == got[4].untyped_storage().data_ptr()
                assert got[4].storage_offset() - got[3].storage_offset() == 192
            out[tag] = list(got)
        return out
    return Case("jpegdec-batch", run, ["scg_jpegdec_decode_batch"],
                excused={"scg_jpegdec_decode_batch": {"table_dev": UPLOADED, "upload_dev": UPLOADED}})


# ---- the camera gradients (camgrad/scg_camgrad.h) ----------------------------------------------------------------------------------

def _camgrad_alone(n, mode, want_campos=True, culled=False):
    """The kernel alone on planted records (test_gpu_camgrad._sized, _kernel), held to the fp64 restatement at the module's own
    bar; culled: every radius 0, where the 35 outputs must still be written — exact zeros."""
    def run(home):
        import test_gpu_camgrad as T
        inputs, cam, records, radii = T._sized(n, 3, mode)
        if culled:
            radii = torch.zeros_like(radii)
        got = T._kernel(inputs, cam, 3, 1.0, records, radii, want_campos=want_campos, home=home)
        if culled:
            assert not got.any() and not np.signbit(got).any()
        else:
            T._held(got, inputs, cam, 3, 1.0, records, radii, ("guarded", n, mode, want_campos), want_campos=want_campos)
        return dict(out35=torch.from_numpy(got))
    return Case(f"camgrad-alone-{n}-{mode}" + ("" if want_campos else "-no-campos") + ("-culled" if culled else ""), run,
                ["scg_camgrad_backward"])


def _camgrad_model(nr, nb):
    def run(home):
        import geometry_refs as G
        import test_gpu_camgrad as T
        from scgaussian_amd import model_path as mp
        n = nr + nb
        model, md = T._raw_model(ray_fraction=nr / n, n=n)
        md = home(md)
        t = mp.tensors_of(md)
        assert mp.supported(t) and (md.zval.shape[0], md.bg_xyz.shape[0]) == (nr, nb)
        inputs = T._activated_inputs(model, md)
        cam = T._cam(1)
        radii = G.oracle_preprocess({k: v for k, v in inputs.items()}, cam, 3, 1.0)["radii"]
        records = G.make_records(n, 43)
        got = T._kernel(inputs, cam, 3, 1.0, records, radii, seven=mp._ModelArgs(t), home=home)
        T._held(got, inputs, cam, 3, 1.0, records, radii, ("guarded", "model", nr, nb))
        return dict(out35=torch.from_numpy(got))
    return Case(f"camgrad-model-{nr}+{nb}", run, ["scg_camgrad_backward_model"])


def _camgrad_routed(P):
    """GaussianRasterizer with viewmatrix, projmatrix and campos requiring grad, two steps of one camera: the staged path, whose
    gradient records are a tensor, then the one-call path, whose records are a raw pointer into the forward's workspace."""
    def run(home):
        import parity_utils as pu
        from scgaussian_amd import rasterizer as R
        from scgaussian_amd import synthetic as syn
        W, H = W_RASTER, H_RASTER
        sc, cam = _sparse_scene("random", P, P)
        st = pu.hip_settings(cam, 3, BG_RASTER)
        st = home(st._replace(**{k: getattr(st, k).detach().clone().requires_grad_(True) for k in ("viewmatrix", "projmatrix", "campos")}))
        camera = {k: getattr(st, k) for k in ("viewmatrix", "projmatrix", "campos")}
        leaves = {k: home(v.detach().to(DEV).contiguous().requires_grad_(True)) for k, v in pu.run_oracle_inputs(sc, cam, 3, 1.0, "sh_sr").items()}
        ups = [home(g.to(DEV)) for g in syn.make_upstream_grads(W, H, seed=P + 50)]
        kw = {k: v for k, v in leaves.items() if k not in ("means3D", "means2D", "opacities")}
        out = {}
        for step in ("staged", "one_call"):
            for t in (*leaves.values(), *camera.values()):
                t.grad = None
            c, radii, d, a = R.GaussianRasterizer(st)(means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacities"], **kw)
            torch.autograd.backward([c, d, a], ups)
            out.update({f"{step}_color": c, f"{step}_depth": d, f"{step}_alpha": a, f"{step}_radii": radii})
            for k, v in (*leaves.items(), *camera.items()):
                assert v.grad is not None, (step, k)
                out[f"grad_{step}_{k}"] = v.grad.clone()
        return out
    absent = _absent_gradients("sh_sr")
    return Case(f"camgrad-routed-P{P}", run, ["scg_camgrad_backward", "scg_forward", "scg_backward"], excused=RASTER_EXCUSED,
                not_passed={"scg_geometry_backward": absent, "scg_backward": absent, "scg_binning": {"keys_sorted"}},
                fields={"scg_forward": ["frame.tile_cost_out"], "scg_backward": ["frame.bwd_cost_out"]},
                close=lambda name: _atomics if name.startswith("grad_") else None)


CASES = (
    [_image_loss(s, lam) for s, lam in (((3, 1, 1), 0.2), ((3, 5, 7), 0.2), ((3, 33, 65), 1.0))]
    + [_image_loss_pair(s) for s in ((3, 1, 1), (3, 33, 65))] + [_image_loss_pair((3, 33, 65), same=True)]
    + [_match_loss(M) for M in (1, 37)] + [_match_loss_outside(37)]
    + [_knn(n) for n in (1, 4, 65, 257)]
    + [_sort(n) for n in (1, 255, 257)] + [_scan(n) for n in (1, 255, 257)]
    + [_dtu(n) for n in (1, 63)] + [_dtu_empty(63)]
    + [_eval_view(False), _eval_view(True), _eval_view(True, nan_depth=True)]
    + [_geocheck(3, 1, 1), _geocheck_singular(3, 5, 7)]
    + [_viz(H, W) for H, W in ((1, 1), (1, 3), (5, 7), (17, 65), (1, 1025))] + [_viz(5, 7, all_nan=True)]
    + [_densify(nr, nb) for nr, nb in ((1, 0), (33, 32), (129, 128))] + [_densify(33, 32, "none"), _densify(33, 32, "prune_all")]
    + [_densify_stats(P) for P in (1, 257)]
    + [_seed(N) for N in (1, 65, 257)] + [_seed_edges()]
    + [_mono("two_views"), _mono("edge_scene")]      # (edge_scene holds the segments without a valid match: pair (2, 4), pair (1, 3) but one)
    + [_matchpoint(N) for N in (1, 5, MP_T + 1)] + [_matchpoint(5, empty_view=True)]
    + [_ply(nr, nb) for nr, nb in ((1, 0), (0, 1), (PLY_T + 1, 3), (33, 0))]
    + [_resize(*a, c) for a in ((1, 7, 3, 5), (5, 7, 3, 5), (17, 7, 6, 5), (7, 5, 20, 9), (1, 1, 3, 2)) for c in (0, 3)]
    + [_resize(*a, c, float_from="empty") for a in ((7, 5, 7, 5), (2, 2, 5, 5)) for c in (0, 3)]      # the copy, an upscale
    + [_warp(3, 3, 3), _warp(VW_T + 1, VW_T - 1, 3), _warp(7, 9, 1)] + [_warp_blind("unseen"), _warp_blind("masked")]
    + [_smooth(2, 2, "chw"), _smooth(1, 1, "none"), _smooth(1, 9, "chw")]
    + [_lp_layer(3, 64, 1, LP_TM + 1, False), _lp_layer(64, 128, 3, 2 * LP_TM + 3, True)] + [_lp_metric(16, 16), _lp_metric(17, 16)]
    + [_lp_metric(16, 16, equal=True)]
    + [_png(True), _png(False)] + [_png_edges(True), _png_edges(False)]
    + [_jpeg("4:2:0"), _jpeg("4:4:4"), _jpeg_shortfall(), _jpeg_edges()]
    + [_raster("sh_sr", 0, 1), _raster("sh_sr", 3, 63), _raster("col_cov", 3, 65), _raster("sh_sr", 0, 257), _raster("sh_sr", 3, 257),
       _raster("col_cov", 3, 257)]
    + [_raster("sh_sr", 3, 65, "culled"), _raster("col_cov", 3, 65, "culled"), _raster("sh_sr", 3, 65, "one_tile"),
       _raster("col_cov", 3, 65, "one_tile")]
    + [_model_path(1, 0, 0), _model_path(0, 1, 3), _model_path(61, 59, 3), _model_path(64, 65, 0)]
    + [_model_path(33, 32, 3, "culled"), _model_path(33, 32, 3, "one_tile")]
    + [_jpegdec_single(), _jpegdec_batch()]
    + [_camgrad_alone(n, mode) for n in (1, 257, 2 * 256 + 1) for mode in ("sh_sr", "col_cov")]
    + [_camgrad_alone(257, "sh_sr", want_campos=False), _camgrad_alone(257, "sh_sr", culled=True)]
    + [_camgrad_model(61, 59), _camgrad_routed(65)]
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
            assert bool(u.eq(0xFF if fill == FILL_A else 0x3C).all())      # the body of a device `empty` reads back as the fill
            torch.as_strided(t, (1,), (1,), t.storage_offset() + 5).fill_(7.5)
            torch.as_strided(idx, (1,), (1,), idx.storage_offset() - 1).fill_(9)
            torch.cuda.synchronize()
        hits = {h.shape: h for h in reg.check()}
        assert set(hits) == {(5,), (4,)}
        assert (hits[(5,)].side, hits[(5,)].offset, hits[(5,)].found) == ("back", 0, 7.5)
        assert (hits[(4,)].side, hits[(4,)].offset, hits[(4,)].found) == ("front", -4, 9)


# ---- coverage: every compute entry of every header is reached by a case above, or named here with its reason --------------------------

# families whose own edge tests already place guard values around their buffers — and start what their runners hand over as
# scratch from both fills of the helper (test_what_the_scratch_held_... / _workspace_held_... in test_gpu_binning_edges.py,
# test_what_the_buffers_held_... in test_gpu_blend_edges.py, test_4f_... in test_gpu_init_stage_edges.py).  scg_adam_step has no
# scratch but `ws`, which is zero by contract (zeroed once, kept) and stays zero in its runner
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
    "scg_png_abi_version", "scg_png_struct_bytes", "scg_png_layout", "scg_jpg_last_error", "scg_jpg_abi_version", "scg_jpg_struct_bytes",
    "scg_jpeg_layout", "scg_vw_last_error", "scg_vw_abi_version", "scg_vw_warp_scratch_bytes",
    "scg_vw_smooth_scratch_bytes", "scg_jpegdec_last_error", "scg_jpegdec_abi_version", "scg_jpegdec_sizes", "scg_jpegdec_batch_plan",
    "scg_camgrad_last_error", "scg_camgrad_abi_version", "scg_camgrad_sizes",
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
