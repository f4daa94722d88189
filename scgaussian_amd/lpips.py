"""The LPIPS metric of metrics.py:90, `lpips(render, gt, net_type='vgg')`, host side (libscg_lp.so, include/lp/scg_lpips.h).

    lpipsPyTorch/modules/networks.py:36-63,88-96   z-score, vgg16().features[0:30], taps 4, 9, 16, 23, 30   -> Lpips.__call__
    lpipsPyTorch/modules/utils.py:6-8              x / (sqrt(sum_c x^2) + 1e-10)                             -> the head
    lpipsPyTorch/modules/lpips.py:30-36            (fx - fy)^2, the 1x1 linear layers, the mean, the sum     -> the head
    lpipsPyTorch/modules/utils.py:22-30            lin{l}.model.1.weight -> {l}.1.weight                     -> map_lin_keys

The reference builds the network with torchvision and fetches both weight sets from the net.  Here the caller brings them: a VGG16
state dict (torchvision's keys) and the LPIPS linear layers' (either spelling), as dicts or as files.  An `Lpips` is an `lpips_fn`
of evaluate.EvalSet / evaluate.render_set: it takes the two images on the device and returns a (1,1,1,1) device tensor without a
host read.  CPU tensors go through `lpips_torch`, the same rule in plain torch."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, _lib_lp
from ._lib_lp import check

VGG_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # the Conv2d modules of vgg16().features
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
POOL_BEFORE = (2, 4, 7, 10)                 # the convolutions (0-based) whose input is the 2x2 max pool of the previous output
TAP_AFTER = (1, 3, 6, 9, 12)                # ... whose ReLU is a tap: modules 4, 9, 16, 23, 30 counted from 1
TAP_CHANNELS = (64, 128, 256, 512, 512)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10


def map_vgg_keys(sd):
    """[(weight (cout,cin,3,3), bias (cout,))] * 13 from a state dict with torchvision's `features.<i>.weight / .bias` keys, or the
    same without the prefix; other keys are ignored.  A missing key or a wrong shape raises ValueError naming the key."""
    out = []
    for i, (cin, cout) in zip(VGG_CONV_INDICES, CHANNELS):
        pair = []
        for part, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = next((k for k in (f"features.{i}.{part}", f"{i}.{part}") if k in sd), None)
            if key is None:
                raise ValueError(f"VGG16 weights: key features.{i}.{part} is missing")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"VGG16 weights: {key} has shape {tuple(sd[key].shape)}, not {shape}")
            pair.append(sd[key])
        out.append(tuple(pair))
    return out


def map_lin_keys(sd):
    """The five (1,C,1,1) linear weights from the published `lin{l}.model.1.weight` keys or the reference's `{l}.1.weight`."""
    out = []
    for l, c in enumerate(TAP_CHANNELS):
        key = next((k for k in (f"lin{l}.model.1.weight", f"{l}.1.weight") if k in sd), None)
        if key is None:
            raise ValueError(f"LPIPS linear weights: key lin{l}.model.1.weight is missing")
        if tuple(sd[key].shape) != (1, c, 1, 1):
            raise ValueError(f"LPIPS linear weights: {key} has shape {tuple(sd[key].shape)}, not {(1, c, 1, 1)}")
        out.append(sd[key])
    return out


def _images(x, y):
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if y.dim() == 4 and y.shape[0] == 1:
        y = y[0]
    if x.dim() != 3 or x.shape[0] != 3 or y.shape != x.shape:
        raise ValueError("LPIPS takes two images of one shape, (3,H,W) or (1,3,H,W)")
    if x.shape[1] < _lib_lp.LP_MIN_DIM or x.shape[2] < _lib_lp.LP_MIN_DIM:
        raise ValueError(f"LPIPS needs H, W >= {_lib_lp.LP_MIN_DIM}: below it a pool has nothing to pool")
    return x, y


def vgg_taps_torch(x, convs):
    """The five normalised maps (1,C,h,w) of one image (1,3,H,W) in x's dtype: the rule in plain torch."""
    mean = torch.tensor(MEAN, dtype=torch.float32).to(x)[None, :, None, None]
    std = torch.tensor(STD, dtype=torch.float32).to(x)[None, :, None, None]
    x = (x - mean) / std
    feats = []
    for i, (w, b) in enumerate(convs):
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, w.to(x), b.to(x), padding=1))
        if i in TAP_AFTER:
            feats.append(x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + EPS))
    return feats


def lpips_torch(x, y, convs, lins):
    """The plain-torch twin: (value (1,1,1,1), terms (5,), features of x, features of y) in the images' dtype and on their device."""
    x, y = _images(x, y)
    fx, fy = vgg_taps_torch(x[None], convs), vgg_taps_torch(y[None], convs)
    res = [F.conv2d((a - b) ** 2, l.to(a)).mean((2, 3), True) for a, b, l in zip(fx, fy, lins)]
    terms = torch.cat(res, 0)
    return torch.sum(terms, 0, True), terms.reshape(-1), fx, fy


class Lpips:
    """lp = Lpips.from_state_dicts(vgg_sd, lin_sd); lp(x, y) -> (1,1,1,1) fp32 on the images' device.  The weights are re-laid once,
    here, into the one array the kernels read (the header's layout).  After a call `terms` holds the five per-tap values (device,
    fp32).  Scratch is cached per (H, W): 0.31 GB at 504 x 378, 3.1 GB at 1600 x 1200.  Not re-entrant across streams: a call
    reuses the scratch of the previous call of the same size."""

    def __init__(self, convs, lins, device="cuda"):
        self.device = torch.device(device)
        self.convs = [(w.detach().float().to(self.device), b.detach().float().to(self.device)) for w, b in convs]
        self.lins = [l.detach().float().to(self.device) for l in lins]
        self.terms = None
        self._scratch = {}
        self.params = None
        if self.device.type == "cuda":
            parts = [w.permute(0, 2, 3, 1).reshape(-1) for w, _ in self.convs] + [b for _, b in self.convs] + \
                [l.reshape(-1) for l in self.lins]
            self.params = torch.cat(parts).contiguous()
            assert self.params.numel() == _lib_lp.LP_PARAM_FLOATS

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd, device="cuda"):
        return cls(map_vgg_keys(vgg_sd), map_lin_keys(lin_sd), device=device)

    @classmethod
    def from_files(cls, vgg_path, lin_path, device="cuda"):
        return cls.from_state_dicts(torch.load(vgg_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True), device=device)

    def _buffers(self, H, W):
        if (H, W) not in self._scratch:
            lib = _lib_lp.load()
            nbytes = lib.scg_lp_scratch_bytes(H, W)
            if nbytes == 0:
                raise ValueError(f"LPIPS: {H} x {W} is out of range")
            with torch.cuda.device(self.device):
                self._scratch[(H, W)] = (torch.empty((nbytes,), dtype=torch.uint8, device=self.device), nbytes)
        return self._scratch[(H, W)]

    def _run(self, x, y, features=None):
        lib = _lib_lp.load()
        stream = _lib.stream_of(x, "Lpips")
        if y.device != x.device or x.device != self.params.device:
            raise ValueError("LPIPS: the images and the weights must be on one device")
        x, y = x.detach().float().contiguous(), y.detach().float().contiguous()
        _, H, W = x.shape
        scratch, nbytes = self._buffers(H, W)
        with torch.cuda.device(x.device):
            out = torch.empty((6,), dtype=torch.float32, device=x.device)          # the value, then the five terms
            check(lib.scg_lp_forward(H, W, x.data_ptr(), y.data_ptr(), self.params.data_ptr(), out.data_ptr(), out.data_ptr() + 4,
                                     _lib.ptr(features), scratch.data_ptr(), nbytes, stream), "scg_lp_forward")
        self.terms = out[1:]
        return out[:1].reshape(1, 1, 1, 1)

    def head(self, H, W, features=None):
        """The head alone (scg_lp_head, 2 launches) on the taps the last call at (H, W) left in the scratch: that call's value and
        `terms` again, bit for bit."""
        lib = _lib_lp.load()
        stream = _lib.stream_of(self.params, "Lpips.head")
        scratch, nbytes = self._buffers(H, W)
        with torch.cuda.device(self.params.device):
            out = torch.empty((6,), dtype=torch.float32, device=self.params.device)
            check(lib.scg_lp_head(H, W, self.params.data_ptr(), out.data_ptr(), out.data_ptr() + 4, _lib.ptr(features),
                                  scratch.data_ptr(), nbytes, stream), "scg_lp_head")
        self.terms = out[1:]
        return out[:1].reshape(1, 1, 1, 1)

    def __call__(self, x, y):
        x, y = _images(x, y)
        if not x.is_cuda:
            value, self.terms, _, _ = lpips_torch(x.float(), y.float(), self.convs, self.lins)
            return value
        return self._run(x, y)

    def features(self, x, y=None):
        """The five normalised maps (1,C,h,w) of x — views of a channels-last buffer — and, with y, a second list for y."""
        x, y2 = _images(x, x if y is None else y)
        if not x.is_cuda:
            fx, fy = vgg_taps_torch(x[None].float(), self.convs), vgg_taps_torch(y2[None].float(), self.convs)
            return fx if y is None else (fx, fy)
        _, H, W = x.shape
        n = _lib_lp.load().scg_lp_feature_floats(H, W)
        with torch.cuda.device(x.device):
            buf = torch.empty((n,), dtype=torch.float32, device=x.device)
        self._run(x, y2, features=buf)
        fx, fy, off, h, w = [], [], 0, H, W
        for c in TAP_CHANNELS:
            pair = buf[off:off + 2 * h * w * c].reshape(2, h, w, c).permute(0, 3, 1, 2)
            fx.append(pair[0:1])
            fy.append(pair[1:2])
            off, h, w = off + 2 * h * w * c, h // 2, w // 2
        return fx if y is None else (fx, fy)


def conv3x3(x, weight, bias, relu=True, pool=False, zscore=False):
    """One layer on its own (scg_lp_conv3x3): x (n,cin,h,w), weight (cout,cin,3,3), bias (cout,) on the GPU -> (n,cout,h',w'), a
    view of the channels-last result.  The stage-alone tests go through this."""
    lib = _lib_lp.load()
    stream = _lib.stream_of(x, "conv3x3")
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    xin = x.detach().float().permute(0, 2, 3, 1).contiguous()
    wt = weight.detach().float().permute(0, 2, 3, 1).contiguous()
    b = bias.detach().float().contiguous()
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    with torch.cuda.device(x.device):
        out = torch.empty((n, max(ho, 0), max(wo, 0), cout), dtype=torch.float32, device=x.device)
        flags = (_lib_lp.LP_RELU if relu else 0) | (_lib_lp.LP_POOL if pool else 0) | (_lib_lp.LP_ZSCORE if zscore else 0)
        check(lib.scg_lp_conv3x3(n, cin, cout, h, w, xin.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), flags, stream),
              "scg_lp_conv3x3")
    return out.permute(0, 3, 1, 2)
