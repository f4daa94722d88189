"""The flat arena of the ordered view pairs (a -> b) of a reference `view_gs` dictionary, host side: what init_stage.py and seed.py
share.  A segment is (key_a, key_b, offset, M): pair (a, b) holds the M elements [offset, offset + M) of every flat tensor."""
import numpy as np
import torch


def walk(view_gs):
    """(keys, [(a, b, offset, M, match_info of a -> b)]) in dictionary order, as the reference's loops walk; M: the pair's rays."""
    keys, pairs, off = list(view_gs.keys()), [], 0
    for a in keys:
        for b, info in view_gs[a]["match_infos"].items():
            M = info["rays_o"].shape[0]
            pairs.append((a, b, off, M, info))
            off += M
    return keys, pairs


def upload_table(records: np.ndarray, dev) -> torch.Tensor:
    """A numpy record array as a uint8 tensor on `dev`: the device copy of a segment table."""
    return torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).to(dev)


def nested(segments, flat: torch.Tensor, column: bool) -> dict:
    """{a: {b: view of the pair's elements of `flat`}}, (M, 1) when `column`, else (M)."""
    out: dict = {}
    for a, b, off, M in segments:
        v = flat[off:off + M]
        out.setdefault(a, {})[b] = v.view(M, 1) if column else v
    return out


def is_arena(flat: torch.Tensor, tensors, segments) -> bool:
    """Are `tensors` the segments' own views into the fp32 `flat`, in arena order?  Then `flat` is read in place."""
    return all(t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() == flat.data_ptr() + 4 * off
               for t, (_a, _b, off, _M) in zip(tensors, segments))
