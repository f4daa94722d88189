"""The layout of the probe build's log behind the n_tiles cost words of ScgFrame.tile_cost_out: the Python side of
scgaussian_amd/csrc/probe_timeline.h (tests/test_probe_timeline_cpu.py holds the two together).  32-bit words throughout.

Four regions of fixed-size records, one record per wave, signed in its last word; offsets are counted from the first word behind
the cost words, i.e. from index n_tiles of the buffer."""

SCATTER_RECORD = 8       # words of a record of tile_scatter_kernel
GEOMETRY_RECORD = 8      # ... of geometry_hist_kernel
BLEND_RECORD = 8         # ... of tile_blend_forward_kernel, and of the sort's second record per workgroup
BACKWARD_RECORD = 4      # ... of blend_backward_kernel

SCATTER_AT = 0
GEOMETRY_AT = 65792
BLEND_AT = 65792 + 32768
TILE_PAD = 8
BLEND_WORDS_PER_TILE = 40
BACKWARD_WORDS_PER_TILE = 16
TAIL_WORDS = 64

SIG_SCATTER = 0xC0FFEE
SIG_GEOMETRY = 0xC0FFEE00     # | chunks the wave took (low 8 bits)
SIG_BLEND = 0xB1E9D000
SIG_SORT = 0x50B70000
SIG_BACKWARD = 0xBAC00000     # | 4 tile + quadrant (low 20 bits)


def backward_at(n_tiles):
    return BLEND_AT + (n_tiles + TILE_PAD) * BLEND_WORDS_PER_TILE


def log_words(n_tiles):
    """Words behind the cost words that a caller allocates: every probe of the build logs, so all regions must exist."""
    return backward_at(n_tiles) + (n_tiles + TILE_PAD) * BACKWARD_WORDS_PER_TILE + TAIL_WORDS


def big_hints(words):
    """Make every camera's two cost buffers `words` longer than its tile count from now on (the probe build logs behind the cost
    words): wraps scgaussian_amd._frames._hints_for.  Returns a function that gives the record of the one camera rendered since."""
    import torch
    from scgaussian_amd import _frames
    orig = _frames._hints_for

    def wrapper(*a, **k):
        h = orig(*a, **k)
        if h.cost is not None and h.cost[0].numel() < words:
            h.cost = [torch.zeros(h.cost[0].numel() + words, dtype=torch.int32, device=h.cost[0].device) for _ in range(2)]
        return h
    _frames._hints_for = wrapper
    return lambda: next(iter(_frames._CAM_HINTS.values()))
