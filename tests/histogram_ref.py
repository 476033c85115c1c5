"""NumPy restatement of the histogram's rule (include/bldp.h) for one window, and
the table of plan cases that the host and the GPU tests share.

``a`` is the selected (nc, ni, nt) Float32 window.  With lo32 = Float32(lo),
hi32 = Float32(hi) and s = Float32(B) / (hi32 - lo32) (Float32 operations), a
sample x goes, in this order, to ``nan`` when x != x, to ``below`` when
x < lo32, to ``above`` when x >= hi32, else to bin
min(floor(Float32(Float32(x - lo32) * s)), B - 1).  For every F x T block the
B + 3 counts: planes 0 .. B-1 the bins, B below, B + 1 above, B + 2 nan."""
from __future__ import annotations

import numpy as np

from masked_ref import masked_blocks


def hist_scale(B, lo, hi):
    """(lo32, hi32, s) as Float32 scalars, every operation rounded to Float32."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    w = np.float32(hi32 - lo32)
    s = np.float32(np.float32(B) / w)
    assert np.isfinite(lo32) and np.isfinite(hi32) and lo32 < hi32
    assert np.isfinite(w) and np.isfinite(s) and s > 0
    return lo32, hi32, s


def hist_k(x, B, lo, hi):
    """The unclamped k = floor((x - lo32) * s) of Float32 samples inside
    [lo32, hi32), as int64."""
    lo32, hi32, s = hist_scale(B, lo, hi)
    x = np.asarray(x, dtype=np.float32)
    assert ((x >= lo32) & (x < hi32)).all()
    d = (x - lo32).astype(np.float32)
    m = (d * s).astype(np.float32)
    return np.floor(m).astype(np.int64)


def hist_planes(x, B, lo, hi):
    """The plane (0 .. B + 2) of every sample of a Float32 array."""
    lo32, hi32, s = hist_scale(B, lo, hi)
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (x >= lo32) & (x < hi32)
        d = (np.where(inside, x, lo32) - lo32).astype(np.float32)  # classed first
        m = (d * s).astype(np.float32)
        q = np.minimum(np.floor(m).astype(np.int64), B - 1)
        q = np.where(x < lo32, B, q)
        q = np.where(x >= hi32, B + 1, q)
        q = np.where(x != x, B + 2, q)
    return q


def histogram_ref(a, B, lo, hi, F=1, T=1):
    """The (nc/F, ni, nt/T, B + 3) int64 counts of every block."""
    a = np.asarray(a, dtype=np.float32)
    q = masked_blocks(hist_planes(a, B, lo, hi), F, T)  # (nco, ni, nto, F*T)
    nco, ni, nto, n = q.shape
    blk = np.arange(nco * ni * nto, dtype=np.int64).reshape(nco, ni, nto, 1)
    flat = (blk * (B + 3) + q).ravel()
    return np.bincount(flat, minlength=nco * ni * nto * (B + 3)).reshape(nco, ni, nto, B + 3)


def hist_edges_ref(B, lo, hi):
    lo32, hi32 = float(np.float32(lo)), float(np.float32(hi))
    return lo32 + np.arange(B + 1, dtype=np.float64) * (hi32 - lo32) / B


# The plan cases, for a device of 256 compute units (an MI355X; what the plan
# call assumes without a GPU).  name -> (dims (nchan, nif, ntime), F, T, B, window
# or None, (path, vector loads, chunks per block, blocks per workgroup)).
# For every path and load width the first entry is the smallest shape that
# selects it; the others are shapes at which the walk can go wrong: a last chunk
# and a last column tile that are short, a last group of fewer blocks, rows and
# channels that are no multiple of the lanes.
#  - "block": one block along the channels, or blocks wider than a workgroup's
#    row of lanes (F > 512 float4 channels, F > 128 dword channels).
#  - "block_split": a lone block of >= 2 * 32768 samples, the fewest that two
#    workgroups share; by rows first, then by column tiles of >= 256 items.
#  - "lanes": two blocks or more that fit a workgroup's row.
#  - "lanes_tsplit": the same with >= 2 * 32768 samples in the group.
PLAN_CASES = {
    "block_vec_min": ((4, 1, 1), 4, 1, 64, None, ("block", 1, 1, 1)),
    "block_vec": ((3 * 516, 2, 6), 516, 3, 64, None, ("block", 1, 1, 1)),
    "block_dword_min": ((1, 1, 1), 1, 1, 64, None, ("block", 0, 1, 1)),
    "block_dword": ((3 * 129, 2, 6), 129, 3, 64, None, ("block", 0, 1, 1)),
    "block_dword_step2": ((2 * 1032, 1, 5), 1032, 5, 64, [0, 1032, 2, 0, 1, 1, 0, 5, 1],
                          ("block", 0, 1, 1)),
    "block_split_vec_min": ((256, 1, 256), 256, 256, 64, None, ("block_split", 1, 2, 1)),
    "block_split_vec": ((512, 1, 1000), 512, 1000, 64, None, ("block_split", 1, 15, 1)),
    "block_split_vec_tiles": ((131076, 1, 2), 131076, 2, 64, None, ("block_split", 1, 8, 1)),
    "block_split_dword_min": ((258, 1, 255), 258, 255, 64, None, ("block_split", 0, 2, 1)),
    "block_split_dword": ((1030, 2, 257), 515, 257, 256, [1029, 1030, -1, 0, 2, 1, 0, 257, 1],
                          ("block_split", 0, 4, 1)),
    "lanes_vec_min": ((8, 1, 1), 4, 1, 64, None, ("lanes", 1, 1, 2)),
    "lanes_vec": ((65 * 64, 2, 48), 64, 16, 64, None, ("lanes", 1, 1, 16)),
    "lanes_vec_f1": ((200, 2, 37), 1, 37, 256, None, ("lanes", 1, 1, 32)),
    "lanes_dword_min": ((2, 1, 1), 1, 1, 64, None, ("lanes", 0, 1, 2)),
    "lanes_dword": ((35 * 5, 2, 9), 5, 3, 64, None, ("lanes", 0, 1, 32)),
    "lanes_tsplit_vec_min": ((4, 1, 16384), 1, 16384, 64, None, ("lanes_tsplit", 1, 2, 4)),
    "lanes_tsplit_vec": ((64, 1, 8001), 1, 8001, 64, None, ("lanes_tsplit", 1, 15, 64)),
    "lanes_tsplit_dword_min": ((2, 1, 32768), 1, 32768, 64, None, ("lanes_tsplit", 0, 2, 2)),
    "lanes_tsplit_dword": ((150, 1, 3001), 3, 3001, 64, [149, 150, -1, 0, 1, 1, 3000, 3001, -1],
                           ("lanes_tsplit", 0, 17, 64)),
}
