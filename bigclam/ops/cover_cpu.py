"""Vectorised CPU best-match between two covers — the CPU path of the
ground-truth evaluation and the oracle for the K8 kernel
(kernels/cover_kernels.hip).  Same contract, bit for bit:

for every community A of X, the community B of Y with c = |A∩B| > 0 that
maximises c/(|A|+|B|) (the argmax of both F1 and Jaccard), fractions
compared EXACTLY by 64-bit integer cross-multiplication, ties to the lowest
Y index; no overlap gives (idx -1, c 0).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def cover_best_match_cpu(
    grp_ptr: np.ndarray,
    grp_nodes: np.ndarray,
    node_ptr: np.ndarray,
    node_comm: np.ndarray,
    size_y: np.ndarray,
) -> Tuple[np.ndarray, np.ndarray]:
    """Returns ``(best_idx int32 [G], best_inter int32 [G])``; the
    arguments are the kernel's (X group-major, Y node-major, |B| sizes)."""
    g = len(grp_ptr) - 1
    gy = len(size_y)
    best_idx = np.full(g, -1, dtype=np.int32)
    best_inter = np.zeros(g, dtype=np.int32)
    if g == 0 or gy == 0 or len(grp_nodes) == 0 or len(node_comm) == 0:
        return best_idx, best_inter
    size_x = np.diff(grp_ptr).astype(np.int64)
    # expand every (x, node) membership over the node's Y-memberships
    x_of = np.repeat(np.arange(g, dtype=np.int64), size_x)
    u = grp_nodes.astype(np.int64)
    cnt = (node_ptr[u + 1] - node_ptr[u]).astype(np.int64)
    total = int(cnt.sum())
    if total == 0:
        return best_idx, best_inter
    starts = np.repeat(node_ptr[u], cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(
        np.cumsum(cnt) - cnt, cnt
    )
    y = node_comm[starts + within].astype(np.int64)
    key, c = np.unique(np.repeat(x_of, cnt) * gy + y, return_counts=True)
    ex = key // gy  # ascending x, then ascending y within x
    ey = key % gy
    ea = size_x[ex]
    eb = size_y.astype(np.int64)[ey]
    c = c.astype(np.int64)
    # exact per-x argmax: doubling tournament over the sorted entries.
    # best[i] = index of the best entry of x's run within [i, i + span);
    # the right-hand candidate always has the higher y, so it must win
    # STRICTLY (ties stay with the lower index).  c < 2^31 and
    # a + b < 2^32, so the cross products fit int64.
    m = len(key)
    best = np.arange(m, dtype=np.int64)
    longest = int(np.bincount(ex).max())
    span = 1
    while span < longest:
        i = np.arange(m - span, dtype=np.int64)
        same = ex[i + span] == ex[i]
        i = i[same]
        l, r = best[i], best[i + span]
        win = c[r] * (ea[l] + eb[l]) > c[l] * (ea[r] + eb[r])
        nb = best.copy()
        nb[i[win]] = r[win]
        best = nb
        span *= 2
    first = np.concatenate([[True], ex[1:] != ex[:-1]])
    head = np.nonzero(first)[0]
    pick = best[head]
    best_idx[ex[head]] = ey[pick].astype(np.int32)
    best_inter[ex[head]] = c[pick].astype(np.int32)
    return best_idx, best_inter
