"""Vectorised CPU cover operations: the best match between two covers (CPU
path of the ground-truth evaluation, oracle of K8) and the per-community
edge counts of a cover on a graph (``community_scores_cpu``, CPU path of
the structural scores, oracle of K10).

Best match — same contract as kernels/cover_kernels.hip, bit for bit:

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


def community_scores_cpu(
    grp_ptr: np.ndarray,
    grp_nodes: np.ndarray,
    indptr: np.ndarray,
    indices: np.ndarray,
    dmed: int,
    chunk: int = 1 << 22,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Per-community integer edge counts of a cover on a graph — the CPU
    path of the structural scores and the oracle for the K10 kernel
    (kernels/score_kernels.hip).  Same contract, bit for bit.

    The graph is a symmetric CSR (``indptr`` int64 [N+1], ``indices`` int32
    [nnz]); the cover is group-major with members ascending per community.
    Returns ``(int_deg int32 [M], vol int64 [G], m2 int64 [G], n_flake
    int32 [G], n_fomd int32 [G])``: for member pair m = (x, u), ``int_deg``
    is the number of CSR entries of row u inside community x; per
    community, ``vol`` sums the members' degrees, ``m2`` their ``int_deg``,
    ``n_flake`` counts members with ``2*int_deg < deg`` and ``n_fomd`` those
    with ``int_deg > dmed``.  Member ids outside [0, N) are skipped.

    The members' rows are expanded ``chunk`` entries at a time and
    membership is a ``searchsorted`` of the key ``x*N + v`` in the cover's
    sorted (community, node) keys."""
    g = len(grp_ptr) - 1
    n = len(indptr) - 1
    m = len(grp_nodes)
    int_deg = np.zeros(m, dtype=np.int32)
    vol = np.zeros(g, dtype=np.int64)
    m2 = np.zeros(g, dtype=np.int64)
    n_flake = np.zeros(g, dtype=np.int32)
    n_fomd = np.zeros(g, dtype=np.int32)
    if g == 0 or m == 0:
        return int_deg, vol, m2, n_flake, n_fomd
    size_x = np.diff(grp_ptr).astype(np.int64)
    x_of = np.repeat(np.arange(g, dtype=np.int64), size_x)
    u = grp_nodes.astype(np.int64)
    ok = (u >= 0) & (u < n)
    us = np.where(ok, u, 0)
    deg = np.where(ok, indptr[us + 1] - indptr[us], 0).astype(np.int64)
    stride = max(n, 1)
    keys = x_of * stride + us  # ascending: (community, node) order
    keys = keys[ok]
    ends = np.cumsum(deg)
    lo = 0
    while lo < m:
        # the longest run of members whose rows hold <= chunk entries (one
        # member at least, so a hub row is a chunk of its own)
        base = ends[lo] - deg[lo]
        hi = int(np.searchsorted(ends, base + chunk, side="right"))
        hi = min(max(hi, lo + 1), m)
        cnt = deg[lo:hi]
        total = int(cnt.sum())
        if total:
            starts = np.repeat(indptr[us[lo:hi]], cnt)
            within = np.arange(total, dtype=np.int64) - np.repeat(
                np.cumsum(cnt) - cnt, cnt
            )
            v = indices[starts + within].astype(np.int64)
            owner = np.repeat(np.arange(lo, hi, dtype=np.int64), cnt)
            key = x_of[owner] * stride + v
            pos = np.searchsorted(keys, key)
            hit = pos < len(keys)
            hit[hit] = keys[pos[hit]] == key[hit]
            int_deg[lo:hi] = np.bincount(
                owner[hit] - lo, minlength=hi - lo
            ).astype(np.int32)
        lo = hi
    d = int_deg.astype(np.int64)
    np.add.at(vol, x_of, deg)
    np.add.at(m2, x_of, d)
    n_flake[:] = np.bincount(
        x_of[ok & (2 * d < deg)], minlength=g
    ).astype(np.int32)
    n_fomd[:] = np.bincount(
        x_of[ok & (d > int(dmed))], minlength=g
    ).astype(np.int32)
    return int_deg, vol, m2, n_flake, n_fomd
