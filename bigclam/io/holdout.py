"""Edge hold-out split for model selection without a ground-truth cover.

The BigCLAM paper chooses K by held-out likelihood: hide a fraction of the
node pairs, fit on the rest, score the hidden pairs.  ``split_edges`` hides
``frac`` of the EDGES (the positives) and draws a uniform sample of
non-edges (the negatives) that stands for the same fraction of all
non-edges; ``engine/holdout.py`` turns the two lists into a likelihood and
a link-prediction AUC.

The train graph keeps the node id space of the input graph (same
``raw_ids``, same N), so F rows, ``--out`` and ``--truth`` line up with the
full graph.  To keep that space meaningful every node keeps at least one
train edge: an edge is held out only while both endpoints still have
degree > 1.  Where that guard leaves fewer than ``round(frac * E)`` edges
to take, the split holds out what it can (``requested - len(pos)`` is the
shortfall).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .edgelist import Graph


@dataclass
class HoldoutSplit:
    train: Graph  # full node space, held-out edges removed
    pos: np.ndarray  # int64 [P, 2] held-out edges, u < v, sorted by (u, v)
    neg: np.ndarray  # int64 [Q, 2] sampled non-edges, u < v, sorted
    neg_weight: float  # non-edges the sample stands for
    requested: int  # round(frac * E); len(pos) may fall short


def canonical_edges(graph: Graph) -> np.ndarray:
    """The undirected edges as int64 [E, 2] with u < v, sorted by (u, v)."""
    n = graph.num_nodes
    src = np.repeat(np.arange(n, dtype=np.int64), graph.degrees())
    dst = graph.indices.astype(np.int64)
    keep = src < dst
    key = np.sort(src[keep] * n + dst[keep])
    return np.stack([key // max(n, 1), key % max(n, 1)], axis=1)


def _rank_within_node(nodes: np.ndarray) -> np.ndarray:
    """For a list of node ids (one per candidate endpoint, in candidate
    order): how many earlier entries name the same node."""
    order = np.argsort(nodes, kind="stable")
    s = nodes[order]
    first = np.ones(len(s), dtype=bool)
    first[1:] = s[1:] != s[:-1]
    start = np.maximum.accumulate(np.where(first, np.arange(len(s)), 0))
    rank = np.empty(len(s), dtype=np.int64)
    rank[order] = np.arange(len(s)) - start
    return rank


def _pick_heldout(edges: np.ndarray, deg: np.ndarray, target: int,
                  rng: np.random.Generator) -> np.ndarray:
    """Indices into ``edges`` of the held-out set: a random permutation is
    consumed in rounds.  A round looks at as many queued candidates as are
    still wanted and lets node w lose at most ``deg[w] - 1`` of them — the
    candidates that rank within that budget at BOTH endpoints (in
    permutation order) are accepted together, which cannot take any node
    below degree 1 whatever else the round accepts.  The others are retried
    in later rounds against the updated degrees; a candidate with an
    endpoint at degree 1 can never become eligible again (degrees only
    fall) and leaves the queue.  The first queued candidate always fits
    its budgets, so every round makes progress."""
    deg = deg.astype(np.int64).copy()
    queue = rng.permutation(len(edges))
    taken = []
    need = target
    while need > 0 and len(queue):
        u, v = edges[queue, 0], edges[queue, 1]
        queue = queue[(deg[u] > 1) & (deg[v] > 1)]
        if not len(queue):
            break
        head = queue[:need]
        hu, hv = edges[head, 0], edges[head, 1]
        # endpoints interleaved (u0, v0, u1, v1, ...) = candidate order
        rank = _rank_within_node(edges[head].reshape(-1)).reshape(-1, 2)
        ok = (rank[:, 0] < deg[hu] - 1) & (rank[:, 1] < deg[hv] - 1)
        acc = head[ok]
        taken.append(acc)
        need -= len(acc)
        deg -= np.bincount(
            np.concatenate([hu[ok], hv[ok]]), minlength=len(deg)
        )
        queue = np.concatenate([head[~ok], queue[len(head):]])
    if not taken:
        return np.empty(0, dtype=np.int64)
    return np.concatenate(taken)


def _sample_non_edges(n: int, edge_keys: np.ndarray, q: int,
                      rng: np.random.Generator) -> np.ndarray:
    """``q`` distinct uniform pairs u < v that are not in ``edge_keys``
    (sorted int64 keys u * n + v), as sorted keys."""
    total = n * (n - 1) // 2 - len(edge_keys)
    q = min(q, total)
    if q <= 0:
        return np.empty(0, dtype=np.int64)
    if 2 * q > total:
        # rejection would stall: enumerate the (few) non-edges instead
        iu, iv = np.triu_indices(n, k=1)
        keys = iu.astype(np.int64) * n + iv
        pos = np.searchsorted(edge_keys, keys)
        hit = np.zeros(len(keys), dtype=bool)
        inb = pos < len(edge_keys)
        hit[inb] = edge_keys[pos[inb]] == keys[inb]
        return np.sort(rng.choice(keys[~hit], size=q, replace=False))
    got = np.empty(0, dtype=np.int64)
    while len(got) < q:
        m = int((q - len(got)) * 1.2) + 16
        a = rng.integers(0, n, size=m, dtype=np.int64)
        b = rng.integers(0, n, size=m, dtype=np.int64)
        keys = np.minimum(a, b) * n + np.maximum(a, b)
        keys = keys[a != b]
        pos = np.searchsorted(edge_keys, keys)
        hit = np.zeros(len(keys), dtype=bool)
        inb = pos < len(edge_keys)
        hit[inb] = edge_keys[pos[inb]] == keys[inb]
        cand = np.concatenate([got, keys[~hit]])
        # distinct, keeping draw order so the cut at q stays uniform
        _, first = np.unique(cand, return_index=True)
        got = cand[np.sort(first)]
    return np.sort(got[:q])


def split_edges(graph: Graph, frac: float, seed: int,
                neg_ratio: float = 1.0) -> HoldoutSplit:
    """Hold out ``round(frac * E)`` edges (degree guard permitting) and
    sample ``round(neg_ratio * P)`` non-edges of the FULL graph.
    Deterministic in ``(graph, frac, seed, neg_ratio)``."""
    if not 0.0 < frac < 1.0:
        raise ValueError(f"frac must be in (0, 1), got {frac}")
    if not neg_ratio > 0.0:
        raise ValueError(f"neg_ratio must be > 0, got {neg_ratio}")
    n = graph.num_nodes
    edges = canonical_edges(graph)
    e = len(edges)
    requested = int(round(frac * e))
    rng = np.random.default_rng(seed)

    held = np.sort(_pick_heldout(edges, graph.degrees(), requested, rng))
    pos = edges[held]  # edges are (u, v)-sorted, so is any sorted subset

    # train CSR: drop both directions of every held-out edge
    src = np.repeat(np.arange(n, dtype=np.int64), graph.degrees())
    dst = graph.indices.astype(np.int64)
    dkey = src * n + dst
    drop = np.sort(
        np.concatenate([pos[:, 0] * n + pos[:, 1], pos[:, 1] * n + pos[:, 0]])
    )
    at = np.searchsorted(drop, dkey)
    gone = np.zeros(len(dkey), dtype=bool)
    inb = at < len(drop)
    gone[inb] = drop[at[inb]] == dkey[inb]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src[~gone], minlength=n), out=indptr[1:])
    train = Graph(
        indptr=indptr,
        indices=graph.indices[~gone].astype(np.int32),
        raw_ids=graph.raw_ids,
    )

    q = int(round(neg_ratio * len(pos)))
    nkeys = _sample_non_edges(n, edges[:, 0] * n + edges[:, 1], q, rng)
    neg = np.stack([nkeys // max(n, 1), nkeys % max(n, 1)], axis=1)
    return HoldoutSplit(
        train=train,
        pos=pos,
        neg=neg.astype(np.int64).reshape(-1, 2),
        neg_weight=float(frac * (n * (n - 1) // 2 - e)),
        requested=requested,
    )
