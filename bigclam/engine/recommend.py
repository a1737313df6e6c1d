"""Top-n link recommendation: which missing edges does the fitted model
consider most likely?

The model says P(edge u-v) = 1 - exp(-F_u·F_v).  ``F_u·F_v`` is nonzero
only when u and v share a nonzero column of F, and a fitted F has a few
nonzeros per row, so the global top-n of row u of F·Fᵀ over all N nodes is
the top-n over the members of u's few communities: one row of a
sparse·sparseᵀ product.  ``recommend`` computes that for a list of query
nodes from the model's sparse form (core/sparse_model.py) — the K11 HIP
kernel on a GPU, ``ops/links_cpu.py`` otherwise; the two agree bitwise.
A node's own CSR neighbours and the node itself are never recommended.

A query's row is the exact global top-n whenever it has at least n
candidates (``n_cand >= n``): every node outside the candidate set scores
exactly 0.  ``exact_frac`` is the share of such queries; the other rows are
padded with (-1, 0) — the model has no opinion on the rest.

On a GPU box a missing extension is an error, never a silent fallback
(same policy as engine/scores.py; ``BIGCLAM_FORCE_TORCH_OPS=1`` is the A/B
override).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from ..core.sparse_model import (
    DEFAULT_MAX_NNZ,
    SparseModel,
    nonzero_triples,
)
from ..ops.links_cpu import candidate_bound, topn_links_cpu


def recommend(
    graph, model: SparseModel, queries=None, n: int = 10,
    device: Optional[torch.device] = None,
    max_community_size: Optional[int] = None, **kernel_args,
) -> dict:
    """The ``n`` most likely missing links of every query node (dense ids;
    default: all nodes) under ``model`` on ``graph``.  GPU device -> K11,
    else the CPU implementation.  ``max_community_size`` drops the columns
    with more members from the model first (``columns_dropped``).  Returns
    ``top_id`` int32 [Q, n] (-1 pads), ``top_score`` float32 [Q, n],
    ``prob`` = 1 - exp(-score) float64 [Q, n], ``n_cand`` int32 [Q],
    ``queries`` int32 [Q], ``n``, ``work`` (sum of the per-query candidate
    bounds T_u), ``exact_frac`` and ``columns_dropped``; on the GPU also
    ``n_lds`` / ``n_global`` / ``global_batches``, the kernel's table
    placement.  ``kernel_args`` go to ``ops.hip.topn_links``."""
    if model.n != graph.num_nodes:
        raise ValueError(
            f"model and graph span different node sets: {model.n} vs "
            f"{graph.num_nodes}"
        )
    device = torch.device(
        device
        if device is not None
        else ("cuda" if torch.cuda.is_available() else "cpu")
    )
    use_hip = device.type == "cuda" and not os.environ.get(
        "BIGCLAM_FORCE_TORCH_OPS"
    )
    if max_community_size is not None:
        model = model.drop_columns_larger_than(max_community_size)
    if queries is None:
        queries = np.arange(graph.num_nodes, dtype=np.int32)
    queries = np.ascontiguousarray(queries, dtype=np.int32)
    if len(queries) and (queries.min() < 0
                         or queries.max() >= graph.num_nodes):
        raise ValueError("query ids must lie in [0, N)")
    n = int(n)
    extra = {}
    if not use_hip:
        if kernel_args:
            raise TypeError(
                f"kernel arguments {sorted(kernel_args)} need a GPU device"
            )
        host = model.numpy()
        top_id, top_score, n_cand = topn_links_cpu(
            host, graph.indptr, graph.indices, queries, n
        )
        work = int(candidate_bound(host, queries).sum())
    else:
        from ..ops import hip as hip_ops  # raises if the extension is missing

        t_id, t_score, t_cand, info = hip_ops.topn_links(
            model.to(device),
            torch.from_numpy(graph.indptr).to(device),
            torch.from_numpy(graph.indices).to(device),
            torch.from_numpy(queries).to(device),
            n, **kernel_args,
        )
        top_id, top_score, n_cand = (
            t.cpu().numpy() for t in (t_id, t_score, t_cand)
        )
        work = info["work"]
        extra = {key: info[key]
                 for key in ("n_lds", "n_global", "global_batches")}
    return dict(
        extra,
        top_id=top_id, top_score=top_score, n_cand=n_cand,
        prob=-np.expm1(-top_score.astype(np.float64)),
        queries=queries, n=n, work=work,
        exact_frac=float((n_cand >= n).mean()) if len(queries) else 0.0,
        columns_dropped=int(model.columns_dropped),
    )


def gather_sparse_model(trainer,
                        max_nnz: int = DEFAULT_MAX_NNZ
                        ) -> Optional[SparseModel]:
    """The whole model's sparse form on rank 0 (``None`` elsewhere).
    Collective: every rank lists the nonzeros of its own rows and sends the
    (row, column, value) arrays to rank 0 as tensors; rank order is global
    row order, so the concatenation is row-major."""
    st = trainer.state
    k = trainer.cfg.k
    rows, cols, vals = nonzero_triples(
        st.F_local, k, row_offset=trainer.shard.start, max_nnz=max_nnz
    )
    if trainer.world_size > 1:
        import torch.distributed as dist

        count = torch.tensor([rows.numel()], device=st.device,
                             dtype=torch.int64)
        counts = [torch.zeros_like(count) for _ in range(trainer.world_size)]
        dist.all_gather(counts, count)
        if trainer.rank != 0:
            if rows.numel():
                for t in (rows, cols, vals):
                    dist.send(t.contiguous(), dst=0)
            return None
        parts = [(rows, cols, vals)]
        for r in range(1, trainer.world_size):
            m = int(counts[r])
            bufs = (
                torch.empty(m, device=st.device, dtype=torch.int64),
                torch.empty(m, device=st.device, dtype=torch.int64),
                torch.empty(m, device=st.device, dtype=torch.float32),
            )
            if m:
                for t in bufs:
                    dist.recv(t, src=r)
            parts.append(bufs)
        total = sum(int(p[0].numel()) for p in parts)
        if total > max_nnz:
            raise ValueError(
                f"F has {total} nonzeros, more than max_nnz = {max_nnz}"
            )
        rows, cols, vals = (torch.cat([p[i] for p in parts])
                            for i in range(3))
    return SparseModel.from_triples(
        rows, cols, vals, trainer.graph.num_nodes, k
    )


def recommend_trainer(trainer, queries=None, n: int = 10,
                      max_community_size: Optional[int] = None,
                      **kernel_args) -> Optional[dict]:
    """Recommend from the trainer's current F against ``trainer.graph`` —
    the graph the model was fitted on.  Collective (the sparse model is
    gathered to rank 0, which computes on the trainer's device); the dict
    on rank 0, ``None`` elsewhere."""
    model = gather_sparse_model(trainer)
    if trainer.rank != 0:
        return None
    return recommend(
        trainer.graph, model, queries=queries, n=n,
        device=trainer.state.device,
        max_community_size=max_community_size, **kernel_args,
    )


def heldout_ranking(result: dict, split) -> dict:
    """How many held-out edges the recommendations recover.  Over the
    queried nodes with at least one held-out edge: ``heldout_recall_at_n``
    = hits / Σ_u |held(u)| (every held-out edge counts from both of its
    endpoints), ``heldout_hit_rate`` = the share of those nodes with at
    least one hit, ``heldout_rank_queries`` = their number."""
    num = int(split.train.num_nodes)
    pos = np.asarray(split.pos, dtype=np.int64).reshape(-1, 2)
    held = np.unique(np.concatenate(
        [pos[:, 0] * num + pos[:, 1], pos[:, 1] * num + pos[:, 0]]
    ))  # sorted keys u * N + v, both directions
    held_u = held // max(num, 1)
    queries = np.asarray(result["queries"], dtype=np.int64)
    top = np.asarray(result["top_id"], dtype=np.int64)
    key = queries[:, None] * num + top
    at = np.searchsorted(held, key)
    hit = np.zeros(key.shape, dtype=bool)
    ok = (top >= 0) & (at < len(held))
    hit[ok] = held[at[ok]] == key[ok]
    n_held = (np.searchsorted(held_u, queries, side="right")
              - np.searchsorted(held_u, queries, side="left"))
    has = n_held > 0
    total = int(n_held[has].sum())
    hits = int(hit[has].sum())
    return {
        "heldout_recall_at_n": hits / total if total else 0.0,
        "heldout_hit_rate": (
            float(hit[has].any(axis=1).mean()) if has.any() else 0.0
        ),
        "heldout_rank_queries": int(has.sum()),
        "n": int(result["n"]),
    }


def write_recommendations(path: str, result: dict,
                          raw_ids: Optional[np.ndarray] = None) -> None:
    """TSV ``node  candidate  score  prob`` in raw ids: one line per
    recommendation, queries in the order given, best first; pads are
    omitted."""
    queries = np.asarray(result["queries"], dtype=np.int64)
    top = np.asarray(result["top_id"], dtype=np.int64)

    def raw(x):
        return x if raw_ids is None else np.asarray(raw_ids)[x]

    with open(path, "w") as f:
        f.write("node\tcandidate\tscore\tprob\n")
        for i in range(len(queries)):
            m = int((top[i] >= 0).sum())
            if m == 0:
                continue
            u = int(raw(queries[i]))
            cand = raw(top[i, :m])
            for j in range(m):
                f.write(
                    f"{u}\t{int(cand[j])}"
                    f"\t{float(result['top_score'][i, j]):.9g}"
                    f"\t{float(result['prob'][i, j]):.17g}\n"
                )
