"""Per-community structural scores of a cover on a graph — which of the K
communities are any good, without a truth file.  The edge-count scoring
functions of Yang & Leskovec ("Defining and evaluating network communities
based on ground-truth"): conductance, internal density, average internal
degree, expansion, cut ratio, Flake-ODF and FOMD.

Every score is a function of a few integers per community S (n = |S|, N
nodes, nnz = 2E CSR entries):

  int_deg(u)  CSR entries v of member u's row with v in S
  vol         sum of deg(u) over S
  m2          sum of int_deg(u) over S (twice the internal edges)
  n_flake     members with 2*int_deg < deg
  n_fomd      members with int_deg > dmed, dmed = floor(median degree)

and, with cut = vol - m2, in fp64 on the host from the integers only:

  conductance          0 if vol == 0, 1 if vol == nnz, else
                       cut / min(vol, nnz - vol)   (K5's guards, core/init.py)
  internal_density     m2 / (n(n-1)), 0 for n < 2
  avg_internal_degree  m2 / n
  expansion            cut / n
  cut_ratio            cut / (n(N-n)), 0 for n == N
  flake_odf            n_flake / n
  fomd                 n_fomd / n

All scores are 0 for an empty community.  The integers come from the K10
HIP kernel when the device is a GPU and from the vectorised CPU
implementation otherwise; both are integer-exact, so the two paths agree
bitwise.  On a GPU box a missing extension is an error, never a silent
fallback (same policy as engine/evaluate.py; ``BIGCLAM_FORCE_TORCH_OPS=1``
is the A/B override).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from ..io.cover import Cover
from ..ops.cover_cpu import community_scores_cpu

SCORE_NAMES = (
    "conductance", "internal_density", "avg_internal_degree", "expansion",
    "cut_ratio", "flake_odf", "fomd",
)


def median_degree_floor(indptr: np.ndarray) -> int:
    """``floor(median of all N degrees)`` in integer arithmetic (for an
    integer i, ``i > median`` is ``i > floor(median)``)."""
    deg = np.diff(np.asarray(indptr, dtype=np.int64))
    n = len(deg)
    if n == 0:
        return 0
    h = n // 2
    if n % 2:
        return int(np.partition(deg, h)[h])
    part = np.partition(deg, (h - 1, h))
    return int((part[h - 1] + part[h]) // 2)


def host_scores(size, vol, m2, n_flake, n_fomd, num_nodes: int,
                nnz: int) -> dict:
    """The seven fp64 score arrays [G] from the per-community integers."""
    n = np.asarray(size, dtype=np.int64)
    vol = np.asarray(vol, dtype=np.int64)
    m2 = np.asarray(m2, dtype=np.int64)
    cut = vol - m2
    g = len(n)
    some = n > 0
    nf = np.where(some, n, 1).astype(np.float64)

    def per_member(num):
        return np.where(some, np.asarray(num, dtype=np.int64) / nf, 0.0)

    cond = np.zeros(g, dtype=np.float64)
    mid = some & (vol != 0) & (vol != nnz)
    cond[some & (vol == nnz) & (vol != 0)] = 1.0
    cond[mid] = cut[mid] / np.minimum(vol[mid], nnz - vol[mid]).astype(
        np.float64
    )
    dens = np.zeros(g, dtype=np.float64)
    two = n >= 2
    dens[two] = m2[two] / (n[two] * (n[two] - 1)).astype(np.float64)
    ratio = np.zeros(g, dtype=np.float64)
    part = some & (n != num_nodes)
    ratio[part] = cut[part] / (n[part] * (num_nodes - n[part])).astype(
        np.float64
    )
    return {
        "conductance": cond,
        "internal_density": dens,
        "avg_internal_degree": per_member(m2),
        "expansion": per_member(cut),
        "cut_ratio": ratio,
        "flake_odf": per_member(n_flake),
        "fomd": per_member(n_fomd),
    }


def community_scores(
    graph, cover: Cover, device: Optional[torch.device] = None,
    tile: Optional[int] = None,
) -> dict:
    """Score every community of ``cover`` on ``graph`` (both over the same
    dense ids).  GPU device -> K10, else the CPU implementation.  Returns
    the per-community integer arrays (``size``, ``vol``, ``m2``, ``cut``,
    ``n_flake``, ``n_fomd``), the seven fp64 score arrays, ``int_deg`` and
    ``deg`` (one per member pair, aligned with ``cover.grp_nodes``) and the
    summary scalars (see :func:`summary`)."""
    n = graph.num_nodes
    if cover.n != n:
        raise ValueError(
            f"cover and graph span different node sets: {cover.n} vs {n}"
        )
    device = torch.device(
        device
        if device is not None
        else ("cuda" if torch.cuda.is_available() else "cpu")
    )
    use_hip = device.type == "cuda" and not os.environ.get(
        "BIGCLAM_FORCE_TORCH_OPS"
    )
    dmed = median_degree_floor(graph.indptr)
    if not use_hip:
        int_deg, vol, m2, n_flake, n_fomd = community_scores_cpu(
            cover.grp_ptr, cover.grp_nodes, graph.indptr, graph.indices, dmed
        )
    else:
        from ..ops import hip as hip_ops  # raises if the extension is missing

        if tile is None:
            largest = int(cover.sizes.max()) if cover.num_comms else 1
            tile = min(hip_ops.score_max_tile(), max(1, largest))
        out = hip_ops.community_scores(
            torch.from_numpy(cover.grp_ptr).to(device),
            torch.from_numpy(cover.grp_nodes).to(device),
            torch.from_numpy(graph.indptr).to(device),
            torch.from_numpy(graph.indices).to(device),
            dmed, tile=tile,
        )
        int_deg, vol, m2, n_flake, n_fomd = (t.cpu().numpy() for t in out)
    nnz = len(graph.indices)
    size = cover.sizes
    res = {
        "size": size, "vol": vol, "m2": m2, "cut": vol - m2,
        "n_flake": n_flake, "n_fomd": n_fomd, "int_deg": int_deg,
        "deg": np.diff(graph.indptr)[cover.grp_nodes.astype(np.int64)],
        "dmed": dmed, "num_nodes": n, "nnz": nnz,
    }
    res.update(host_scores(size, vol, m2, n_flake, n_fomd, n, nnz))
    keep = size > 0

    def mean(name):
        return float(res[name][keep].mean()) if keep.any() else 0.0

    res.update({
        "mean_conductance": mean("conductance"),
        "median_conductance": (
            float(np.median(res["conductance"][keep])) if keep.any() else 0.0
        ),
        "mean_internal_density": mean("internal_density"),
        "mean_flake_odf": mean("flake_odf"),
        "mean_fomd": mean("fomd"),
        "n_scored": int(keep.sum()),
        "nodes_covered": (
            float(np.count_nonzero(np.diff(cover.node_ptr))) / n if n else 0.0
        ),
    })
    return res


SUMMARY_KEYS = (
    "mean_conductance", "median_conductance", "mean_internal_density",
    "mean_flake_odf", "mean_fomd", "n_scored", "nodes_covered",
)


def summary(result: dict) -> dict:
    """The JSON-serialisable scalars of a ``community_scores`` result."""
    return {k: result[k] for k in SUMMARY_KEYS}


def score_trainer(trainer) -> Optional[dict]:
    """Extract the fitted model's communities (sharded K7 — every rank
    takes part in its gather; no further collective here) and score them on
    rank 0, on the trainer's device, against ``trainer.graph`` — the graph
    the model was fitted on.  Other ranks return ``None``."""
    from .extract import extract_communities_sharded

    pairs = extract_communities_sharded(trainer)
    if trainer.rank != 0:
        return None
    return score_pairs(pairs, trainer)


def score_pairs(pairs, trainer) -> dict:
    """Score the rank-0 ``(comms, nodes)`` membership pairs of
    ``extract_communities_sharded`` against ``trainer.graph``."""
    g = trainer.graph
    det = Cover.from_pairs(
        pairs[0], pairs[1], g.num_nodes, num_comms=trainer.cfg.k
    )
    return community_scores(g, det, device=trainer.state.device)


def write_per_community(path: str, result: dict) -> None:
    """TSV of the integers and the seven scores of every community."""
    with open(path, "w") as f:
        f.write(
            "community\tsize\tvolume\tinternal_edges\tcut\t"
            + "\t".join(SCORE_NAMES) + "\n"
        )
        for c in range(len(result["size"])):
            f.write(
                f"{c}\t{int(result['size'][c])}\t{int(result['vol'][c])}"
                f"\t{int(result['m2'][c]) // 2}\t{int(result['cut'][c])}\t"
                + "\t".join(f"{result[s][c]:.17g}" for s in SCORE_NAMES)
                + "\n"
            )


def write_per_member(path: str, result: dict, cover: Cover,
                     raw_ids: Optional[np.ndarray] = None) -> None:
    """TSV of every (community, node) pair: community, raw id, degree,
    internal degree."""
    nodes = cover.grp_nodes.astype(np.int64)
    deg = result["deg"]
    ids = nodes if raw_ids is None else np.asarray(raw_ids)[nodes]
    comms = cover.comms
    with open(path, "w") as f:
        f.write("community\tnode\tdegree\tinternal_degree\n")
        for i in range(len(nodes)):
            f.write(
                f"{int(comms[i])}\t{int(ids[i])}\t{int(deg[i])}"
                f"\t{int(result['int_deg'][i])}\n"
            )
