"""Ground-truth evaluation: average best-match F1 / Jaccard between a
detected and a true cover (the BigCLAM paper's headline recovery metric;
absent from the reference implementation).

For A in one cover and B in the other, c = |A∩B|, F1 = 2c/(|A|+|B|),
Jaccard = c/(|A|+|B|-c).  ``best(A)`` is the B with c > 0 maximising
c/(|A|+|B|) — one argmax for both scores — chosen EXACTLY (integer
cross-multiplication, ties to the lowest index; no overlap: idx -1, score
0).  ``avg_f1 = (mean_A F1(A, best(A)) + mean_B F1(B, best(B))) / 2`` over
the non-empty communities of each side; ``avg_jaccard`` likewise.  Scores
are fp64 on the host from the integer triples (|A|, |B|, c), so the GPU and
CPU paths agree bitwise.

The matching runs on the K8 HIP kernel when the device is a GPU and on the
vectorised CPU implementation otherwise.  On a GPU box a missing extension
is an error, never a silent fallback (same policy as core/state.py;
``BIGCLAM_FORCE_TORCH_OPS=1`` is the A/B override).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from ..io.cover import Cover
from ..ops.cover_cpu import cover_best_match_cpu


def _device_views(cover: Cover, device: torch.device) -> dict:
    key = str(device)
    views = cover._dev.get(key)
    if views is None:
        views = {
            name: torch.from_numpy(getattr(cover, name)).to(device)
            for name in ("grp_ptr", "grp_nodes", "node_ptr", "node_comm",
                         "sizes")
        }
        cover._dev[key] = views
    return views


def best_match(
    x: Cover, y: Cover, device: Optional[torch.device] = None,
    tile: Optional[int] = None,
) -> Tuple[np.ndarray, np.ndarray]:
    """``(best_idx, best_inter)`` int32 [x.num_comms]: the best Y-community
    for every X-community.  GPU device -> K8, else the CPU implementation."""
    if x.n != y.n:
        raise ValueError(f"covers span different node sets: {x.n} vs {y.n}")
    device = torch.device(
        device
        if device is not None
        else ("cuda" if torch.cuda.is_available() else "cpu")
    )
    use_hip = device.type == "cuda" and not os.environ.get(
        "BIGCLAM_FORCE_TORCH_OPS"
    )
    if not use_hip:
        return cover_best_match_cpu(
            x.grp_ptr, x.grp_nodes, y.node_ptr, y.node_comm, y.sizes
        )
    from ..ops import hip as hip_ops  # raises if the extension is missing

    xv = _device_views(x, device)
    yv = _device_views(y, device)
    idx, inter = hip_ops.cover_best_match(
        xv["grp_ptr"], xv["grp_nodes"], yv["node_ptr"], yv["node_comm"],
        yv["sizes"], tile=tile,
    )
    return idx.cpu().numpy(), inter.cpu().numpy()


def _scores(size_x, size_y, idx, inter):
    """fp64 (f1, jaccard) per X-community from the integer triples."""
    a = size_x.astype(np.int64)
    c = inter.astype(np.int64)
    hit = idx >= 0
    b = np.zeros_like(a)
    b[hit] = size_y.astype(np.int64)[idx[hit]]
    f1 = np.zeros(len(a), dtype=np.float64)
    jac = np.zeros(len(a), dtype=np.float64)
    f1[hit] = 2.0 * c[hit] / (a[hit] + b[hit])
    jac[hit] = c[hit] / (a[hit] + b[hit] - c[hit]).astype(np.float64)
    return f1, jac


def _mean_nonempty(v, sizes) -> float:
    keep = sizes > 0
    return float(v[keep].mean()) if keep.any() else 0.0


def evaluate_covers(
    det: Cover, truth: Cover, device=None, tile: Optional[int] = None
) -> dict:
    """Average best-match F1/Jaccard of ``det`` against ``truth`` (both
    over the same dense node ids) plus the per-community matches."""
    d_idx, d_int = best_match(det, truth, device, tile)
    t_idx, t_int = best_match(truth, det, device, tile)
    d_f1, d_j = _scores(det.sizes, truth.sizes, d_idx, d_int)
    t_f1, t_j = _scores(truth.sizes, det.sizes, t_idx, t_int)
    f1_dt = _mean_nonempty(d_f1, det.sizes)
    f1_td = _mean_nonempty(t_f1, truth.sizes)
    j_dt = _mean_nonempty(d_j, det.sizes)
    j_td = _mean_nonempty(t_j, truth.sizes)
    return {
        "avg_f1": 0.5 * (f1_dt + f1_td),
        "avg_jaccard": 0.5 * (j_dt + j_td),
        "f1_det_to_truth": f1_dt,
        "f1_truth_to_det": f1_td,
        "jaccard_det_to_truth": j_dt,
        "jaccard_truth_to_det": j_td,
        "n_detected": int((det.sizes > 0).sum()),
        "n_truth": int((truth.sizes > 0).sum()),
        "truth_nodes_dropped": int(truth.dropped),
        "per_detected": {
            "size": det.sizes, "idx": d_idx, "inter": d_int, "f1": d_f1,
            "jaccard": d_j,
        },
        "per_truth": {
            "size": truth.sizes, "idx": t_idx, "inter": t_int, "f1": t_f1,
            "jaccard": t_j,
        },
    }


def summary(result: dict) -> dict:
    """The JSON-serialisable scalars of an ``evaluate_covers`` result."""
    return {
        k: v for k, v in result.items()
        if k not in ("per_detected", "per_truth")
    }


def evaluate_pairs(pairs, num_nodes: int, k: int, truth: Cover,
                   device=None) -> dict:
    """Evaluate the rank-0 ``(comms, nodes)`` membership pairs of
    ``extract_communities_sharded`` against ``truth``."""
    det = Cover.from_pairs(pairs[0], pairs[1], num_nodes, num_comms=k)
    return evaluate_covers(det, truth, device=device)


def evaluate_trainer(trainer, truth: Cover) -> Optional[dict]:
    """Extract the fitted model's communities (sharded K7 — every rank
    takes part in its gather; no further collective here) and evaluate them
    against ``truth`` on rank 0, on the trainer's device.  Other ranks
    return ``None``."""
    from .extract import extract_communities_sharded

    pairs = extract_communities_sharded(trainer)
    if trainer.rank != 0:
        return None
    return evaluate_pairs(
        pairs, trainer.graph.num_nodes, trainer.cfg.k, truth,
        device=trainer.state.device,
    )


def write_per_community(path: str, result: dict) -> None:
    """TSV of the per-community matches of both directions."""
    with open(path, "w") as f:
        f.write("side\tcommunity\tsize\tbest_idx\tinter\tf1\tjaccard\n")
        for side, key in (("detected", "per_detected"),
                          ("truth", "per_truth")):
            p = result[key]
            for c in range(len(p["idx"])):
                f.write(
                    f"{side}\t{c}\t{int(p['size'][c])}\t{int(p['idx'][c])}"
                    f"\t{int(p['inter'][c])}\t{p['f1'][c]:.17g}"
                    f"\t{p['jaccard'][c]:.17g}\n"
                )
