"""Held-out pair scoring: likelihood and link-prediction AUC of a fit.

The model says P(edge u-v) = 1 - exp(-F_u·F_v).  ``score_pairs`` computes
``x = F_u·F_v`` for arbitrary pairs (K9 on the GPU, the torch reference on
CPU) against the row-sharded F; ``heldout_metrics`` turns the scores of a
hold-out split (io/holdout.py) into

  heldout_llh = Σ_pos log(1 - p(x))  -  neg_weight · mean_neg(x),
  p(x) = clamp(exp(-x), min_p, max_p),

an unbiased estimate of the paper's held-out pair log-likelihood (every
held-out edge, plus the sampled non-edges scaled up to the
``frac``-share of all non-edges they stand for, each contributing
log exp(-x) = -x), and the exact mid-rank AUC of positives against
negatives.  Both are finalised on rank 0 in fp64 from the fp32 scores, by
the same code on every device.
"""
from __future__ import annotations

import time
from typing import Optional

import numpy as np
import torch

from ..core.pairs import fetch_extra_rows, make_pair_shard
from ..io.holdout import HoldoutSplit
from ..ops import reference as ref_ops


def score_pairs(trainer, pairs: np.ndarray) -> Optional[np.ndarray]:
    """``x[i] = F[u_i]·F[v_i]`` (fp32) for global-id pairs ``[P, 2]`` with
    ``u <= v``, in the order given.  Collective over the trainer's ranks;
    returns the scores on rank 0 and ``None`` elsewhere.

    Internally the pairs are scored sorted by ``(u, v)``: that groups them
    by owner rank, and consecutive K9 waves share row u."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    st = trainer.state
    ps = make_pair_shard(
        pairs[order], trainer.bounds, trainer.rank, trainer.world_size
    )
    extra = fetch_extra_rows(st, ps)
    pu = torch.from_numpy(ps.pu).to(st.device)
    pv = torch.from_numpy(ps.pv).to(st.device)
    if st.use_hip:
        from ..ops import hip as hip_ops

        x = hip_ops.pair_dot(st.F_local, extra, pu, pv)
    else:
        x = ref_ops.pair_dot(st.F_local, extra, pu, pv)

    # (u, v)-sorted pairs are contiguous per owner, in rank order
    if trainer.world_size == 1:
        parts = [x.cpu()]
    else:
        import torch.distributed as dist

        if trainer.rank != 0:
            if x.numel():
                dist.send(x, dst=0)
            return None
        parts = [x.cpu()]
        for r in range(1, trainer.world_size):
            buf = torch.empty(
                ps.counts[r], device=st.device, dtype=torch.float32
            )
            if ps.counts[r]:
                dist.recv(buf, src=r)
            parts.append(buf.cpu())
    out = np.empty(len(pairs), dtype=np.float32)
    out[order] = torch.cat(parts).numpy()
    return out


def pair_auc(x_pos: np.ndarray, x_neg: np.ndarray) -> Optional[float]:
    """Exact mid-rank (Mann-Whitney) AUC: the probability that a positive
    outscores a negative, ties counting one half.  Integer arithmetic —
    2U = Σ_pos (2·#neg below + #neg equal) from one sort and two
    ``searchsorted`` — divided once in fp64.  ``None`` when either side
    is empty."""
    x_pos = np.asarray(x_pos)
    x_neg = np.asarray(x_neg)
    if len(x_pos) == 0 or len(x_neg) == 0:
        return None
    s = np.sort(x_neg)
    below = np.searchsorted(s, x_pos, side="left").astype(np.int64)
    upto = np.searchsorted(s, x_pos, side="right").astype(np.int64)
    two_u = int((below + upto).sum())  # 2·below + (upto - below)
    return two_u / (2.0 * len(x_pos) * len(x_neg))


def metrics_from_scores(x_pos: np.ndarray, x_neg: np.ndarray,
                        neg_weight: float, requested: int, min_p: float,
                        max_p: float) -> dict:
    """The held-out figures from fp32 scores, in fp64."""
    xp = np.asarray(x_pos, dtype=np.float64)
    xn = np.asarray(x_neg, dtype=np.float64)
    p = np.clip(np.exp(-xp), min_p, max_p)
    llh = float(np.log1p(-p).sum())
    if len(xn):
        llh -= float(neg_weight) * float(xn.mean())
    return {
        "heldout_llh": llh,
        "heldout_auc": pair_auc(x_pos, x_neg),
        "heldout_pos": int(len(xp)),
        "heldout_neg": int(len(xn)),
        "heldout_requested": int(requested),
        "heldout_pos_zero_frac": float((xp == 0).mean()) if len(xp) else 0.0,
        "heldout_neg_zero_frac": float((xn == 0).mean()) if len(xn) else 0.0,
    }


def heldout_metrics(trainer, split: HoldoutSplit) -> Optional[dict]:
    """Score ``split``'s positives and negatives under the trainer's
    current F.  Collective; the dict on rank 0, ``None`` elsewhere."""
    t0 = time.perf_counter()
    n_pos = len(split.pos)
    x = score_pairs(trainer, np.concatenate([split.pos, split.neg]))
    if x is None:
        return None
    cfg = trainer.cfg
    out = metrics_from_scores(
        x[:n_pos], x[n_pos:], split.neg_weight, split.requested,
        cfg.min_p, cfg.max_p,
    )
    out["heldout_eval_s"] = time.perf_counter() - t0
    return out
