"""Model selection over K (v4 semantics, codes/bigclam4-7.scala:115-266).

Sweeps a geometric K grid (config.k_grid); for each K re-initializes F from
the one-time conductance seed ranking and fits to convergence; stops when
the LLH gain over the previous K flattens: ``(1 - LLH_new/LLH_old) < k_tol``
(no abs — codes/bigclam4-7.scala:259).  Returns the selected K.

Deviations (documented): the reference's ``LLHKold == null`` first-iteration
branch is dead code (always false on a Double) — we use an explicit
first-iteration flag; and we report the converged LLH rather than the
second-to-last sweep's (``SGDFindC`` returns the pre-convergence LLHold,
codes/bigclam4-7.scala:225-243 — a REPL quirk, not a capability).

``select_k(..., holdout=frac)`` replaces that rule with the BigCLAM
paper's: the K with the highest held-out likelihood over an edge hold-out
split (absent upstream; needs no ground truth).  Without ``holdout``
nothing changes.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

from ..config import BigClamConfig, k_grid
from ..io.edgelist import Graph
from ..utils.metrics import MetricsLogger
from .trainer import Trainer


def _select_k_heldout(graph, cfg, ks, metrics, init, frac, seed, neg_ratio,
                      patience) -> dict:
    """The paper's criterion: hold out ``frac`` of the edges once, fit
    every grid K on the remaining graph, return the K with the highest
    held-out likelihood (engine/holdout.py).  Stops after ``patience``
    consecutive grid points that do not beat the best so far
    (``patience=0``: run the whole grid)."""
    import torch

    from .. import comm
    from ..io.holdout import split_edges
    from .holdout import heldout_metrics

    split = split_edges(graph, frac, seed, neg_ratio)
    history = []
    seeds = None
    best_k, best_llh, stale = None, None, 0
    for k in ks:
        tr = Trainer(split.train, dataclasses.replace(cfg, k=k),
                     metrics=metrics)
        if seeds is not None:
            tr._seeds = seeds  # ranked once, on the train graph
        res = tr.fit(init=init)
        seeds = tr._seeds
        hm = heldout_metrics(tr, split)
        # rank 0 holds the figures; every rank needs the stopping decision
        t = torch.zeros(2, dtype=torch.float64, device=tr.state.device)
        if hm is not None:
            auc = hm["heldout_auc"]
            t[0] = hm["heldout_llh"]
            t[1] = float("nan") if auc is None else auc
        comm.all_reduce_(t)
        h_llh, h_auc = float(t[0].item()), float(t[1].item())
        rec = {"k": k, "llh": res.llh, "sweeps": res.sweeps,
               "heldout_llh": h_llh,
               "heldout_auc": None if h_auc != h_auc else h_auc}
        history.append(rec)
        metrics.log(dict(rec, select_k=k))
        if best_llh is None or h_llh > best_llh:
            best_k, best_llh, stale = k, h_llh, 0
        else:
            stale += 1
            if patience and stale >= patience:
                break
    return {
        "k": best_k,
        "history": history,
        "grid": ks,
        "criterion": "heldout_llh",
        "heldout_pos": int(len(split.pos)),
        "heldout_neg": int(len(split.neg)),
        "heldout_requested": int(split.requested),
    }


def select_k(
    graph: Graph,
    cfg: BigClamConfig,
    metrics: Optional[MetricsLogger] = None,
    init: str = "seed",
    holdout: Optional[float] = None,
    holdout_seed: int = 0,
    neg_ratio: float = 1.0,
    patience: int = 2,
) -> dict:
    ks = k_grid(cfg.k_min, cfg.k_max, cfg.k_div)
    metrics = metrics or MetricsLogger(quiet=True)
    if holdout is not None:
        return _select_k_heldout(graph, cfg, ks, metrics, init, holdout,
                                 holdout_seed, neg_ratio, patience)
    llh_old = None
    k_for_c = 0
    history = []
    seeds = None
    for k in ks:
        kcfg = dataclasses.replace(cfg, k=k)
        tr = Trainer(graph, kcfg, metrics=metrics)
        if seeds is not None:
            tr._seeds = seeds  # rank the seeds once, reuse per K
        res = tr.fit(init=init)
        seeds = tr._seeds
        llh = res.llh
        history.append({"k": k, "llh": llh, "sweeps": res.sweeps})
        metrics.log({"select_k": k, "llh": llh, "sweeps": res.sweeps})
        k_for_c = k  # if the grid exhausts without flattening, keep the
        # largest K tried (the reference loop simply runs out of grid)
        if llh_old is not None and (1.0 - llh / llh_old) < cfg.k_tol:
            break
        llh_old = llh
    return {"k": k_for_c, "history": history, "grid": ks}
