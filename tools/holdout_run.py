#!/usr/bin/env python3
"""Measured held-out evaluation at bench scale (profiles/r04_holdout.md).

What `python -m bigclam fit planted:5000:70:10 --k 5000 --dtype bf16
--holdout 0.2` runs — edge split, fit on the train graph, K9 scoring of the
held-out edges and sampled non-edges, held-out likelihood and AUC — with the
timings the CLI does not print: split and fit wall-clock, the K9 kernel's
device time for the P+Q pairs (device events, one warm-up, median of
several windows of back-to-back launches), the bandwidth that implies
against the 2*(P+Q)*kp*esize bytes the pairs address, and the torch gather
formulation (ops/reference.pair_dot) on the same device tensors.

  python tools/holdout_run.py
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bigclam.cli import PLANTED_SEED  # noqa: E402
from bigclam.config import BigClamConfig  # noqa: E402
from bigclam.core.pairs import fetch_extra_rows, make_pair_shard  # noqa: E402
from bigclam.engine.holdout import heldout_metrics  # noqa: E402
from bigclam.engine.trainer import Trainer  # noqa: E402
from bigclam.io import planted_overlap  # noqa: E402
from bigclam.io.holdout import split_edges  # noqa: E402
from bigclam.ops import hip as hip_ops  # noqa: E402
from bigclam.ops import reference as ref_ops  # noqa: E402


def _event_ms(fn, windows, inner):
    """Median over ``windows`` of (device time of ``inner`` back-to-back
    calls) / inner, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--communities", type=int, default=5000)
    ap.add_argument("--size", type=int, default=70)
    ap.add_argument("--overlap", type=int, default=10)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--init", default="seed")
    ap.add_argument("--holdout", type=float, default=0.2)
    ap.add_argument("--holdout-seed", type=int, default=0)
    ap.add_argument("--max-sweeps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--torch-windows", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")

    t0 = time.perf_counter()
    g, _ = planted_overlap(args.communities, args.size, args.overlap, 0.5, 0,
                           seed=PLANTED_SEED)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    split = split_edges(g, args.holdout, args.holdout_seed)
    split_s = time.perf_counter() - t0

    # the CLI's defaults (BigClamConfig) apart from the arguments above
    cfg = BigClamConfig(k=args.k, dtype=args.dtype, device="cuda",
                        max_sweeps=args.max_sweeps)
    tr = Trainer(split.train, cfg, rank=0, world_size=1, device=dev)
    t0 = time.perf_counter()
    res = tr.fit(init=args.init)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    hm = heldout_metrics(tr, split)
    hm2 = heldout_metrics(tr, split)  # warm: the first call loads code

    # the K9 launch alone, on the tensors score_pairs builds
    pairs = np.concatenate([split.pos, split.neg])
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    ps = make_pair_shard(pairs, tr.bounds, 0, 1)
    st = tr.state
    extra = fetch_extra_rows(st, ps)
    pu = torch.from_numpy(ps.pu).to(dev)
    pv = torch.from_numpy(ps.pv).to(dev)
    F = st.F_local
    k9_ms, k9_all = _event_ms(
        lambda: hip_ops.pair_dot(F, extra, pu, pv), args.windows, args.inner)
    th_ms, th_all = _event_ms(
        lambda: ref_ops.pair_dot(F, extra, pu, pv), args.torch_windows, 1)
    x9 = hip_ops.pair_dot(F, extra, pu, pv)
    xt = ref_ops.pair_dot(F, extra, pu, pv)
    rel = ((x9 - xt).abs() / xt.abs().clamp_min(1e-30)).max().item()
    nbytes = 2 * len(pairs) * st.kp * F.element_size()
    rec = {
        "n": g.num_nodes, "undirected_edges": g.num_edges,
        "graph_build_s": round(build_s, 2), "split_s": round(split_s, 2),
        "train_edges": split.train.num_edges,
        "k": args.k, "kp": st.kp, "dtype": args.dtype, "init": args.init,
        "sweeps": res.sweeps, "converged": res.converged, "llh": res.llh,
        "fit_wall_s": round(fit_s, 2),
        "f_nnz_frac": float((F != 0).float().mean().item()),
        **{key: hm[key] for key in (
            "heldout_llh", "heldout_auc", "heldout_pos", "heldout_neg",
            "heldout_requested", "heldout_pos_zero_frac",
            "heldout_neg_zero_frac")},
        "heldout_eval_first_s": round(hm["heldout_eval_s"], 4),
        "heldout_eval_warm_s": round(hm2["heldout_eval_s"], 4),
        "pairs": len(pairs),
        "k9_ms_median": round(k9_ms, 4), "k9_ms_windows": k9_all,
        "k9_windows_x_inner": [args.windows, args.inner],
        "addressed_bytes": nbytes,
        "k9_implied_TBps": round(nbytes / (k9_ms * 1e-3) / 1e12, 3),
        "torch_ms_median": round(th_ms, 3), "torch_ms_windows": th_all,
        "k9_vs_torch_max_rel_diff": rel,
        "k9_not_slower_than_torch": bool(k9_ms <= th_ms),
    }
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
