#!/usr/bin/env python3
"""Measured quality and cost of top-n link recommendation at bench scale
(profiles/r13_recommend.md).

The `planted:5000:70:10` graph of profiles/r03_recovery.md with 20 % of its
edges held out, a seed-init bf16 fit at K = 5000 on the rest, then the 10
most likely missing links of every node: recall@10 and hit rate of the
held-out edges, the share of exact rows, the distributions of the candidate
counts and of the candidate bounds T_u, and the timings `python -m bigclam
recommend` does not print — the K11 wrapper's device time (HIP events), the
whole `recommend` call (host clock), the CPU implementation on a fixed
sample of queries and the dense torch formulation (`F[q] @ F.T`, mask,
`topk`) on one batch of queries.

  python tools/recommend_run.py --out-dir out
  python tools/recommend_run.py --kernel-only   # K11 launches only, for a
                                                # kernel trace
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
from bigclam.engine.recommend import (  # noqa: E402
    gather_sparse_model,
    heldout_ranking,
    recommend,
)
from bigclam.engine.trainer import Trainer  # noqa: E402
from bigclam.io import planted_overlap  # noqa: E402
from bigclam.io.holdout import split_edges  # noqa: E402
from bigclam.ops.links_cpu import candidate_bound, topn_links_cpu  # noqa: E402

PCTS = (0, 1, 5, 25, 50, 75, 95, 99, 100)


def _dist(x):
    x = np.asarray(x)
    return {"mean": round(float(x.mean()), 2),
            **{f"p{p}": int(np.percentile(x, p)) for p in PCTS}}


def _event_ms(fn, reps, inner=1):
    """Device time of ``fn``: HIP events around ``inner`` back-to-back
    calls, per call; one warm-up, then the median of ``reps`` windows."""
    fn()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return round(statistics.median(ts), 4), [round(t, 4) for t in ts]


def _host_ms(fn, reps, sync):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), [round(t, 3) for t in ts]


def dense_topk(F32, indptr, indices, qb, n):
    """What a user would write without K11: one dense row block of F·Fᵀ,
    self and neighbours masked, ``topk``."""
    s = F32[qb] @ F32.T
    start = indptr[qb]
    deg = indptr[qb + 1] - start
    rows = torch.repeat_interleave(
        torch.arange(len(qb), device=qb.device), deg)
    first = torch.cumsum(deg, 0) - deg
    offs = torch.arange(len(rows), device=qb.device) - first[rows]
    s[rows, indices[start[rows] + offs].long()] = 0.0
    s[torch.arange(len(qb), device=qb.device), qb] = 0.0
    return torch.topk(s, n, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--communities", type=int, default=5000)
    ap.add_argument("--size", type=int, default=70)
    ap.add_argument("--overlap", type=int, default=10)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--holdout", type=float, default=0.2)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--max-sweeps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--cpu-sample", type=int, default=2000)
    ap.add_argument("--dense-batch", type=int, default=4096)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out-dir", default="out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from bigclam.ops import hip as hip_ops

    dev = torch.device("cuda")
    os.makedirs(args.out_dir, exist_ok=True)
    g, _ = planted_overlap(args.communities, args.size, args.overlap, 0.5, 0,
                           seed=PLANTED_SEED)
    t0 = time.perf_counter()
    split = split_edges(g, args.holdout, 0)
    split_s = time.perf_counter() - t0
    train = split.train
    cfg = BigClamConfig(k=args.k, dtype=args.dtype, device="cuda", seed=7,
                        tol=1e-4, max_sweeps=args.max_sweeps)
    tr = Trainer(train, cfg, rank=0, world_size=1, device=dev)
    t0 = time.perf_counter()
    fit = tr.fit(init="seed")
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    n = args.top
    model = gather_sparse_model(tr)
    indptr = torch.from_numpy(train.indptr).to(dev)
    indices = torch.from_numpy(train.indices).to(dev)
    q_all = torch.arange(g.num_nodes, device=dev, dtype=torch.int32)

    def k11():
        return hip_ops.topn_links(model, indptr, indices, q_all, n)

    if args.kernel_only:
        for _ in range(5):
            k11()
        torch.cuda.synchronize()
        return

    rec = {
        "nodes": g.num_nodes, "edges": g.num_edges,
        "train_edges": train.num_edges, "heldout_edges": int(len(split.pos)),
        "split_s": round(split_s, 2), "k": args.k, "dtype": args.dtype,
        "fit_wall_s": round(fit_s, 2), "sweeps": fit.sweeps,
        "converged": fit.converged, "model_nnz": model.nnz,
        "nnz_per_row": round(model.nnz / g.num_nodes, 3), "top": n,
    }
    res = recommend(train, model, n=n, device=dev)
    rec.update(heldout_ranking(res, split))
    host = model.numpy()
    bound = candidate_bound(host, res["queries"])
    sizes = np.diff(host["col_ptr"])
    rec.update({
        "exact_frac": res["exact_frac"], "work": res["work"],
        "n_lds": res["n_lds"], "n_global": res["n_global"],
        "global_batches": res["global_batches"],
        "n_cand": _dist(res["n_cand"]), "T_u": _dist(bound),
        "queries_without_candidates": int((res["n_cand"] == 0).sum()),
        "column_size": _dist(sizes[sizes > 0]),
        "empty_columns": int((sizes == 0).sum()),
    })
    # a random baseline for the recall: as many random non-neighbours
    rng = np.random.default_rng(0)
    rand = rng.integers(0, g.num_nodes, size=res["top_id"].shape)
    rec["random_recall_at_n"] = heldout_ranking(
        dict(res, top_id=rand.astype(np.int32)), split
    )["heldout_recall_at_n"]
    print(json.dumps(rec), flush=True)

    # timings
    k_ms, k_all = _event_ms(k11, args.reps)
    call_ms, call_all = _host_ms(
        lambda: recommend(train, model, n=n, device=dev), 5, True)
    rec.update({"k11_wrapper_event_ms_median": k_ms,
                "k11_wrapper_event_ms_all": k_all,
                "recommend_call_ms_median": call_ms,
                "recommend_call_ms_all": call_all})
    print(json.dumps({"k11_ms": k_ms, "call_ms": call_ms}), flush=True)

    # CPU implementation on a fixed sample, and equality with the device
    sample = np.sort(np.random.default_rng(1).choice(
        g.num_nodes, size=args.cpu_sample, replace=False)).astype(np.int32)
    t0 = time.perf_counter()
    cpu = topn_links_cpu(host, train.indptr, train.indices, sample, n)
    cpu_s = time.perf_counter() - t0
    same = all(
        np.array_equal(c, res[key][sample]) and c.dtype == res[key].dtype
        for key, c in zip(("top_id", "top_score", "n_cand"), cpu))
    rec.update({"cpu_sample": len(sample), "cpu_sample_s": round(cpu_s, 3),
                "cpu_ms_per_query": round(cpu_s * 1e3 / len(sample), 4),
                "gpu_equals_cpu_on_sample": bool(same)})
    print(json.dumps({"cpu_sample_s": cpu_s, "same": bool(same)}),
          flush=True)

    # the dense torch formulation on one batch
    F32 = tr.state.F_local_k.float().contiguous()
    qb = torch.from_numpy(np.sort(np.random.default_rng(2).choice(
        g.num_nodes, size=args.dense_batch, replace=False))).to(dev)
    d_ms, d_all = _event_ms(
        lambda: dense_topk(F32, indptr, indices, qb, n), 5)
    qb32 = qb.to(torch.int32)
    kb_ms, kb_all = _event_ms(
        lambda: hip_ops.topn_links(model, indptr, indices, qb32, n),
        args.reps)
    vals, ids = dense_topk(F32, indptr, indices, qb, n)
    mine = torch.from_numpy(res["top_id"]).to(dev)[qb].long()
    # a dense top-k row names zero-score nodes where K11 pads
    ids = torch.where(vals > 0, ids, torch.full_like(ids, -1))
    rows_same_set = float(
        (torch.sort(ids, 1).values == torch.sort(mine, 1).values)
        .all(dim=1).float().mean())
    rec.update({"dense_batch": len(qb), "dense_topk_event_ms_median": d_ms,
                "dense_topk_event_ms_all": d_all,
                "k11_same_batch_event_ms_median": kb_ms,
                "k11_same_batch_event_ms_all": kb_all,
                "dense_rows_with_the_same_id_set": round(rows_same_set, 4),
                "dense_flops": 2 * len(qb) * g.num_nodes * args.k})
    print(json.dumps(rec), flush=True)
    with open(os.path.join(args.out_dir, "recommend_run.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
