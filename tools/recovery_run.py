#!/usr/bin/env python3
"""Measured ground-truth recovery at bench scale (profiles/r03_recovery.md).

What `python -m bigclam fit planted:5000:70:10 --k 5000 --dtype bf16
--truth planted` runs — overlapping planted communities, fit to tol, K7
extraction, K8 best-match evaluation — with the timings the CLI does not
print: fit wall-clock, the evaluation's device time (one warm-up + median
of several) and the CPU implementation's time on the same covers.

  python tools/recovery_run.py --inits seed,random
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bigclam.cli import PLANTED_SEED  # noqa: E402
from bigclam.config import BigClamConfig  # noqa: E402
from bigclam.engine.evaluate import evaluate_covers  # noqa: E402
from bigclam.engine.extract import extract_communities_sharded  # noqa: E402
from bigclam.engine.trainer import Trainer  # noqa: E402
from bigclam.io import Cover, planted_overlap  # noqa: E402
from bigclam.utils.metrics import MetricsLogger  # noqa: E402


def _median_ms(fn, reps, sync):
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


def _kernel_ms(det, truth, reps):
    """Device time of the two K8 launches alone (HIP events around 100
    back-to-back pairs, per pair)."""
    from bigclam.engine.evaluate import _device_views
    from bigclam.ops import hip as hip_ops

    dev = torch.device("cuda")
    d, t = _device_views(det, dev), _device_views(truth, dev)

    def both():
        hip_ops.cover_best_match(d["grp_ptr"], d["grp_nodes"], t["node_ptr"],
                                 t["node_comm"], t["sizes"])
        hip_ops.cover_best_match(t["grp_ptr"], t["grp_nodes"], d["node_ptr"],
                                 d["node_comm"], d["sizes"])

    both()
    inner = 100  # back-to-back pairs per timed window (sub-ms kernels)
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            both()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return round(statistics.median(ts), 4)


def run(args, init, g, truth):
    cfg = BigClamConfig(k=args.k, dtype=args.dtype, device="cuda", seed=7,
                        tol=1e-4, max_sweeps=args.max_sweeps)
    metrics = MetricsLogger(
        os.path.join(args.out_dir, f"recovery_{init}.jsonl"), rank=0,
        quiet=True,
    )
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cuda"),
                 metrics=metrics)
    t0 = time.perf_counter()
    res = tr.fit(init=init)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    comms, nodes = extract_communities_sharded(tr)
    det = Cover.from_pairs(comms, nodes, g.num_nodes, num_comms=args.k)
    ev = evaluate_covers(det, truth, device="cuda")
    gpu_ms, gpu_all = _median_ms(
        lambda: evaluate_covers(det, truth, device="cuda"), args.reps, True)
    cpu_ms, cpu_all = _median_ms(
        lambda: evaluate_covers(det, truth, device="cpu"), args.cpu_reps,
        False)
    ref = evaluate_covers(det, truth, device="cpu")
    same = all(
        (ev[s][k] == ref[s][k]).all()
        for s in ("per_detected", "per_truth") for k in ("idx", "inter")
    )
    rec = {
        "init": init, "n": g.num_nodes, "undirected_edges": g.num_edges,
        "k": args.k, "dtype": args.dtype, "sweeps": res.sweeps,
        "converged": res.converged, "llh": res.llh,
        "fit_wall_s": round(fit_s, 2),
        "avg_f1": ev["avg_f1"], "avg_jaccard": ev["avg_jaccard"],
        "f1_det_to_truth": ev["f1_det_to_truth"],
        "f1_truth_to_det": ev["f1_truth_to_det"],
        "n_detected": ev["n_detected"], "n_truth": ev["n_truth"],
        "memberships_detected": det.num_pairs,
        "memberships_truth": truth.num_pairs,
        "eval_gpu_ms_median": gpu_ms, "eval_gpu_ms_all": gpu_all,
        "eval_k8_kernels_ms_median": _kernel_ms(det, truth, args.reps),
        "eval_cpu_ms_median": cpu_ms, "eval_cpu_ms_all": cpu_all,
        "gpu_equals_cpu": bool(same),
    }
    print(json.dumps(rec), flush=True)
    del tr
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--communities", type=int, default=5000)
    ap.add_argument("--size", type=int, default=70)
    ap.add_argument("--overlap", type=int, default=10)
    ap.add_argument("--p-in", type=float, default=0.5)
    ap.add_argument("--bg-edges", type=int, default=0)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--inits", default="seed,random")
    ap.add_argument("--max-sweeps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--cpu-reps", type=int, default=7)
    ap.add_argument("--out-dir", default="out")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    os.makedirs(args.out_dir, exist_ok=True)
    t0 = time.perf_counter()
    g, members = planted_overlap(args.communities, args.size, args.overlap,
                                 args.p_in, args.bg_edges, seed=PLANTED_SEED)
    truth = Cover.from_raw_members(members, g.raw_ids)
    print(json.dumps({"graph_build_s": round(time.perf_counter() - t0, 2),
                      "n": g.num_nodes, "undirected_edges": g.num_edges}),
          flush=True)
    for init in args.inits.split(","):
        run(args, init, g, truth)


if __name__ == "__main__":
    main()
