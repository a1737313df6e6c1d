#!/usr/bin/env python3
"""Measured cost of the per-community structural scores at bench scale
(profiles/r12_community_scores.md).

The `planted:5000:70:10` graph of profiles/r03_recovery.md, scored for two
covers — the generator's truth and the detected cover of a seed-init bf16
fit — with the timings `python -m bigclam score` does not print: the K10
kernel's device time (HIP events around back-to-back launches), the whole
`community_scores` call on the GPU (uploads, copies, host scores) and the
CPU implementation on the same inputs; plus the launch's tile and the share
of the kernel time one block of the largest community takes.

  python tools/scores_run.py --out-dir out
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
from bigclam.engine.extract import extract_communities_sharded  # noqa: E402
from bigclam.engine.scores import (  # noqa: E402
    community_scores,
    median_degree_floor,
    summary,
)
from bigclam.engine.trainer import Trainer  # noqa: E402
from bigclam.io import Cover, planted_overlap  # noqa: E402
from bigclam.ops.cover_cpu import community_scores_cpu  # noqa: E402


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


def _kernel_ms(args4, dmed, tile, reps, inner):
    """Device time of one K10 launch: HIP events around ``inner``
    back-to-back launches, per launch; median of ``reps`` windows."""
    from bigclam.ops import hip as hip_ops

    def once():
        hip_ops.community_scores(*args4, dmed, tile=tile)

    once()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            once()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return round(statistics.median(ts), 5), [round(t, 5) for t in ts]


def measure(name, g, cover, args):
    from bigclam.ops import hip as hip_ops

    dev = torch.device("cuda")
    dmed = median_degree_floor(g.indptr)
    largest = int(cover.sizes.max())
    tile = min(hip_ops.score_max_tile(), max(1, largest))
    a4 = [torch.from_numpy(a).to(dev) for a in
          (cover.grp_ptr, cover.grp_nodes, g.indptr, g.indices)]
    # the largest community alone: one block
    big = int(cover.sizes.argmax())
    one = Cover.from_members([cover.members(big)], g.num_nodes)
    o4 = [torch.from_numpy(a).to(dev) for a in (one.grp_ptr, one.grp_nodes)]
    o4 += a4[2:]
    k_ms, k_all = _kernel_ms(a4, dmed, tile, args.reps, args.inner)
    one_ms, _ = _kernel_ms(o4, dmed, tile, args.reps, args.inner)
    gpu = community_scores(g, cover, device="cuda")
    cpu = community_scores(g, cover, device="cpu")
    same = all(
        np.array_equal(gpu[k], cpu[k]) and gpu[k].dtype == cpu[k].dtype
        for k in ("int_deg", "vol", "m2", "n_flake", "n_fomd")
    ) and summary(gpu) == summary(cpu)
    call_ms, call_all = _median_ms(
        lambda: community_scores(g, cover, device="cuda"), args.reps, True)
    cpu_call_ms, cpu_call_all = _median_ms(
        lambda: community_scores(g, cover, device="cpu"), args.cpu_reps,
        False)
    cpu_k_ms, cpu_k_all = _median_ms(
        lambda: community_scores_cpu(cover.grp_ptr, cover.grp_nodes,
                                     g.indptr, g.indices, dmed),
        args.cpu_reps, False)
    deg = np.diff(g.indptr)
    rec = {
        "cover": name, "n": g.num_nodes, "nnz": int(len(g.indices)),
        "communities": int(cover.num_comms),
        "non_empty": int((cover.sizes > 0).sum()),
        "memberships": int(cover.num_pairs),
        "membership_tests": int(deg[cover.grp_nodes.astype(np.int64)].sum()),
        "largest_community": largest, "tile": tile,
        "lds_bytes_per_block": max(4 * tile, 96), "dmed": dmed,
        "k10_ms_median": k_ms, "k10_ms_all": k_all,
        "k10_largest_block_alone_ms": one_ms,
        "largest_block_share": round(one_ms / k_ms, 4) if k_ms else None,
        "call_gpu_ms_median": call_ms, "call_gpu_ms_all": call_all,
        "call_cpu_ms_median": cpu_call_ms, "call_cpu_ms_all": cpu_call_all,
        "counts_cpu_ms_median": cpu_k_ms, "counts_cpu_ms_all": cpu_k_all,
        "gpu_equals_cpu": bool(same), "summary": summary(gpu),
    }
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--communities", type=int, default=5000)
    ap.add_argument("--size", type=int, default=70)
    ap.add_argument("--overlap", type=int, default=10)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--max-sweeps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--out-dir", default="out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    os.makedirs(args.out_dir, exist_ok=True)
    g, members = planted_overlap(args.communities, args.size, args.overlap,
                                 0.5, 0, seed=PLANTED_SEED)
    truth = Cover.from_raw_members(members, g.raw_ids)
    recs = [measure("truth", g, truth, args)]
    cfg = BigClamConfig(k=args.k, dtype=args.dtype, device="cuda", seed=7,
                        tol=1e-4, max_sweeps=args.max_sweeps)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cuda"))
    t0 = time.perf_counter()
    res = tr.fit(init="seed")
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    comms, nodes = extract_communities_sharded(tr)
    det = Cover.from_pairs(comms, nodes, g.num_nodes, num_comms=args.k)
    print(json.dumps({"fit_wall_s": round(fit_s, 2), "sweeps": res.sweeps,
                      "converged": res.converged}), flush=True)
    recs.append(dict(measure("detected", g, det, args),
                     fit_wall_s=round(fit_s, 2), sweeps=res.sweeps))
    with open(os.path.join(args.out_dir, "scores_run.json"), "w") as f:
        json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
