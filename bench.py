#!/usr/bin/env python3
"""Flagship benchmark: edges/sec per gradient sweep (BASELINE.json metric).

One "step" = one full synchronous gradient/line-search sweep over every node
(K1 grad+llh -> K2 16-candidate Armijo -> K3 commit + ΔsumF allreduce ->
halo exchange -> K4 full LLH + scalar allreduce) — exactly the reference's
``backtrackingLineSearchs`` unit of work (codes/bigclamv3-7.scala:133-204).

Default config: com-Amazon-shaped synthetic power-law graph (335k nodes /
926k undirected edges — the real dataset is a missing blob upstream),
K=5000, random-init F.  The graph is global and fixed as GPUs are added
(row-sharded) -> strong scaling.  The headline number is bf16 (fp32
accumulation everywhere — grad, sumF, LLH in fp64).

A plain run does only what the headline figure needs: set up, warm up,
time ``--steps`` sweeps, print the JSON result line.  ``--full`` adds the
second-dtype measurement (fp32 storage when the headline is bf16), emitted
alongside in ``variants`` so neither number can be read as a
precision-assisted claim.  ``--dump-outputs DIR`` writes what the last
timed sweep returned (see ``_collect_outputs``) as ``DIR/<name>.npy``;
graph and init are seeded, so two builds run with the same arguments see
identical inputs and can be compared output for output.

Run (driver contract):
  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
  torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from bigclam import comm
from bigclam.config import BigClamConfig
from bigclam.engine.trainer import Trainer
from bigclam.io import shaped_graph
from bigclam.utils.metrics import MetricsLogger


_DUMP_MATRIX_BYTES = 20 << 20  # per sampled [rows, K] fp32 matrix
_DUMP_VECTOR_ELEMS = 1 << 20  # per per-node vector


def _sample(n, max_n):
    """Fixed, seeded, sorted subset of range(n) (all of it when it fits)."""
    if n <= max_n:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(12345)
    return np.sort(rng.choice(n, size=max_n, replace=False)).astype(np.int64)


def _collect_outputs(tr, carry, llh, steps):
    """What the last timed ``pipelined_sweep`` handed back, as host
    float32/float64 arrays (this rank's rows), bounded to well under 64 MB:

      llh          [1]  f64  global objective after the committed step
      steps        [n]  f32  step sizes the sweep committed
      steps_next   [n]  f32  carry: line-search result for the next commit
      grad_rows    [r,K] f32 carry: gradient, on a seeded row sample (rows
                             the sparse kernel handled carry their gradient
                             in compact form and are written as zeros)
      F_rows       [r,K] f32 the model after the commit, same row sample
      sumF         [K]  f32  its column sums
      vector_rows / matrix_rows  f64  the node ids of the sampled entries
    """
    grad, steps_next, pack = carry
    st = tr.state
    n, k = st.n_local, tr.cfg.k
    vrows = _sample(n, _DUMP_VECTOR_ELEMS)
    mrows = _sample(n, max(1, _DUMP_MATRIX_BYTES // (4 * k)))
    vsel = torch.from_numpy(vrows).to(steps.device)
    msel = torch.from_numpy(mrows).to(steps.device)
    g = grad[msel, :k].float()
    if pack is not None:
        routed = torch.zeros(n, dtype=torch.bool, device=g.device)
        routed[pack["order"].long()] = True
        g[routed[msel]] = 0.0
    return {
        "llh": np.asarray([llh], dtype=np.float64),
        "steps": steps[vsel].float().cpu().numpy(),
        "steps_next": steps_next[vsel].float().cpu().numpy(),
        "grad_rows": g.cpu().numpy(),
        "F_rows": st.F_local_k[msel].float().cpu().numpy(),
        "sumF": st.sumF[:k].float().cpu().numpy(),
        "vector_rows": vrows.astype(np.float64),
        "matrix_rows": mrows.astype(np.float64),
    }


def _time_sweeps(graph, dtype, args, rank, world, device, use_cuda,
                 collect=False):
    """Build a trainer at ``dtype`` and time ``args.steps`` pipelined
    sweeps after ``args.warmup`` untimed ones.  Returns (elapsed_s, value,
    ms_per_step, outputs) with elapsed = MAX over ranks; ``outputs`` is
    ``_collect_outputs`` of the last timed sweep when ``collect``."""
    cfg = BigClamConfig(
        k=args.k,
        dtype=dtype,
        device="cuda" if use_cuda else "cpu",
        seed=7,
        ls_steps=args.ls_steps,
    )
    tr = Trainer(
        graph, cfg, device=device, metrics=MetricsLogger(rank=rank, quiet=True)
    )
    tr.init_F("random")

    def sync():
        if use_cuda:
            torch.cuda.synchronize()

    # pipelined loop: each timed step = one full algorithmic sweep
    # (projected commit of the carried Armijo steps -> sumF allreduce ->
    # halo exchange -> fused grad+LLH+16-candidate line-search pass ->
    # scalar LLH allreduce); the post-update LLH comes from the next grad
    # pass (see engine/trainer.py).
    carry, _ = tr.prologue()
    for _ in range(args.warmup):
        carry, _, _ = tr.pipelined_sweep(carry)
    comm.barrier()
    sync()
    t0 = time.perf_counter()
    llh = steps = None
    for _ in range(args.steps):
        carry, llh, steps = tr.pipelined_sweep(carry)
    comm.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    outputs = None
    if collect and steps is not None:
        outputs = _collect_outputs(tr, carry, llh, steps)

    # max over ranks
    el = torch.tensor(
        [elapsed],
        dtype=torch.float64,
        device=device if world > 1 and use_cuda else "cpu",
    )
    if world > 1:
        import torch.distributed as dist

        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    ms_per_step = elapsed / args.steps * 1000.0
    edges_per_sec = graph.num_directed_edges / (elapsed / args.steps)
    del tr
    if use_cuda:
        torch.cuda.empty_cache()
    return elapsed, edges_per_sec, ms_per_step, outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--nodes", type=int, default=334863)  # com-Amazon N
    ap.add_argument("--edges", type=int, default=925872)  # com-Amazon E
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    ap.add_argument("--graph-seed", type=int, default=42)
    ap.add_argument("--locality", type=float, default=0.7)
    ap.add_argument("--ls-steps", type=int, default=15,
                    help="Armijo ladder depth (reference: 15 -> 16 candidates)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (the second-dtype variant)")
    ap.add_argument("--no-variant", action="store_true",
                    help="with --full: skip the second-dtype measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed sweep's outputs as "
                         "DIR/<name>.npy (rank 0's rows)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    rank = comm.init_distributed()
    world = comm.get_world_size()
    use_cuda = torch.cuda.is_available()
    device = torch.device("cuda") if use_cuda else torch.device("cpu")

    graph = shaped_graph(
        args.nodes, args.edges, locality=args.locality, seed=args.graph_seed
    )
    _, value, ms_per_step, outputs = _time_sweeps(
        graph, args.dtype, args, rank, world, device, use_cuda,
        collect=args.dump_outputs is not None,
    )
    if outputs is not None and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in outputs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)
    del outputs
    variants = {}
    if args.full and not args.no_variant:
        other = "fp32" if args.dtype == "bf16" else "bf16"
        try:
            _, v2, ms2, _ = _time_sweeps(
                graph, other, args, rank, world, device, use_cuda
            )
            variants[other] = {"value": v2, "ms_per_step": ms2}
        except Exception as e:  # e.g. K above a dtype's kernel coverage
            variants[other] = {"error": str(e)[:200]}

    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "edges/sec per grad iter",
                    "value": value,
                    "unit": "edges/s",
                    "n_gpus": world,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": ms_per_step,
                    "higher_is_better": True,
                    "scaling": "strong",
                    "vs_baseline": None,  # reference publishes no numbers
                    "dtype": args.dtype,
                    "data": "synthetic",
                    "variants": variants,
                    "config": {
                        "model": "bigclam",
                        "graph": "com-Amazon-shaped synthetic power-law (Chung-Lu)",
                        "nodes": graph.num_nodes,
                        "undirected_edges": graph.num_edges,
                        "directed_edge_visits_per_sweep": graph.num_directed_edges,
                        "k": args.k,
                        "init": "random",
                        "ladder": 16,
                        "sweep": "pipelined (grad+llh fused; post-update LLH = next grad pass)",
                        "parallelism": f"dp{world} row-sharded, RCCL halo",
                    },
                }
            ),
            flush=True,
        )


if __name__ == "__main__":
    main()
