#!/usr/bin/env python3
"""How empty the sparse sweep's items are, measured from the device state.

For a state of the headline config prints one JSON line with
  empty_edge_share   edges whose neighbour has an empty support list
  bound0_share       local nodes with routing bound 0 (nothing staged, no
                     own support)
  wave_idle_share    wave-class nodes that commit nothing (step <= 0 or an
                     empty active set) in the sweep just computed
at three kinds of state: the benchmark's (random init, after the warm-up
sweeps), the converged state of tools/sparse_prof.py (10 dense sweeps from
the seed init), and sweeps 0..3 of a seed-init fit on the sparse path.

  python tools/empty_shares.py [--k 5000] [--state bench|converged|seed]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bigclam.config import BigClamConfig  # noqa: E402
from bigclam.core.state import ShardState  # noqa: E402
from bigclam.engine.trainer import Trainer  # noqa: E402
from bigclam.io import shaped_graph  # noqa: E402
from bigclam.utils.metrics import MetricsLogger  # noqa: E402


def shares(tr, carry, tag):
    st = tr.state
    n = st.n_local
    pack = carry[2]
    out = {"state": tag, "routed": None}
    if pack is None:
        print(json.dumps(out), flush=True)
        return
    sc = st._sp_scount
    nbr = sc[st._indices64]
    bound, _ = ShardState.sparse_bounds(sc, st.indptr, st._indices64, n)
    order = pack["order"].long()
    nb = int(pack["n_block"])
    wave = order[nb:]
    idle = (pack["best"][wave] <= 0) | (pack["gcount"][nb:] == 0)
    out.update(
        routed=int(order.numel()), n_local=n, n_wave=int(wave.numel()),
        n_pack=int(pack.get("n_pack", 0)),
        f_nnz_frac=float(sc[:n].sum().item()) / (n * tr.cfg.k),
        empty_edge_share=float((nbr == 0).float().mean().item()),
        bound0_share=float((bound[:n] == 0).float().mean().item()),
        wave_idle_share=float(idle.float().mean().item())
        if wave.numel() else None,
        accepted_share=float((pack["best"][order] > 0).float().mean().item()))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--nodes", type=int, default=334863)
    ap.add_argument("--edges", type=int, default=925872)
    ap.add_argument("--state", choices=["bench", "converged", "seed", "all"],
                    default="all")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    g = shaped_graph(args.nodes, args.edges, locality=0.7, seed=42)

    def trainer(**kw):
        cfg = BigClamConfig(k=args.k, dtype=args.dtype, device="cuda", seed=7,
                            **kw)
        return Trainer(g, cfg, rank=0, world_size=1,
                       device=torch.device("cuda"),
                       metrics=MetricsLogger(rank=0, quiet=True))

    if args.state in ("bench", "all"):
        os.environ["BIGCLAM_SPARSE"] = "1"
        tr = trainer(ls_steps=15)
        tr.init_F("random")
        carry, _ = tr.prologue()
        for i in range(7):
            carry, _, _ = tr.pipelined_sweep(carry)
            if i in (1, 6):
                shares(tr, carry, f"bench after {i + 1} sweeps")
        del tr
    if args.state in ("seed", "all"):
        os.environ["BIGCLAM_SPARSE"] = "1"
        tr = trainer()
        tr.init_F("seed")
        carry, _ = tr.prologue()
        shares(tr, carry, "seed-init sweep 0")
        for i in range(1, 4):
            carry, _, _ = tr.pipelined_sweep(carry)
            shares(tr, carry, f"seed-init sweep {i}")
        del tr
    if args.state in ("converged", "all"):
        os.environ["BIGCLAM_SPARSE"] = "0"
        tr = trainer(max_sweeps=10, tol=0.0)
        tr.fit(init="seed")
        os.environ["BIGCLAM_SPARSE"] = "1"
        carry, _ = tr.prologue()
        for _ in range(3):
            carry, _, _ = tr.pipelined_sweep(carry)
        shares(tr, carry, "converged (10 dense sweeps + 3 sparse)")


if __name__ == "__main__":
    main()
