"""Command-line entry point: ``python -m bigclam <cmd>``.

The reference has no CLI/config surface at all (hard-coded paths and vars,
SURVEY.md §2.15); this exposes the full hyperparameter set with the
reference's defaults.

  fit        fit a K-community model on an edge list, write communities + ckpt
             (--truth FILE|planted adds avg best-match F1/Jaccard;
             --holdout FRAC adds held-out likelihood + link-prediction AUC)
  select-k   model selection over the geometric K grid (v4 semantics;
             --holdout FRAC: the K with the highest held-out likelihood)
  extract    re-extract communities from a checkpoint
  eval       score a detected cover against a ground-truth cover
  score      per-community structural scores of a cover on its graph
             (conductance, density, Flake-ODF, FOMD, ...; no truth needed;
             fit --community-scores OUT.tsv does it for the fitted model)
  recommend  top-N most likely missing links per node from a checkpoint
             (fit --recommend OUT.tsv does it for the fitted model; with
             --holdout it adds recall@N of the held-out edges)
  bench      one timed sweep loop (see also bench.py at the repo root)
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

from .config import BigClamConfig
from . import comm
from .engine.extract import extract_communities, write_communities
from .engine.model_select import select_k
from .engine.trainer import Trainer
from .io import load_graph, rmat_graph
from .utils.metrics import MetricsLogger


def _add_common(p: argparse.ArgumentParser):
    d = BigClamConfig()
    p.add_argument("--k", type=int, default=d.k)
    p.add_argument("--alpha", type=float, default=d.alpha)
    p.add_argument("--beta", type=float, default=d.beta)
    p.add_argument("--ls-steps", type=int, default=d.ls_steps)
    p.add_argument("--tol", type=float, default=d.tol)
    p.add_argument(
        "--max-sweeps", type=int, default=d.max_sweeps,
        help="sweep budget for THIS invocation (with --resume: additional "
        "sweeps on top of the checkpoint's sweep count)",
    )
    p.add_argument("--dtype", choices=["fp32", "bf16"], default=d.dtype)
    p.add_argument("--device", default=None, help="cuda|cpu (auto)")
    p.add_argument("--seed", type=int, default=d.seed)
    p.add_argument("--init", choices=["seed", "random"], default="seed")
    p.add_argument("--seed-rank-compat", action="store_true")
    p.add_argument("--checkpoint-every", type=int, default=0)
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--metrics", default=None, help="JSONL metrics path")
    p.add_argument("--quiet", action="store_true")
    p.add_argument(
        "--holdout", metavar="FRAC", type=float, default=None,
        help="hold out this fraction of the edges (and as many sampled "
        "non-edges), fit on the rest and report held-out likelihood and "
        "link-prediction AUC; with select-k: choose K by held-out "
        "likelihood",
    )
    p.add_argument("--holdout-seed", type=int, default=0)
    p.add_argument(
        "--holdout-neg-ratio", type=float, default=1.0,
        help="sampled non-edges per held-out edge",
    )


def _cfg_from(args) -> BigClamConfig:
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    return BigClamConfig(
        k=args.k,
        alpha=args.alpha,
        beta=args.beta,
        ls_steps=args.ls_steps,
        tol=args.tol,
        max_sweeps=args.max_sweeps,
        dtype=args.dtype,
        device=device,
        seed=args.seed,
        seed_rank_compat=args.seed_rank_compat,
        checkpoint_every=args.checkpoint_every,
        checkpoint_dir=args.checkpoint_dir,
        out=args.out,
        k_min=getattr(args, "k_min", 1000),
        k_max=getattr(args, "k_max", 9000),
        k_div=getattr(args, "k_div", 100),
        k_tol=getattr(args, "k_tol", 1e-3),
    )


PLANTED_SEED = 42  # planted:<...> graphs are the same on every invocation


def _load(args):
    if args.edgelist.startswith("planted:"):
        # planted:<communities>:<size>:<overlap>[:<p_in>:<bg_edges>] —
        # overlapping planted communities (io/synthetic.py
        # planted_overlap); the generator's ground truth is kept for
        # `--truth planted`
        from .io import planted_overlap

        parts = args.edgelist.split(":")[1:]
        if len(parts) not in (3, 5):
            raise SystemExit(
                "planted:<communities>:<size>:<overlap>[:<p_in>:<bg_edges>]"
            )
        p_in = float(parts[3]) if len(parts) == 5 else 0.5
        bg = int(parts[4]) if len(parts) == 5 else 0
        g, truth = planted_overlap(
            int(parts[0]), int(parts[1]), int(parts[2]), p_in, bg,
            seed=PLANTED_SEED,
        )
        args.planted_truth = truth
        return g
    if args.edgelist.startswith("rmat:"):
        # rmat:<scale>:<edge_factor> synthetic graph
        _, scale, ef = args.edgelist.split(":")
        return rmat_graph(int(scale), float(ef))
    if args.edgelist.startswith("shaped:"):
        # shaped:<nodes>:<edges> — power-law graph with exactly that
        # shape (the bench/convergence configs, io/synthetic.py); named
        # presets for the headline shapes:
        #   shaped:amazon = 334863:925872, shaped:enron = 36692:183831,
        #   shaped:youtube = 1134890:2987624
        from .io import shaped_graph

        presets = {
            "amazon": (334863, 925872),
            "enron": (36692, 183831),
            "youtube": (1134890, 2987624),
        }
        parts = args.edgelist.split(":")[1:]
        if len(parts) == 1 and parts[0] in presets:
            n, e = presets[parts[0]]
        else:
            n, e = int(parts[0]), int(parts[1])
        return shaped_graph(n, e, locality=0.7, seed=42)
    return load_graph(args.edgelist)


def _truth_cover(args, g):
    """The --truth cover over g's dense ids (None without --truth)."""
    from .io import Cover, load_cover

    if not getattr(args, "truth", None):
        return None
    if args.truth == "planted":
        members = getattr(args, "planted_truth", None)
        if members is None:
            raise SystemExit("--truth planted needs a planted:<...> graph")
        return Cover.from_raw_members(members, g.raw_ids)
    return load_cover(args.truth, g.raw_ids)


def _cmd_eval(args) -> int:
    from .engine.evaluate import (
        evaluate_covers,
        summary,
        write_per_community,
    )
    from .io import Cover, read_cover_lines

    det = read_cover_lines(args.detected)
    truth = read_cover_lines(args.truth)
    if args.graph:
        raw_ids = _load(argparse.Namespace(edgelist=args.graph)).raw_ids
    else:  # densify over the union of both files' ids
        ids = [m for m in det + truth if len(m)]
        raw_ids = (
            np.unique(np.concatenate(ids)) if ids
            else np.empty(0, dtype=np.int64)
        )
    res = evaluate_covers(
        Cover.from_raw_members(det, raw_ids),
        Cover.from_raw_members(truth, raw_ids),
        device=args.device,
    )
    if args.per_community:
        write_per_community(args.per_community, res)
    print(json.dumps(summary(res)))
    return 0


def _cmd_score(args) -> int:
    from .engine.scores import (
        community_scores,
        summary,
        write_per_community,
        write_per_member,
    )
    from .io import Cover, read_cover_lines

    g = _load(argparse.Namespace(edgelist=args.graph))
    cover = Cover.from_raw_members(read_cover_lines(args.cover), g.raw_ids)
    res = community_scores(g, cover, device=args.device)
    if args.per_community:
        write_per_community(args.per_community, res)
    if args.per_member:
        write_per_member(args.per_member, res, cover, g.raw_ids)
    print(json.dumps(dict(summary(res), nodes_dropped=int(cover.dropped))))
    return 0


def _cmd_recommend(args) -> int:
    from .ckpt.checkpoint import load_full_F
    from .core.sparse_model import SparseModel
    from .engine.recommend import recommend, write_recommendations

    g = _load(argparse.Namespace(edgelist=args.graph))
    F = torch.from_numpy(load_full_F(args.checkpoint_dir))
    if F.shape[0] != g.num_nodes:
        raise SystemExit(
            f"checkpoint has {F.shape[0]} rows, the graph {g.num_nodes} nodes"
        )
    queries, dropped = None, 0
    if args.nodes:
        with open(args.nodes) as f:
            raw = np.array([int(l) for l in f.read().split()], dtype=np.int64)
        at = np.minimum(np.searchsorted(g.raw_ids, raw), g.num_nodes - 1)
        known = g.raw_ids[at] == raw
        dropped = int((~known).sum())
        queries = at[known].astype(np.int32)
    res = recommend(
        g, SparseModel.from_F(F), queries=queries, n=args.top,
        device=args.device, max_community_size=args.max_community_size,
    )
    write_recommendations(args.out, res, g.raw_ids)
    print(json.dumps({
        "queries": int(len(res["queries"])),
        "n": res["n"],
        "exact_frac": res["exact_frac"],
        "work": res["work"],
        "columns_dropped": res["columns_dropped"],
        "nodes_dropped": dropped,
        "mean_n_cand": (
            float(res["n_cand"].mean()) if len(res["n_cand"]) else 0.0
        ),
    }))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(
        prog="bigclam",
        description="BigCLAM overlapping community detection, "
        "MI355X-native (see README.md)",
    )
    sub = ap.add_subparsers(dest="cmd", required=True)

    p_fit = sub.add_parser(
        "fit", help="fit a K-community model on an edge list, "
        "write communities + checkpoint")
    p_fit.add_argument("edgelist")
    _add_common(p_fit)
    p_fit.add_argument(
        "--resume",
        metavar="CKPT_DIR",
        default=None,
        help="resume the fit from a checkpoint directory (any world size)",
    )

    p_fit.add_argument(
        "--truth",
        metavar="FILE|planted",
        default=None,
        help="ground-truth cover file (one community per line); adds the "
        "average best-match F1/Jaccard to the result.  'planted' = the "
        "planted:<...> generator's own truth",
    )

    p_fit.add_argument(
        "--community-scores",
        metavar="OUT.tsv",
        default=None,
        help="write the per-community structural scores of the fitted "
        "communities (conductance, internal density, expansion, cut ratio, "
        "Flake-ODF, FOMD) on the fitted graph and add their summary to the "
        "result",
    )

    p_fit.add_argument(
        "--recommend",
        metavar="OUT.tsv",
        default=None,
        help="write the top-N most likely missing links of every node under "
        "the fitted model (node, candidate, score, prob) on the fitted "
        "graph; with --holdout adds recall@N and hit rate of the held-out "
        "edges to the result",
    )
    p_fit.add_argument("--recommend-top", metavar="N", type=int, default=10)

    p_sel = sub.add_parser(
        "select-k", help="model selection over the geometric K grid "
        "(the reference v4 semantics)")
    p_sel.add_argument("edgelist")
    _add_common(p_sel)
    p_sel.add_argument("--k-min", dest="k_min", type=int, default=1000)
    p_sel.add_argument("--k-max", dest="k_max", type=int, default=9000)
    p_sel.add_argument("--k-div", dest="k_div", type=int, default=100)
    p_sel.add_argument("--k-tol", dest="k_tol", type=float, default=1e-3)
    p_sel.add_argument(
        "--k-patience", dest="k_patience", type=int, default=2,
        help="with --holdout: stop after this many consecutive grid points "
        "without a better held-out likelihood (0 = whole grid)",
    )

    p_ext = sub.add_parser(
        "extract", help="re-extract communities from a checkpoint")
    p_ext.add_argument("checkpoint_dir")
    p_ext.add_argument("edgelist")
    p_ext.add_argument("--out", required=True)

    p_eval = sub.add_parser(
        "eval", help="average best-match F1/Jaccard of a detected cover "
        "against a ground-truth cover")
    p_eval.add_argument("detected", help="cover file (fit --out format)")
    p_eval.add_argument("truth", help="cover file (SNAP cmty format)")
    p_eval.add_argument(
        "--graph", metavar="EDGELIST", default=None,
        help="map ids through this graph (ids not in it are dropped); "
        "default: densify over the union of both files")
    p_eval.add_argument("--device", default=None, help="cuda|cpu (auto)")
    p_eval.add_argument("--per-community", metavar="OUT.tsv", default=None)

    p_score = sub.add_parser(
        "score", help="per-community structural scores of a cover on its "
        "graph: conductance, internal density, expansion, cut ratio, "
        "Flake-ODF, FOMD")
    p_score.add_argument("cover", help="cover file (fit --out or SNAP cmty)")
    p_score.add_argument(
        "graph", help="edge list, or planted:/rmat:/shaped: as for fit")
    p_score.add_argument("--device", default=None, help="cuda|cpu (auto)")
    p_score.add_argument("--per-community", metavar="OUT.tsv", default=None)
    p_score.add_argument("--per-member", metavar="OUT.tsv", default=None)

    p_rec = sub.add_parser(
        "recommend", help="top-N most likely missing links per node from a "
        "checkpoint's model")
    p_rec.add_argument("checkpoint_dir")
    p_rec.add_argument(
        "graph", help="edge list, or planted:/rmat:/shaped: as for fit")
    p_rec.add_argument("--out", required=True, metavar="OUT.tsv")
    p_rec.add_argument("--top", metavar="N", type=int, default=10)
    p_rec.add_argument(
        "--nodes", metavar="FILE", default=None,
        help="raw ids to recommend for, one per line (default: all nodes; "
        "ids not in the graph are dropped and counted)")
    p_rec.add_argument(
        "--max-community-size", metavar="M", type=int, default=None,
        help="ignore communities with more than M members")
    p_rec.add_argument("--device", default=None, help="cuda|cpu (auto)")

    sub.add_parser(
        "bench",
        help="flagship benchmark (forwards to bench.py)",
        add_help=False,
        description="flagship benchmark; all flags forwarded to bench.py",
    )

    if argv is None:
        argv = sys.argv[1:]
    if argv and argv[0] == "bench":
        # delegate to the repo-root bench harness (same contract the
        # scaling driver uses); works installed or from a checkout
        import runpy

        sys.argv = ["bench.py"] + list(argv[1:])
        here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        bench = os.path.join(here, "bench.py")
        if not os.path.exists(bench):  # installed wheel: no repo-root bench.py
            print(
                "bigclam bench requires a repo checkout (bench.py at the "
                "repo root); run it from the source tree",
                file=sys.stderr,
            )
            return 2
        runpy.run_path(bench, run_name="__main__")
        return 0

    args = ap.parse_args(argv)
    if args.cmd == "eval":
        return _cmd_eval(args)
    if args.cmd == "score":
        return _cmd_score(args)
    if args.cmd == "recommend":
        return _cmd_recommend(args)
    holdout = getattr(args, "holdout", None)
    if holdout is not None and getattr(args, "resume", None):
        raise SystemExit(
            "--holdout cannot be combined with --resume: the checkpoint "
            "does not record the edge split it was fitted on"
        )
    rank = comm.init_distributed()

    if args.cmd == "extract":
        from .ckpt.checkpoint import load_full_F, load_meta

        g = _load(args)
        F = torch.from_numpy(load_full_F(args.checkpoint_dir))
        members = extract_communities(F, g.num_edges)
        write_communities(args.out, members, g.raw_ids)
        print(json.dumps({"communities": sum(1 for m in members if len(m))}))
        return 0

    cfg = _cfg_from(args)
    g = _load(args)
    metrics = MetricsLogger(args.metrics, rank=rank, quiet=args.quiet)

    if args.cmd == "select-k":
        out = select_k(
            g, cfg, metrics=metrics, init=args.init, holdout=holdout,
            holdout_seed=args.holdout_seed,
            neg_ratio=args.holdout_neg_ratio, patience=args.k_patience,
        )
        if rank == 0:
            print(json.dumps(out))
        return 0

    split = None
    if holdout is not None:
        # fit on the train graph; it keeps g's node space, so --out and
        # --truth below work unchanged
        import time

        from .io.holdout import split_edges

        t0 = time.perf_counter()
        split = split_edges(
            g, holdout, args.holdout_seed, args.holdout_neg_ratio
        )
        split_s = time.perf_counter() - t0
    tr = Trainer(g if split is None else split.train, cfg, metrics=metrics)
    if getattr(args, "resume", None):
        from .ckpt.checkpoint import resume as ckpt_resume

        sweep0, llh0 = ckpt_resume(args.resume, tr)
        metrics.log({"note": "resumed", "from_sweep": sweep0, "llh": llh0})
        res = tr.fit(skip_init=True, llh_old=llh0, sweep0=sweep0)
    else:
        res = tr.fit(init=args.init)
    if cfg.checkpoint_dir:  # every rank writes its own shard file
        from .ckpt.checkpoint import save_shard_checkpoint

        save_shard_checkpoint(cfg.checkpoint_dir, tr, res.sweeps, res.llh)
    truth = _truth_cover(args, g)
    scores = {}
    cs_path = getattr(args, "community_scores", None)
    if cfg.out or truth is not None or cs_path:
        # sharded K7: per-rank device-side threshold, compacted lists to
        # rank 0 — no N×K gather; one extraction serves
        # both the output file and the ground-truth evaluation
        from .engine.extract import (
            extract_communities_sharded,
            write_membership_pairs,
        )

        pairs = extract_communities_sharded(tr)
        if rank == 0 and cfg.out:
            write_membership_pairs(cfg.out, pairs[0], pairs[1], g.raw_ids)
        if rank == 0 and truth is not None:
            from .engine.evaluate import evaluate_pairs

            ev = evaluate_pairs(
                pairs, g.num_nodes, cfg.k, truth, device=tr.state.device
            )
            scores = {
                key: ev[key]
                for key in ("avg_f1", "avg_jaccard", "n_truth", "n_detected")
            }
            metrics.log(dict(scores, note="truth_eval",
                             truth_nodes_dropped=ev["truth_nodes_dropped"]))
        if rank == 0 and cs_path:
            # scored on the graph the model was fitted on (with --holdout:
            # the train graph)
            from .engine.scores import (
                score_pairs,
                summary as score_summary,
                write_per_community as write_community_scores,
            )

            cs = score_pairs(pairs, tr)
            write_community_scores(cs_path, cs)
            cs_sum = score_summary(cs)
            metrics.log(dict(cs_sum, note="community_scores"))
            scores.update(cs_sum)
    if split is not None:
        from .engine.holdout import heldout_metrics

        hm = heldout_metrics(tr, split)  # collective; dict on rank 0
        if rank == 0:
            metrics.log(dict(hm, note="heldout_eval", split_s=split_s,
                             train_edges=split.train.num_edges))
            scores.update(
                {key: hm[key] for key in ("heldout_llh", "heldout_auc",
                                          "heldout_pos", "heldout_neg")}
            )
    rec_path = getattr(args, "recommend", None)
    if rec_path:
        # on the graph the model was fitted on (with --holdout: the train
        # graph, so held-out edges are legitimate candidates)
        from .engine.recommend import (
            heldout_ranking,
            recommend_trainer,
            write_recommendations,
        )

        rec = recommend_trainer(tr, n=args.recommend_top)  # collective
        if rank == 0:
            write_recommendations(rec_path, rec, g.raw_ids)
            note = {
                "note": "recommend", "n": rec["n"],
                "queries": int(len(rec["queries"])),
                "exact_frac": rec["exact_frac"], "work": rec["work"],
                "mean_n_cand": float(rec["n_cand"].mean()),
            }
            if split is not None:
                hr = heldout_ranking(rec, split)
                note.update(hr)
                scores.update(
                    {key: hr[key] for key in ("heldout_recall_at_n",
                                              "heldout_hit_rate")}
                )
            metrics.log(note)
    if rank == 0:
        print(
            json.dumps(
                dict(
                    {
                        "llh": res.llh,
                        "sweeps": res.sweeps,
                        "converged": res.converged,
                        "n": g.num_nodes,
                        "edges": g.num_edges,
                        "k": cfg.k,
                    },
                    **scores,
                )
            )
        )
    return 0


if __name__ == "__main__":
    sys.exit(main())
