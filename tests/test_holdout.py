"""Held-out edge scoring on CPU: the edge split, the exact AUC, the torch
pair-dot reference, the held-out metrics, held-out select-k and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bigclam.config import BigClamConfig
from bigclam.engine.holdout import (
    heldout_metrics,
    pair_auc,
    score_pairs,
)
from bigclam.engine.model_select import select_k
from bigclam.engine.trainer import Trainer
from bigclam.io import build_graph, planted_overlap
from bigclam.io.holdout import canonical_edges, split_edges
from bigclam.ops import reference as ref_ops

FRAC = 0.2


@pytest.fixture(scope="module")
def graph():
    g, _ = planted_overlap(8, 24, 6, 0.5, 0, seed=11)
    assert g.num_nodes == 150 and g.num_edges == 1114
    return g


def _keys(pairs, n):
    return pairs[:, 0] * n + pairs[:, 1]


# ------------------------------------------------------------------ split
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_split_properties(graph, seed):
    n = graph.num_nodes
    sp = split_edges(graph, FRAC, seed)
    full = _keys(canonical_edges(graph), n)
    train = _keys(canonical_edges(sp.train), n)
    pos = _keys(sp.pos, n)
    neg = _keys(sp.neg, n)
    assert sp.requested == 223 and len(sp.pos) == 223
    assert sp.pos.dtype == np.int64 and sp.neg.dtype == np.int64
    # train ∪ pos = full, disjoint
    assert len(np.intersect1d(train, pos)) == 0
    np.testing.assert_array_equal(np.sort(np.concatenate([train, pos])), full)
    # same node space, nobody isolated, CSR still symmetric
    assert sp.train.num_nodes == n
    np.testing.assert_array_equal(sp.train.raw_ids, graph.raw_ids)
    assert sp.train.degrees().min() >= 1
    assert sp.train.indices.dtype == np.int32
    assert len(sp.train.indices) == 2 * len(train)
    # negatives: u < v, distinct, not edges of the FULL graph
    assert len(sp.neg) == 223
    assert (sp.neg[:, 0] < sp.neg[:, 1]).all()
    assert (sp.pos[:, 0] < sp.pos[:, 1]).all()
    assert len(np.unique(neg)) == len(neg)
    assert len(np.intersect1d(neg, full)) == 0
    assert sp.neg.min() >= 0 and sp.neg.max() < n
    # both lists sorted by (u, v)
    assert (np.diff(pos) > 0).all() and (np.diff(neg) > 0).all()
    assert sp.neg_weight == FRAC * (n * (n - 1) / 2 - graph.num_edges)


def test_split_deterministic_and_seeded(graph):
    a = split_edges(graph, FRAC, 0)
    b = split_edges(graph, FRAC, 0)
    c = split_edges(graph, FRAC, 1)
    np.testing.assert_array_equal(a.pos, b.pos)
    np.testing.assert_array_equal(a.neg, b.neg)
    np.testing.assert_array_equal(a.train.indices, b.train.indices)
    np.testing.assert_array_equal(a.train.indptr, b.train.indptr)
    assert not np.array_equal(a.pos, c.pos)
    assert not np.array_equal(a.neg, c.neg)


def test_split_neg_ratio(graph):
    sp = split_edges(graph, FRAC, 0, neg_ratio=2.5)
    assert len(sp.neg) == round(2.5 * 223)
    assert len(np.unique(_keys(sp.neg, graph.num_nodes))) == len(sp.neg)


def test_split_shortfall_is_not_an_error():
    # a star: every edge has a degree-1 endpoint, nothing can be held out
    star = build_graph(np.array([[0, i] for i in range(1, 9)]))
    sp = split_edges(star, 0.3, 0)
    assert len(sp.pos) == 0 and sp.requested > 0 and len(sp.neg) == 0
    assert sp.train.num_edges == star.num_edges
    # the 3-node path likewise
    p3 = build_graph(np.array([[0, 1], [1, 2]]))
    sp = split_edges(p3, 0.5, 0)
    assert len(sp.pos) == 0 and sp.requested == 1
    # a longer path can lose some interior edges, never the asked-for 90 %
    p10 = build_graph(np.array([[i, i + 1] for i in range(9)]))
    for seed in range(5):
        sp = split_edges(p10, 0.9, seed)
        assert sp.requested == 8 and 0 < len(sp.pos) < 8
        assert sp.train.degrees().min() >= 1
        assert sp.train.num_edges + len(sp.pos) == 9


def test_split_dense_graph_caps_negatives():
    # K5 minus one edge: a single non-edge exists, however many are asked
    e = [[i, j] for i in range(5) for j in range(i + 1, 5) if (i, j) != (1, 3)]
    sp = split_edges(build_graph(np.array(e)), 0.4, 0, neg_ratio=3.0)
    assert len(sp.pos) == 4
    np.testing.assert_array_equal(sp.neg, [[1, 3]])


@pytest.mark.parametrize(
    "frac,neg_ratio", [(0.0, 1.0), (1.0, 1.0), (-0.1, 1.0), (1.5, 1.0),
                       (0.2, 0.0), (0.2, -1.0)])
def test_split_rejects_bad_arguments(graph, frac, neg_ratio):
    with pytest.raises(ValueError):
        split_edges(graph, frac, 0, neg_ratio=neg_ratio)


# -------------------------------------------------------------------- AUC
def _auc_brute(xp, xn):
    d = xp[:, None] - xn[None, :]
    return ((d > 0).sum() + 0.5 * (d == 0).sum()) / (len(xp) * len(xn))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pair_auc_matches_brute_force_under_heavy_ties(seed):
    rng = np.random.default_rng(seed)
    xp = (np.floor(rng.random(301) ** 0.5 * 5) / 4).astype(np.float32)
    xn = (np.floor(rng.random(257) ** 2.0 * 5) / 4).astype(np.float32)
    assert len(np.unique(np.concatenate([xp, xn]))) <= 5
    want = _auc_brute(xp, xn)
    assert 0.5 < want < 1.0
    assert pair_auc(xp, xn) == pytest.approx(want, abs=1e-15)
    # ties are neither wins nor losses
    assert (xp[:, None] == xn[None, :]).mean() > 0.1


def test_pair_auc_edge_cases():
    one = np.ones(7, dtype=np.float32)
    assert pair_auc(one, np.ones(9, dtype=np.float32)) == 0.5
    assert pair_auc(np.zeros(3), np.zeros(4)) == 0.5
    assert pair_auc(one * 2, one) == 1.0
    assert pair_auc(one, one * 2) == 0.0
    assert pair_auc(np.array([1.0, 3.0]), np.array([2.0])) == 0.5
    assert pair_auc(np.empty(0), one) is None
    assert pair_auc(one, np.empty(0)) is None


# ---------------------------------------------------------- ref pair_dot
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_extra", [0, 5])
def test_ref_pair_dot_against_fp64(dtype, n_extra):
    g = torch.Generator().manual_seed(4)
    n_own, kp = 11, 24
    F_own = torch.rand(n_own, kp, generator=g).to(dtype)
    F_extra = torch.rand(n_extra, kp, generator=g).to(dtype)
    n = n_own + n_extra
    pu = torch.randint(0, n, (97,), generator=g)
    pv = torch.randint(0, n, (97,), generator=g)
    pu[:3] = torch.tensor([0, n - 1, n_own - 1])
    pv[:3] = torch.tensor([n - 1, n - 1, n_own - 1])
    if n_extra:
        assert (pu >= n_own).any() and (pu < n_own).any()
    allF = torch.cat([F_own, F_extra]).double()
    want = torch.einsum("pk,pk->p", allF[pu], allF[pv])
    for chunk in (None, 10):  # one chunk / many ragged chunks
        got = ref_ops.pair_dot(F_own, F_extra, pu.int(), pv.int(), chunk=chunk)
        assert got.dtype == torch.float32 and got.shape == (97,)
        np.testing.assert_allclose(got.double(), want, rtol=kp * 2.0 ** -23)
    empty = ref_ops.pair_dot(F_own, F_extra, pu[:0].int(), pv[:0].int())
    assert empty.shape == (0,)
    with pytest.raises(IndexError, match="range"):
        ref_ops.pair_dot(F_own, F_extra, torch.tensor([n]), torch.tensor([0]))
    with pytest.raises(IndexError, match="range"):
        ref_ops.pair_dot(F_own, F_extra, torch.tensor([0]), torch.tensor([-1]))


# -------------------------------------------------------- heldout_metrics
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_heldout_metrics_match_direct_evaluation(graph, dtype):
    sp = split_edges(graph, FRAC, 0)
    cfg = BigClamConfig(k=8, device="cpu", seed=3, dtype=dtype, max_sweeps=25)
    tr = Trainer(sp.train, cfg, rank=0, world_size=1,
                 device=torch.device("cpu"))
    tr.fit(init="random")
    hm = heldout_metrics(tr, sp)
    F = tr.gather_F().double().numpy()
    xp = (F[sp.pos[:, 0]] * F[sp.pos[:, 1]]).sum(-1)
    xn = (F[sp.neg[:, 0]] * F[sp.neg[:, 1]]).sum(-1)
    p = np.clip(np.exp(-xp), cfg.min_p, cfg.max_p)
    want = np.log1p(-p).sum() - sp.neg_weight * xn.mean()
    # the engine finalises fp32 dots (k = 8 terms) in fp64
    assert hm["heldout_llh"] == pytest.approx(want, rel=1e-5)
    assert hm["heldout_pos"] == 223 and hm["heldout_neg"] == 223
    assert hm["heldout_requested"] == 223
    # AUC from the engine's own fp32 scores (fp64 dots could break fp32 ties)
    x = score_pairs(tr, np.concatenate([sp.pos, sp.neg]))
    assert x.dtype == np.float32
    np.testing.assert_allclose(x[:223], xp, rtol=1e-5, atol=1e-30)
    assert hm["heldout_auc"] == pytest.approx(
        _auc_brute(x[:223], x[223:]), abs=1e-12)
    assert hm["heldout_auc"] > 0.7
    assert hm["heldout_neg_zero_frac"] == float((x[223:] == 0).mean())
    assert hm["heldout_pos_zero_frac"] == float((x[:223] == 0).mean())
    # order of the pair list does not matter to the scores
    perm = np.random.default_rng(0).permutation(446)
    pairs = np.concatenate([sp.pos, sp.neg])
    np.testing.assert_array_equal(score_pairs(tr, pairs[perm]), x[perm])


# --------------------------------------------------------------- select_k
@pytest.fixture(scope="module")
def selections(graph):
    cfg = BigClamConfig(device="cpu", seed=3, k_min=2, k_max=8, k_div=1)
    return [
        select_k(graph, cfg, init="random", holdout=FRAC, holdout_seed=s)
        for s in (0, 1, 2)
    ]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_select_k_by_heldout_likelihood(selections, i):
    out = selections[i]
    assert out["grid"] == [2, 8]
    hist = {h["k"]: h for h in out["history"]}
    assert set(hist) == {2, 8}
    print({k: (h["heldout_llh"], h["heldout_auc"]) for k, h in hist.items()})
    assert out["k"] == 8
    assert hist[8]["heldout_llh"] > hist[2]["heldout_llh"]
    assert hist[8]["heldout_auc"] > 0.85
    assert hist[8]["heldout_auc"] > hist[2]["heldout_auc"]
    assert out["heldout_pos"] == 223 and out["heldout_requested"] == 223


def test_select_k_patience(graph):
    """Grid 1,2,4,8 with two-sweep fits: patience=0 walks the whole grid
    and returns its arg-max; patience=1 stops at the first grid point
    that does not beat the best so far, wherever that falls."""
    cfg = BigClamConfig(device="cpu", seed=3, k_min=1, k_max=8, k_div=3,
                        max_sweeps=2)
    full = select_k(graph, cfg, init="random", holdout=FRAC, patience=0)
    assert [h["k"] for h in full["history"]] == full["grid"] == [1, 2, 4, 8]
    best = max(full["history"], key=lambda h: h["heldout_llh"])
    assert full["k"] == best["k"]
    one = select_k(graph, cfg, init="random", holdout=FRAC, patience=1)
    llhs = [h["heldout_llh"] for h in full["history"]]
    stop = next((j for j in range(1, 4) if llhs[j] <= max(llhs[:j])), 3)
    assert [h["k"] for h in one["history"]] == full["grid"][: stop + 1]


def test_select_k_without_holdout_is_unchanged(graph):
    cfg = BigClamConfig(device="cpu", seed=3, k_min=2, k_max=8, k_div=1,
                        max_sweeps=5)
    out = select_k(graph, cfg, init="random")
    assert set(out) == {"k", "history", "grid"}
    assert all(set(h) == {"k", "llh", "sweeps"} for h in out["history"])


# -------------------------------------------------------------------- CLI
def _cli(*args):
    return subprocess.run(
        [sys.executable, "-m", "bigclam", *args],
        capture_output=True, text=True, timeout=300,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    )


def test_cli_fit_holdout(tmp_path):
    met = tmp_path / "m.jsonl"
    out = _cli("fit", "planted:8:24:6", "--k", "8", "--holdout", "0.2",
               "--device", "cpu", "--init", "random", "--max-sweeps", "20",
               "--quiet", "--metrics", str(met), "--truth", "planted",
               "--out", str(tmp_path / "comms.txt"))
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(
        [l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    for key in ("heldout_llh", "heldout_auc", "heldout_pos", "heldout_neg"):
        assert key in rec
    assert rec["heldout_pos"] > 0 and rec["heldout_neg"] == rec["heldout_pos"]
    assert rec["heldout_llh"] < 0 and 0.5 < rec["heldout_auc"] <= 1.0
    assert "avg_f1" in rec and (tmp_path / "comms.txt").exists()
    notes = [json.loads(l) for l in open(met)]
    ev = [r for r in notes if r.get("note") == "heldout_eval"]
    assert len(ev) == 1 and ev[0]["heldout_llh"] == rec["heldout_llh"]
    assert ev[0]["train_edges"] + rec["heldout_pos"] == rec["edges"]


def test_cli_holdout_refuses_resume(tmp_path):
    out = _cli("fit", "planted:8:24:6", "--k", "8", "--holdout", "0.2",
               "--device", "cpu", "--resume", str(tmp_path))
    assert out.returncode != 0
    assert "--holdout cannot be combined with --resume" in out.stderr
