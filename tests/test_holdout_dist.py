"""Pair scoring against a row-sharded F on CPU (gloo): the scores and the
held-out metrics at world sizes 2 and 3 are bitwise those of world size 1,
and the pair plan is consistent across ranks."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from bigclam.config import BigClamConfig
from bigclam.core.pairs import make_pair_shard, pair_owner
from bigclam.core.shard import partition_bounds
from bigclam.engine.holdout import heldout_metrics, score_pairs
from bigclam.engine.trainer import Trainer
from bigclam.io import planted_partition
from bigclam.io.holdout import HoldoutSplit

K = 5
METRIC_KEYS = ("heldout_llh", "heldout_auc", "heldout_pos", "heldout_neg",
               "heldout_requested", "heldout_pos_zero_frac",
               "heldout_neg_zero_frac")


def _graph():
    g, _ = planted_partition(3, 14, p_in=0.5, p_out=0.03, seed=13)
    return g


def _pairs(g):
    """Positives: edges among the first third of the nodes plus a few that
    reach into the last rows; negatives: non-edges from the same rows.  No
    pair has its u in the last quarter of the node range, so the last rank
    owns none at world sizes 2 and 3 (asserted in the plan test)."""
    n = g.num_nodes
    cut = n // 3
    pos = [(u, int(v)) for u in range(cut) for v in g.neighbors(u) if u < v]
    pos += [(u, n - 1 - i) for i, u in enumerate(range(0, cut, 3))
            if (n - 1 - i) in set(g.neighbors(u).tolist())]
    neg = [(u, v) for u in range(0, cut, 2) for v in range(u + 1, n, 5)
           if v not in set(g.neighbors(u).tolist())]
    pos = np.unique(np.array(pos, dtype=np.int64), axis=0)
    neg = np.unique(np.array(neg, dtype=np.int64), axis=0)
    return pos, neg


def _split(g):
    pos, neg = _pairs(g)
    return HoldoutSplit(train=g, pos=pos, neg=neg, neg_weight=37.5,
                        requested=len(pos) + 2)


def _set_F(tr):
    """Dense deterministic F with exact zeros sprinkled in (a fit's F is
    sparse); the same global matrix at every world size."""
    n = tr.graph.num_nodes
    rng = np.random.default_rng(21)
    F = rng.random((n, K)).astype(np.float32) * 1.5
    F[rng.random((n, K)) < 0.4] = 0.0
    tr.state.set_local_F(torch.from_numpy(F[tr.shard.start:tr.shard.stop]))


def _run(tr):
    split = _split(tr.graph)
    x = score_pairs(tr, np.concatenate([split.neg, split.pos]))
    hm = heldout_metrics(tr, split)
    return x, hm


def _single(dtype):
    cfg = BigClamConfig(k=K, device="cpu", dtype=dtype)
    tr = Trainer(_graph(), cfg, rank=0, world_size=1,
                 device=torch.device("cpu"))
    _set_F(tr)
    return _run(tr)


def _worker(rank, world_size, port, out_dir, dtype):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world_size)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        cfg = BigClamConfig(k=K, device="cpu", dtype=dtype)
        tr = Trainer(_graph(), cfg, device=torch.device("cpu"))
        _set_F(tr)
        F_before = tr.state.F.clone()
        x, hm = _run(tr)
        # the trainer's own buffers are left alone
        assert torch.equal(tr.state.F, F_before)
        if rank == 0:
            np.save(os.path.join(out_dir, "x.npy"), x)
            with open(os.path.join(out_dir, "hm.json"), "w") as f:
                json.dump({k: hm[k] for k in METRIC_KEYS}, f)
        else:
            assert x is None and hm is None
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single():
    return {d: _single(d) for d in ("fp32", "bf16")}


@pytest.mark.parametrize("world_size", [2, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sharded_scores_bitwise_equal_single(single, world_size, dtype,
                                             tmp_path):
    x1, hm1 = single[dtype]
    assert (x1 > 0).any() and (x1 == 0).any()
    port = 29800 + world_size + (10 if dtype == "bf16" else 0)
    mp.spawn(_worker, args=(world_size, port, str(tmp_path), dtype),
             nprocs=world_size, join=True)
    xw = np.load(tmp_path / "x.npy")
    assert xw.dtype == np.float32
    np.testing.assert_array_equal(xw.view(np.uint32), x1.view(np.uint32))
    hmw = json.load(open(tmp_path / "hm.json"))
    for key in METRIC_KEYS:
        assert hmw[key] == hm1[key], key


@pytest.mark.parametrize("world_size", [2, 3, 4])
def test_pair_plan_consistency(world_size):
    g = _graph()
    pos, neg = _pairs(g)
    pairs = np.concatenate([pos, neg])
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    bounds = partition_bounds(g, world_size)
    shards = [make_pair_shard(pairs, bounds, r, world_size)
              for r in range(world_size)]
    # the pair list exercises what it is meant to
    assert any(len(s.sel) == 0 for s in shards), "some rank owns no pair"
    assert any(s.n_extra > 0 for s in shards), "some v is off-shard"
    assert sum(s.plan.total_send for s in shards) == sum(
        s.plan.total_recv for s in shards) > 0
    covered = np.concatenate([s.sel for s in shards])
    np.testing.assert_array_equal(np.sort(covered), np.arange(len(pairs)))
    for s in shards:
        assert s.counts == [len(t.sel) for t in shards]
        assert s.plan.total_recv == s.n_extra
        assert (np.diff(s.extra_globals) > 0).all()  # ascending, distinct
        inside = (s.extra_globals >= s.start) & (s.extra_globals < s.stop)
        assert not inside.any()
        np.testing.assert_array_equal(
            pair_owner(pairs[s.sel, 0], bounds), s.rank)
        # local indices map back to the global pair
        assert s.pu.dtype == np.int32 and s.pv.dtype == np.int32
        assert ((s.pu >= 0) & (s.pu < s.n_own)).all()
        assert ((s.pv >= 0) & (s.pv < s.n_own + s.n_extra)).all()
        np.testing.assert_array_equal(s.pu + s.start, pairs[s.sel, 0])
        back = np.where(
            s.pv < s.n_own, s.pv + s.start,
            s.extra_globals[np.clip(s.pv - s.n_own, 0, None)]
            if s.n_extra else s.pv,
        )
        np.testing.assert_array_equal(back, pairs[s.sel, 1])
        for p, t in enumerate(shards):
            if p == s.rank:
                continue
            # what s sends to p is exactly p's extra rows in s's range
            want = t.extra_globals[
                (t.extra_globals >= s.start) & (t.extra_globals < s.stop)]
            np.testing.assert_array_equal(s.plan.send_idx[p] + s.start, want)
            assert t.plan.recv_counts[s.rank] == len(want)


def test_pair_plan_rejects_bad_pairs():
    bounds = np.array([0, 5, 10])
    with pytest.raises(ValueError):
        make_pair_shard(np.array([[3, 1]]), bounds, 0, 2)
    with pytest.raises(IndexError):
        make_pair_shard(np.array([[3, 10]]), bounds, 0, 2)
    empty = make_pair_shard(np.empty((0, 2), dtype=np.int64), bounds, 1, 2)
    assert len(empty.sel) == 0 and empty.n_extra == 0
    assert empty.plan.total_send == 0 and empty.counts == [0, 0]
