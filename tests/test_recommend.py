"""Top-n link recommendation on the CPU: ``topn_links_cpu`` against an
independent dense oracle (bitwise), the edge fixture's own claims, the
sparse model form, the held-out ranking figures, the TSV writer, the CLI
and a gloo ws=2 run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import link_fixtures as lfx
from bigclam.config import BigClamConfig
from bigclam.core.sparse_model import SparseModel
from bigclam.engine.recommend import (
    heldout_ranking,
    recommend,
    recommend_trainer,
    write_recommendations,
)
from bigclam.engine.trainer import Trainer
from bigclam.io import planted_overlap
from bigclam.io.holdout import HoldoutSplit, split_edges
from bigclam.ops.links_cpu import candidate_bound, topn_links_cpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("top_id", "top_score", "n_cand")
DTYPES = (np.int32, np.float32, np.int32)
TOPS = (1, 10, 64)


def _model(F):
    return SparseModel.from_F(torch.from_numpy(F))


def _assert_same(want, got, what):
    for name, dt, w, g in zip(NAMES, DTYPES, want, got):
        assert g.dtype == dt and w.dtype == dt, f"{what}: {name} dtype"
        assert g.shape == w.shape, f"{what}: {name} shape"
        assert g.tobytes() == w.tobytes(), f"{what}: {name}"


@pytest.fixture(scope="module")
def edge():
    F, graph = lfx.edge_fixture()
    oracle = {n: lfx.dense_oracle(F, graph, lfx.EDGE_QUERIES, n)
              for n in TOPS}
    return F, graph, oracle


@pytest.fixture(scope="module")
def rand():
    F, graph, q = lfx.random_inputs(seed=7)
    return F, graph, q, {n: lfx.dense_oracle(F, graph, q, n) for n in TOPS}


# ------------------------------------------------------------------ oracle

@pytest.mark.parametrize("n", TOPS)
def test_cpu_equals_dense_oracle_edge_fixture(edge, n):
    F, graph, oracle = edge
    got = topn_links_cpu(_model(F), graph.indptr, graph.indices,
                         lfx.EDGE_QUERIES, n)
    _assert_same(oracle[n], got, f"edge n={n}")


@pytest.mark.parametrize("n", TOPS)
def test_cpu_equals_dense_oracle_random_model(rand, n):
    F, graph, q, oracle = rand
    got = topn_links_cpu(_model(F), graph.indptr, graph.indices, q, n)
    _assert_same(oracle[n], got, f"random n={n}")
    assert (oracle[n][2] >= n).any()


def test_edge_fixture_is_what_it_claims(edge):
    """On the oracle's output, so the fixture cannot be vacuous."""
    F, graph, oracle = edge
    n = lfx.EDGE_TOP
    q = lfx.EDGE_QUERIES
    top_id, top_score, n_cand = oracle[n]
    row = {int(u): i for i, u in reversed(list(enumerate(q.tolist())))}
    assert len(q) % 4 and len(q) % 64
    assert (np.diff(q) < 0).any() and (q == lfx.Q_BIG).sum() == 2
    assert not (F < 0).any()
    assert lfx.smallest_product(F) >= 2.0 ** -126
    # (a) a column beyond a wave and beyond a 128-slot table
    assert (F[:, 0] != 0).sum() == lfx.BIG_SIZE > 128
    assert F[lfx.Q_BIG, 0] != 0
    # (b) empty row
    assert not F[lfx.Q_EMPTY].any()
    assert n_cand[row[lfx.Q_EMPTY]] == 0
    assert (top_id[row[lfx.Q_EMPTY]] == -1).all()
    # (c) shares a column, yet every candidate is a neighbour
    mates = np.flatnonzero(F[:, 1])
    assert lfx.Q_ALLNB in mates and len(mates) > 1
    assert n_cand[row[lfx.Q_ALLNB]] == 0
    # (d) n-1, n, n+1 candidates
    assert [int(n_cand[row[u]]) for u in
            (lfx.Q_NM1, lfx.Q_N, lfx.Q_NP1)] == [n - 1, n, n + 1]
    assert top_id[row[lfx.Q_NM1], n - 1] == -1
    assert top_score[row[lfx.Q_NM1], n - 1] == 0
    assert (top_id[row[lfx.Q_N]] >= 0).all()
    # (e) a column whose only member is the query
    assert np.flatnonzero(F[:, 5]).tolist() == [lfx.Q_SELFCOL]
    assert n_cand[row[lfx.Q_SELFCOL]] == 2
    # (f) the order of the fp32 sum is the column order
    cols = np.flatnonzero(F[lfx.Q_ORDER] * F[lfx.C_ORDER])
    prods = (F[lfx.Q_ORDER, cols] * F[lfx.C_ORDER, cols]).tolist()
    assert prods == [2.0 ** 18, 2.0 ** -6, 2.0 ** -6]
    r = row[lfx.Q_ORDER]
    assert top_id[r, 0] == lfx.C_ORDER
    assert top_score[r, 0] == np.float32(2.0 ** 18)
    other = np.float32(2.0 ** -6) + np.float32(2.0 ** -6)
    assert other + np.float32(2.0 ** 18) == np.float32(2.0 ** 18 + 2.0 ** -5)
    assert np.float32(2.0 ** 18 + 2.0 ** -5) != np.float32(2.0 ** 18)
    # (g) at least 12 equal scores straddling place n: lowest ids win
    r = row[lfx.Q_TIE]
    tied = np.flatnonzero(top_score[r] == np.float32(lfx.TIE_SCORE))
    ahead = n - len(tied)
    assert len(lfx.TIE_GROUP) >= 12 and 0 < ahead < n
    assert n_cand[r] == ahead + len(lfx.TIE_GROUP) > n
    assert top_id[r, ahead:].tolist() == list(lfx.TIE_GROUP[:n - ahead])
    assert (np.diff(top_score[r, :ahead + 1]) < 0).all()
    # (h) a column mate that is a CSR neighbour is excluded
    r = row[lfx.Q_BIG]
    nb = graph.neighbors(lfx.Q_BIG)
    assert all(v in nb and F[v, 0] != 0 for v in lfx.NB_IN_COL)
    assert n_cand[r] == lfx.BIG_SIZE - 1 - len(lfx.NB_IN_COL)
    full = oracle[64][0][r]
    assert not np.isin(full, list(nb) + [lfx.Q_BIG]).any()
    # the candidate bound puts queries on both sides of a small LDS table
    t = candidate_bound(_model(F).numpy(), q)
    assert t[row[lfx.Q_BIG]] == lfx.BIG_SIZE and (2 * t <= 64).any()


def test_random_model_products_are_normal():
    for bf16 in (False, True):
        F = lfx.random_model(seed=7, bf16=bf16)
        assert lfx.smallest_product(F) >= 2.0 ** -126
        sizes = (F != 0).sum(axis=0)
        assert 90 < sizes.mean() < 160 and (F != 0).sum(axis=1).max() == 8
    Fb = lfx.random_model(seed=7, bf16=True)
    assert np.array_equal(
        Fb, torch.from_numpy(Fb).to(torch.bfloat16).float().numpy())


# ------------------------------------------------------------- SparseModel

def _triples(ptr, inner, val, by_row):
    outer = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    rows, cols = (outer, inner) if by_row else (inner, outer)
    return sorted(zip(rows.tolist(), cols.tolist(), val.tolist()))


def test_sparse_model_orientations():
    F = lfx.random_model(N=300, K=20, max_row_nnz=5, seed=3)
    m = _model(F).numpy()
    assert m["row_ptr"].dtype == np.int64 and m["col_ptr"].dtype == np.int64
    assert m["row_col"].dtype == np.int32 and m["col_row"].dtype == np.int32
    assert m["row_val"].dtype == np.float32
    assert m["col_val"].dtype == np.float32
    assert len(m["row_ptr"]) == 301 and len(m["col_ptr"]) == 21
    by_row = _triples(m["row_ptr"], m["row_col"], m["row_val"], True)
    by_col = _triples(m["col_ptr"], m["col_row"], m["col_val"], False)
    rr, cc = np.nonzero(F)
    assert by_row == by_col == sorted(
        zip(rr.tolist(), cc.tolist(), F[rr, cc].tolist()))
    for ptr, inner in ((m["row_ptr"], m["row_col"]),
                       (m["col_ptr"], m["col_row"])):
        for a, b in zip(ptr[:-1], ptr[1:]):
            assert (np.diff(inner[a:b]) > 0).all()


def test_sparse_model_ignores_padding_and_upcasts_bf16():
    F = lfx.random_model(N=100, K=12, max_row_nnz=4, seed=5, bf16=True)
    padded = np.concatenate(
        [F, np.full((100, 4), 3.0, dtype=np.float32)], axis=1)
    a = SparseModel.from_F(torch.from_numpy(padded).to(torch.bfloat16), k=12)
    b = _model(F)
    assert a.k == 12 and a.n == 100 and a.nnz == b.nnz == (F != 0).sum()
    for key, x in a.numpy().items():
        assert np.array_equal(x, b.numpy()[key]), key
        assert x.dtype == b.numpy()[key].dtype


def test_sparse_model_drop_columns():
    F = lfx.random_model(N=300, K=20, max_row_nnz=5, seed=3)
    sizes = (F != 0).sum(axis=0)
    m = int(np.sort(sizes)[-4])  # the three largest columns go
    big = sizes > m
    assert 0 < big.sum() < 20
    dropped = _model(F).drop_columns_larger_than(m)
    Fz = F.copy()
    Fz[:, big] = 0
    want = _model(Fz)
    assert dropped.columns_dropped == big.sum() and dropped.k == 20
    for key, x in dropped.numpy().items():
        assert np.array_equal(x, want.numpy()[key]), key
    same = _model(F).drop_columns_larger_than(int(sizes.max()))
    assert same.columns_dropped == 0 and same.nnz == (F != 0).sum()
    # recommend applies it and reports it
    graph = lfx.random_graph(300, 600, seed=4)
    q = np.arange(0, 300, 7, dtype=np.int32)
    res = recommend(graph, _model(F), queries=q, n=5, device="cpu",
                    max_community_size=m)
    assert res["columns_dropped"] == big.sum()
    _assert_same(lfx.dense_oracle(Fz, graph, q, 5),
                 [res[k] for k in NAMES], "dropped columns")


def test_sparse_model_max_nnz():
    F = torch.ones(10, 8)
    with pytest.raises(ValueError, match=r"80 nonzeros.*max_nnz = 79"):
        SparseModel.from_F(F, max_nnz=79)
    assert SparseModel.from_F(F, max_nnz=80).nnz == 80
    assert SparseModel.from_F(F, k=4, max_nnz=40).nnz == 40


# --------------------------------------------------- result dict, ranking

def test_recommend_result_fields(edge):
    F, graph, oracle = edge
    res = recommend(graph, _model(F), queries=lfx.EDGE_QUERIES, n=10,
                    device="cpu")
    _assert_same(oracle[10], [res[k] for k in NAMES], "recommend")
    assert res["prob"].dtype == np.float64
    x = res["top_score"].astype(np.float64)
    assert np.array_equal(res["prob"], -np.expm1(-x))  # 1 - exp(-x)
    np.testing.assert_allclose(res["prob"], 1.0 - np.exp(-x), rtol=0,
                               atol=2.0 ** -52)
    assert (res["prob"][res["top_id"] < 0] == 0).all()
    assert res["n"] == 10 and res["columns_dropped"] == 0
    assert res["exact_frac"] == float((res["n_cand"] >= 10).mean())
    assert 0 < res["exact_frac"] < 1
    assert res["work"] == candidate_bound(
        _model(F).numpy(), lfx.EDGE_QUERIES).sum()
    # default queries: all nodes, in order
    full = recommend(graph, _model(F), n=3, device="cpu")
    assert np.array_equal(full["queries"], np.arange(lfx.EDGE_N))
    with pytest.raises(ValueError):
        recommend(graph, _model(F), queries=[lfx.EDGE_N], device="cpu")


def _hand_result():
    # 6 nodes; held-out edges 0-1, 0-2, 3-4
    top = np.array([[1, 5, -1],    # node 0: hits 1, misses 2
                    [0, 2, 3],     # node 1: hits 0
                    [4, 5, -1],    # node 2: held 0, no hit
                    [5, 1, 4],     # node 3: hits 4
                    [-1, -1, -1],  # node 4: held 3, nothing recommended
                    [0, 1, 2]],    # node 5: no held-out edge
                   dtype=np.int32)
    return {"top_id": top, "queries": np.arange(6, dtype=np.int32), "n": 3}


def test_heldout_ranking_hand_computed():
    train = lfx.graph_from_edges(6, [(0, 5), (1, 5), (2, 3), (4, 5)])
    split = HoldoutSplit(
        train=train, pos=np.array([[0, 1], [0, 2], [3, 4]], dtype=np.int64),
        neg=np.empty((0, 2), dtype=np.int64), neg_weight=1.0, requested=3)
    hr = heldout_ranking(_hand_result(), split)
    # held counts: node0 2, node1 1, node2 1, node3 1, node4 1 = 6; hits 3
    assert hr == {"heldout_recall_at_n": 3 / 6, "heldout_hit_rate": 3 / 5,
                  "heldout_rank_queries": 5, "n": 3}
    # a subset of the nodes, in another order
    res = _hand_result()
    sub = np.array([5, 3, 0])
    res["top_id"], res["queries"] = res["top_id"][sub], res["queries"][sub]
    hr = heldout_ranking(res, split)
    assert hr == {"heldout_recall_at_n": 2 / 3, "heldout_hit_rate": 1.0,
                  "heldout_rank_queries": 2, "n": 3}
    empty = HoldoutSplit(train=train, pos=np.empty((0, 2), dtype=np.int64),
                         neg=np.empty((0, 2), dtype=np.int64),
                         neg_weight=1.0, requested=0)
    assert heldout_ranking(_hand_result(), empty)["heldout_rank_queries"] == 0


def _read_tsv(path):
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert rows[0] == ["node", "candidate", "score", "prob"]
    return rows[1:]


def test_writer_round_trips_raw_ids_and_omits_pads(tmp_path):
    res = _hand_result()
    res["top_score"] = np.where(
        res["top_id"] >= 0, np.float32(0.1) * (res["top_id"] + 1), 0
    ).astype(np.float32)
    res["prob"] = -np.expm1(-res["top_score"].astype(np.float64))
    raw = np.arange(6) * 10 + 7
    path = tmp_path / "r.tsv"
    write_recommendations(str(path), res, raw)
    rows = _read_tsv(path)
    assert len(rows) == int((res["top_id"] >= 0).sum()) == 13
    want = [(int(raw[u]), int(raw[v]))
            for u in range(6) for v in res["top_id"][u] if v >= 0]
    assert [(int(r[0]), int(r[1])) for r in rows] == want
    for r, (u, j) in zip(rows[:2], ((0, 0), (0, 1))):
        assert np.float32(r[2]) == res["top_score"][u, j]
        assert float(r[3]) == res["prob"][u, j]
    assert all(len(r) == 4 for r in rows)


# --------------------------------------------------------------------- CLI

def _run(args):
    return subprocess.run(
        [sys.executable, "-m", "bigclam"] + args,
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )


def _result_from_tsv(path, graph, n):
    """The (queries, top_id) of a written table, over dense ids."""
    rows = _read_tsv(path)
    top = np.full((graph.num_nodes, n), -1, dtype=np.int32)
    fill = np.zeros(graph.num_nodes, dtype=np.int64)
    for r in rows:
        u = int(np.searchsorted(graph.raw_ids, int(r[0])))
        v = int(np.searchsorted(graph.raw_ids, int(r[1])))
        assert graph.raw_ids[u] == int(r[0]) and graph.raw_ids[v] == int(r[1])
        assert float(r[2]) > 0 and 0 < float(r[3]) <= 1
        top[u, fill[u]] = v
        fill[u] += 1
    return {"top_id": top, "n": n,
            "queries": np.arange(graph.num_nodes, dtype=np.int32)}


def test_cli_fit_recommend_then_recommend(tmp_path, capsys):
    from bigclam.cli import PLANTED_SEED, main

    out, out2 = tmp_path / "out.tsv", tmp_path / "out2.tsv"
    ck, metrics = tmp_path / "ck", tmp_path / "m.jsonl"
    r = _run(["fit", "planted:40:24:4", "--k", "40", "--holdout", "0.2",
              "--recommend", str(out), "--recommend-top", "10",
              "--checkpoint-dir", str(ck), "--device", "cpu", "--quiet",
              "--metrics", str(metrics)])
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert {"llh", "sweeps", "heldout_auc", "heldout_recall_at_n",
            "heldout_hit_rate"} <= set(res)
    assert 0.0 < res["heldout_recall_at_n"] <= 1.0
    assert 0.0 < res["heldout_hit_rate"] <= 1.0
    logged = [json.loads(l) for l in open(metrics)]
    note = [l for l in logged if l.get("note") == "recommend"]
    assert len(note) == 1 and note[0]["n"] == 10
    assert note[0]["heldout_recall_at_n"] == res["heldout_recall_at_n"]

    # the table is well-formed and reproduces the reported recall
    g, _ = planted_overlap(40, 24, 4, 0.5, 0, seed=PLANTED_SEED)
    split = split_edges(g, 0.2, 0, 1.0)
    table = _result_from_tsv(out, g, 10)
    assert (table["top_id"] >= 0).any()
    train = split.train
    for u in range(g.num_nodes):  # never self, never a train neighbour
        rec = table["top_id"][u]
        rec = rec[rec >= 0]
        assert u not in rec and len(set(rec.tolist())) == len(rec)
        assert not np.isin(rec, train.neighbors(u)).any()
    hr = heldout_ranking(table, split)
    assert hr["heldout_recall_at_n"] == res["heldout_recall_at_n"]
    assert hr["heldout_hit_rate"] == res["heldout_hit_rate"]

    # an order, not a threshold: better than as many random non-neighbours
    rng = np.random.default_rng(0)
    rand_top = np.full_like(table["top_id"], -1)
    for u in range(g.num_nodes):
        pool = np.setdiff1d(np.arange(g.num_nodes),
                            np.append(train.neighbors(u), u))
        m = int((table["top_id"][u] >= 0).sum())
        rand_top[u, :m] = rng.choice(pool, size=m, replace=False)
    baseline = heldout_ranking(dict(table, top_id=rand_top), split)
    print("recall@10", hr["heldout_recall_at_n"], "random",
          baseline["heldout_recall_at_n"])
    assert hr["heldout_recall_at_n"] > baseline["heldout_recall_at_n"]

    # the stand-alone command on the checkpoint, for a few nodes
    nodes = tmp_path / "nodes.txt"
    ids = [int(g.raw_ids[0]), int(g.raw_ids[17]), int(g.raw_ids.max()) + 5]
    nodes.write_text("".join(f"{i}\n" for i in ids))
    # (in-process: the command neither forks nor joins a process group)
    capsys.readouterr()
    assert main(["recommend", str(ck), "planted:40:24:4", "--out", str(out2),
                 "--device", "cpu", "--nodes", str(nodes), "--top", "5"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    res2 = json.loads(lines[0])
    assert set(res2) == {"queries", "n", "exact_frac", "work",
                         "columns_dropped", "nodes_dropped", "mean_n_cand"}
    assert res2["queries"] == 2 and res2["nodes_dropped"] == 1
    assert res2["n"] == 5 and res2["columns_dropped"] == 0
    rows2 = _read_tsv(out2)
    assert 0 < len(rows2) <= 10
    assert {int(r[0]) for r in rows2} <= set(ids[:2])
    # all nodes by default
    assert main(["recommend", str(ck), "planted:40:24:4", "--out", str(out2),
                 "--device", "cpu"]) == 0
    res3 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res3["queries"] == g.num_nodes and res3["n"] == 10
    assert res3["nodes_dropped"] == 0 and res3["work"] > 0


# ------------------------------------------------------------- distributed

K_DIST = 12


def _dist_graph():
    g, _ = planted_overlap(K_DIST, 30, 8, 0.5, 0, seed=11)
    return g


def _fitted_F(path):
    """A small ws=1 fit; its F is saved so that every world size installs
    the same model."""
    cfg = BigClamConfig(k=K_DIST, device="cpu", max_sweeps=6)
    tr = Trainer(_dist_graph(), cfg, rank=0, world_size=1,
                 device=torch.device("cpu"))
    tr.fit(init="seed")
    np.save(path, tr.state.F_local_k.float().numpy())
    return tr


def _worker_recommend(rank, world_size, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world_size)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        cfg = BigClamConfig(k=K_DIST, device="cpu")
        tr = Trainer(_dist_graph(), cfg, device=torch.device("cpu"))
        F = np.load(os.path.join(out_dir, "F.npy"))
        tr.state.set_local_F(
            torch.from_numpy(F[tr.shard.start:tr.shard.stop]))
        res = recommend_trainer(tr, n=7)
        if rank == 0:
            np.savez(os.path.join(out_dir, "rank0.npz"),
                     **{k: res[k] for k in NAMES + ("prob", "queries")},
                     work=res["work"], exact_frac=res["exact_frac"])
        else:
            assert res is None
    finally:
        dist.destroy_process_group()


def test_recommend_trainer_gloo_ws2_equals_ws1(tmp_path):
    tr = _fitted_F(tmp_path / "F.npy")
    one = recommend_trainer(tr, n=7)
    assert (one["n_cand"] > 0).any() and one["work"] > 0
    # the fit's F is sparse and the recommendations are not trivial
    assert 0 < (np.load(tmp_path / "F.npy") != 0).mean() < 0.6
    mp.spawn(_worker_recommend, args=(2, 29835, str(tmp_path)), nprocs=2,
             join=True)
    two = np.load(tmp_path / "rank0.npz")
    for k in NAMES + ("prob", "queries"):
        assert two[k].dtype == one[k].dtype, k
        assert two[k].tobytes() == one[k].tobytes(), k
    assert int(two["work"]) == one["work"]
    assert float(two["exact_frac"]) == one["exact_frac"]
