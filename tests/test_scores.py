"""Per-community structural scores on the CPU: the vectorised integer
counts against a plain set-based oracle, the fp64 host scores against
hand-computed values, the median-degree floor, the CLI surface and the
sharded ``score_trainer``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import score_fixtures as sfx
from bigclam.config import BigClamConfig
from bigclam.engine.scores import (
    SUMMARY_KEYS,
    community_scores,
    median_degree_floor,
    score_trainer,
    summary,
    write_per_community,
    write_per_member,
)
from bigclam.engine.trainer import Trainer
from bigclam.io import Cover, planted_overlap
from bigclam.ops.cover_cpu import community_scores_cpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("int_deg", "vol", "m2", "n_flake", "n_fomd")
DTYPES = (np.int32, np.int64, np.int64, np.int32, np.int32)


def _assert_oracle(graph, cover, **kw):
    dmed = sfx.dmed_of(graph)
    assert median_degree_floor(graph.indptr) == dmed
    got = community_scores_cpu(
        cover.grp_ptr, cover.grp_nodes, graph.indptr, graph.indices, dmed,
        **kw,
    )
    want = sfx.set_oracle(graph, cover, dmed)
    for name, dt, a, b in zip(NAMES, DTYPES, got, want):
        assert a.dtype == dt, name
        np.testing.assert_array_equal(a, b, err_msg=name)
    return got


# ------------------------------------------------------------ integer counts

@pytest.mark.parametrize("chunk", [1 << 22, 97])
def test_cpu_counts_equal_set_oracle_random(chunk):
    graph = sfx.random_graph(600, 2400, seed=3)
    cover = sfx.random_cover(600, 40, 6, seed=4)
    int_deg, vol, m2, _, _ = _assert_oracle(graph, cover, chunk=chunk)
    assert ((m2 > 0) & (m2 < vol)).any() and int_deg.max() > 1


@pytest.fixture(scope="module")
def edge():
    graph, cover = sfx.edge_fixture()
    return graph, cover, _assert_oracle(graph, cover)


def test_cpu_counts_equal_set_oracle_edge_fixture(edge):
    _assert_oracle(edge[0], edge[1], chunk=64)  # the hub row alone overflows


def test_edge_fixture_is_what_it_claims(edge):
    graph, cover, (int_deg, vol, m2, n_flake, n_fomd) = edge
    deg = np.diff(graph.indptr)
    n = cover.sizes.astype(np.int64)
    assert graph.num_nodes == sfx.EDGE_N == cover.n
    assert n.tolist() == [0, 1, 16, 17, 64, 65, 130, 700, 41, 41, 20, 10, 0,
                          6]
    assert deg[sfx.HUB] == 600
    assert int((cover.grp_nodes == sfx.HUB).sum()) == 5
    for u, d in sfx.DEGREE_NODES.items():
        assert deg[u] == d
    assert all(deg[u] == 0 for u in sfx.ISOLATED)
    np.testing.assert_array_equal(
        cover.members(sfx.C_TWIN_A), cover.members(sfx.C_TWIN_B))
    assert m2[sfx.C_INDEP] == 0 and vol[sfx.C_INDEP] == 20
    # the clique's cut is its overlap node's one outside edge
    assert m2[sfx.C_CLIQUE] == 90 and vol[sfx.C_CLIQUE] - 90 == 1
    # all nodes: every entry is internal
    assert vol[sfx.C_ALL] == m2[sfx.C_ALL] == len(graph.indices)
    # the last community and the last node are non-empty
    assert cover.grp_nodes[-1] == sfx.EDGE_N - 1 and deg[-1] == 3
    assert m2[sfx.C_LAST] == 8 and vol[sfx.C_LAST] == 3 + 2 + 2 + deg[600]
    # not vacuous
    assert ((m2 > 0) & (m2 < vol)).any()
    assert ((n_flake > 0) & (n_flake < n)).any()
    assert ((n_fomd > 0) & (n_fomd < n)).any()


def test_member_ids_outside_the_graph_are_skipped():
    graph = sfx.random_graph(50, 120, seed=1)
    ptr = np.array([0, 4, 6], dtype=np.int64)
    nodes = np.array([-3, 2, 5, 50, 7, 900], dtype=np.int32)
    int_deg, vol, m2, n_flake, n_fomd = community_scores_cpu(
        ptr, nodes, graph.indptr, graph.indices, 0
    )
    deg = np.diff(graph.indptr)
    assert int_deg[0] == int_deg[3] == int_deg[5] == 0
    assert vol.tolist() == [deg[2] + deg[5], deg[7]]
    both = int(5 in graph.neighbors(2).tolist())
    assert m2.tolist() == [2 * both, 0]


# --------------------------------------------------------------- host scores

def _two_triangles():
    """0-1-2 and 2-3-4 share node 2; node 5 is isolated.  nnz = 12, degrees
    2 2 4 2 2 0, median 2."""
    graph = sfx.graph_from_edges(
        6, [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)])
    members = [[0, 1, 2], [2, 3, 4, 5], [5], [0, 1, 2, 3, 4, 5],
               [0, 1, 2, 3, 4], [2], [0, 3], []]
    return graph, Cover.from_members(
        [np.asarray(m, dtype=np.int64) for m in members], 6)


def test_host_scores_hand_computed():
    graph, cover = _two_triangles()
    r = community_scores(graph, cover, device="cpu")
    assert r["dmed"] == 2 and r["nnz"] == 12
    assert r["vol"].tolist() == [8, 8, 0, 12, 12, 4, 4, 0]
    assert r["m2"].tolist() == [6, 6, 0, 12, 12, 0, 0, 0]
    assert r["cut"].tolist() == [2, 2, 0, 0, 0, 4, 4, 0]
    assert r["n_flake"].tolist() == [0, 0, 0, 0, 0, 1, 2, 0]
    assert r["n_fomd"].tolist() == [0, 0, 0, 1, 1, 0, 0, 0]
    assert r["int_deg"].tolist() == [2, 2, 2, 2, 2, 2, 0, 0,
                                     2, 2, 4, 2, 2, 0, 2, 2, 4, 2, 2,
                                     0, 0, 0]
    want = {
        # [0,1,2]; [2,3,4,5]; [5]: vol == 0 and n < 2; all six: vol == nnz
        # and n == N; [0..4]: vol == nnz with n < N; [2]; [0,3]; empty
        "conductance": [2 / 4, 2 / 4, 0.0, 1.0, 1.0, 4 / 4, 4 / 4, 0.0],
        "internal_density": [6 / 6, 6 / 12, 0.0, 12 / 30, 12 / 20, 0.0,
                             0 / 2, 0.0],
        "avg_internal_degree": [6 / 3, 6 / 4, 0.0, 12 / 6, 12 / 5, 0.0, 0.0,
                                0.0],
        "expansion": [2 / 3, 2 / 4, 0.0, 0.0, 0.0, 4 / 1, 4 / 2, 0.0],
        "cut_ratio": [2 / 9, 2 / 8, 0 / 5, 0.0, 0 / 5, 4 / 5, 4 / 8, 0.0],
        "flake_odf": [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0],
        "fomd": [0.0, 0.0, 0.0, 1 / 6, 1 / 5, 0.0, 0.0, 0.0],
    }
    for name, vals in want.items():
        assert r[name].dtype == np.float64
        np.testing.assert_array_equal(r[name], np.array(vals), err_msg=name)
    s = summary(r)
    assert set(s) == set(SUMMARY_KEYS)
    json.dumps(s)
    assert s["n_scored"] == 7 and s["nodes_covered"] == 1.0
    assert s["mean_conductance"] == np.mean(want["conductance"][:7])
    assert s["median_conductance"] == 1.0
    assert s["mean_internal_density"] == np.mean(
        want["internal_density"][:7])
    assert s["mean_flake_odf"] == 2 / 7
    assert s["mean_fomd"] == np.mean(want["fomd"][:7])


def test_nodes_covered_and_empty_cover():
    graph, _ = _two_triangles()
    part = Cover.from_members([np.array([0, 1]), np.array([1, 4])], 6)
    assert community_scores(graph, part, device="cpu")["nodes_covered"] == 0.5
    none = Cover.from_members([], 6)
    r = community_scores(graph, none, device="cpu")
    assert r["n_scored"] == 0 and r["mean_conductance"] == 0.0
    assert len(r["vol"]) == 0 and len(r["int_deg"]) == 0
    with pytest.raises(ValueError):
        community_scores(graph, Cover.from_members([], 7), device="cpu")


def test_dmed_is_the_floor_of_a_half_median():
    # a path of four nodes: degrees 1 2 2 1, median 1.5
    graph = sfx.graph_from_edges(4, [(0, 1), (1, 2), (2, 3)])
    assert np.median(np.diff(graph.indptr)) == 1.5
    assert median_degree_floor(graph.indptr) == 1
    every = Cover.from_members([np.arange(4)], 4)
    r = community_scores(graph, every, device="cpu")
    # int_deg 1 2 2 1: two members above 1.5 — not four (dmed 0), not none
    # (dmed 2)
    assert r["dmed"] == 1 and r["n_fomd"].tolist() == [2]
    odd = sfx.graph_from_edges(5, [(0, 1), (1, 2), (2, 3), (1, 3)])
    assert median_degree_floor(odd.indptr) == 2  # degrees 1 3 2 2 0
    assert median_degree_floor(np.zeros(1, dtype=np.int64)) == 0


def test_writers(tmp_path):
    graph, cover = _two_triangles()
    r = community_scores(graph, cover, device="cpu")
    pc, pm = tmp_path / "pc.tsv", tmp_path / "pm.tsv"
    write_per_community(str(pc), r)
    rows = [l.split("\t") for l in pc.read_text().splitlines()]
    assert rows[0] == ["community", "size", "volume", "internal_edges", "cut",
                       "conductance", "internal_density",
                       "avg_internal_degree", "expansion", "cut_ratio",
                       "flake_odf", "fomd"]
    assert len(rows) == 1 + 8
    assert rows[1][:5] == ["0", "3", "8", "3", "2"]
    assert float(rows[1][8]) == 2 / 3  # %.17g round-trips
    raw = np.arange(6) * 10 + 7
    write_per_member(str(pm), r, cover, raw)
    rows = [l.split("\t") for l in pm.read_text().splitlines()]
    assert rows[0] == ["community", "node", "degree", "internal_degree"]
    assert len(rows) == 1 + cover.num_pairs
    assert rows[3] == ["0", "27", "4", "2"] and rows[7] == ["1", "57", "0", "0"]


# --------------------------------------------------------------------- CLI

def _run(args):
    return subprocess.run(
        [sys.executable, "-m", "bigclam"] + args,
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )


def test_cli_score_planted_truth(tmp_path):
    from bigclam.cli import PLANTED_SEED

    g, truth = planted_overlap(6, 30, 8, 0.5, 0, seed=PLANTED_SEED)
    tf = tmp_path / "truth.cmty.txt"
    tf.write_text(
        "".join(" ".join(str(int(i)) for i in t) + "\n" for t in truth)
    )
    pc, pm = tmp_path / "pc.tsv", tmp_path / "pm.tsv"
    r = _run(["score", str(tf), "planted:6:30:8", "--device", "cpu",
              "--per-community", str(pc), "--per-member", str(pm)])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    res = json.loads(lines[0])
    cover = Cover.from_raw_members(truth, g.raw_ids)
    want = community_scores(g, cover, device="cpu")
    assert {k: res[k] for k in SUMMARY_KEYS} == summary(want)
    assert res["n_scored"] == 6 and res["nodes_dropped"] == 0
    assert 0.0 < res["mean_conductance"] < 1.0
    assert len(pc.read_text().splitlines()) == 1 + 6
    assert len(pm.read_text().splitlines()) == 1 + cover.num_pairs


def test_cli_fit_community_scores(tmp_path):
    tsv, metrics = tmp_path / "cs.tsv", tmp_path / "m.jsonl"
    base = ["fit", "planted:4:16:4", "--k", "4", "--init", "random",
            "--device", "cpu", "--quiet", "--max-sweeps", "3"]
    r = _run(base + ["--community-scores", str(tsv), "--metrics",
                     str(metrics)])
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(res) == {"llh", "sweeps", "converged", "n", "edges",
                        "k"} | set(SUMMARY_KEYS)
    assert 1 <= res["n_scored"] <= 4
    rows = tsv.read_text().splitlines()
    assert rows[0].split("\t")[:3] == ["community", "size", "volume"]
    assert len(rows) == 1 + 4
    logged = [json.loads(l) for l in open(metrics)]
    assert any(l.get("note") == "community_scores" and
               l["mean_conductance"] == res["mean_conductance"]
               for l in logged)
    # without the flag: none of the new keys, the same fit
    r2 = _run(base)
    assert r2.returncode == 0, r2.stderr
    res2 = json.loads(r2.stdout.strip().splitlines()[-1])
    assert set(res2) == {"llh", "sweeps", "converged", "n", "edges", "k"}
    assert res2 == {k: res[k] for k in res2}


# ------------------------------------------------------------- distributed

K_DIST = 6


def _dist_fixture():
    g, truth = planted_overlap(K_DIST, 30, 8, 0.5, 0, seed=11)
    return g, Cover.from_raw_members(truth, g.raw_ids)


def _set_F(tr, tc):
    """The truth's indicator matrix, minus community 4 (left empty), as
    the model: the same global F at every world size."""
    F = np.zeros((tr.graph.num_nodes, K_DIST), dtype=np.float32)
    F[tc.grp_nodes, tc.comms] = 1.0
    F[:, 4] = 0.0
    tr.state.set_local_F(torch.from_numpy(F[tr.shard.start:tr.shard.stop]))


def _worker_score(rank, world_size, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world_size)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        g, tc = _dist_fixture()
        cfg = BigClamConfig(k=K_DIST, device="cpu")
        tr = Trainer(g, cfg, device=torch.device("cpu"))
        _set_F(tr, tc)
        res = score_trainer(tr)
        if rank == 0:
            np.savez(os.path.join(out_dir, "rank0.npz"),
                     **{k: res[k] for k in NAMES + ("conductance", "size")})
            with open(os.path.join(out_dir, "rank0.json"), "w") as f:
                json.dump(summary(res), f)
        else:
            with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
                json.dump({"is_none": res is None}, f)
    finally:
        dist.destroy_process_group()


def test_score_trainer_gloo_ws2_equals_ws1(tmp_path):
    g, tc = _dist_fixture()
    cfg = BigClamConfig(k=K_DIST, device="cpu")
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cpu"))
    _set_F(tr, tc)
    one = score_trainer(tr)
    assert one["size"][4] == 0 and one["n_scored"] == K_DIST - 1
    assert one["m2"].sum() > 0
    mp.spawn(_worker_score, args=(2, 29763, str(tmp_path)), nprocs=2,
             join=True)
    two = np.load(tmp_path / "rank0.npz")
    for k in NAMES + ("conductance", "size"):
        assert two[k].dtype == one[k].dtype
        np.testing.assert_array_equal(two[k], one[k], err_msg=k)
    assert json.load(open(tmp_path / "rank0.json")) == summary(one)
    assert json.load(open(tmp_path / "rank1.json")) == {"is_none": True}
