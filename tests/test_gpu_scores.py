"""K10 (k10_community_scores) on the GPU: bitwise agreement with the CPU
implementation on all five integer outputs — there is no tolerance in this
feature — across the single- and multi-tile paths, the edge fixture, random
covers, the wrapper's validation and the end-to-end fit scoring."""
import numpy as np
import pytest
import torch

import score_fixtures as sfx
from bigclam.config import BigClamConfig
from bigclam.engine.scores import (
    SCORE_NAMES,
    SUMMARY_KEYS,
    community_scores,
    median_degree_floor,
    score_trainer,
)
from bigclam.engine.trainer import Trainer
from bigclam.io import Cover, planted_overlap
from bigclam.ops.cover_cpu import community_scores_cpu

pytestmark = pytest.mark.gpu

NAMES = ("int_deg", "vol", "m2", "n_flake", "n_fomd")
DTYPES = (np.int32, np.int64, np.int64, np.int32, np.int32)
N = 3000


def _cpu(graph, cover):
    return community_scores_cpu(
        cover.grp_ptr, cover.grp_nodes, graph.indptr, graph.indices,
        median_degree_floor(graph.indptr),
    )


def _device_args(graph, cover):
    dev = torch.device("cuda")
    return [torch.from_numpy(a).to(dev) for a in
            (cover.grp_ptr, cover.grp_nodes, graph.indptr, graph.indices)]


def _gpu(graph, cover, tile):
    from bigclam.ops import hip as hip_ops

    out = hip_ops.community_scores(
        *_device_args(graph, cover), median_degree_floor(graph.indptr),
        tile=tile,
    )
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(cpu, gpu, what):
    for name, dt, c, g in zip(NAMES, DTYPES, cpu, gpu):
        assert g.dtype == dt and c.dtype == dt, f"{what}: {name} dtype"
        np.testing.assert_array_equal(g, c, err_msg=f"{what}: {name}")


@pytest.fixture(scope="module")
def edge():
    graph, cover = sfx.edge_fixture()
    return graph, cover, _cpu(graph, cover)


def test_edge_fixture_sanity(edge):
    """On the CPU result, so the fixture cannot be vacuous."""
    _, cover, (int_deg, vol, m2, n_flake, n_fomd) = edge
    n = cover.sizes.astype(np.int64)
    assert ((m2 > 0) & (m2 < vol)).any()
    assert ((n_flake > 0) & (n_flake < n)).any()
    assert ((n_fomd > 0) & (n_fomd < n)).any()
    assert n[sfx.C_EMPTY] == 0 and n[-1] > 0
    assert cover.grp_nodes[-1] == sfx.EDGE_N - 1


@pytest.mark.parametrize("tile", sfx.EDGE_TILES,
                         ids=["tile16", "tile64", "tile65", "default-tile"])
def test_edge_fixture(edge, tile):
    graph, cover, cpu = edge
    _assert_same(cpu, _gpu(graph, cover, tile), f"edge tile={tile}")


@pytest.fixture(scope="module")
def random_inputs():
    graph = sfx.random_graph(N, 12000, seed=2024)
    # 0..6 memberships per node over 37 communities (sizes ~240), 0..8 over
    # 200 (sizes ~60, the largest above one 64-id tile)
    covers = {g: sfx.random_cover(N, g, mem, seed=g)
              for g, mem in ((37, 6), (200, 8))}
    return graph, {g: (c, _cpu(graph, c)) for g, c in covers.items()}


@pytest.mark.parametrize("tile", [64, None], ids=["tile64", "default-tile"])
@pytest.mark.parametrize("num_comms", [37, 200])
def test_random_covers(random_inputs, num_comms, tile):
    graph, covers = random_inputs
    cover, cpu = covers[num_comms]
    assert cover.sizes.max() > 64  # tile 64 takes more than one pass
    assert ((cpu[2] > 0) & (cpu[2] < cpu[1])).any()
    _assert_same(cpu, _gpu(graph, cover, tile), f"G={num_comms} tile={tile}")


def test_reproducible(random_inputs):
    graph, covers = random_inputs
    cover, _ = covers[200]
    a = _gpu(graph, cover, 64)
    b = _gpu(graph, cover, 64)
    for name, x, y in zip(NAMES, a, b):
        assert x.tobytes() == y.tobytes(), name


def test_member_ids_outside_the_graph_are_skipped():
    from bigclam.ops import hip as hip_ops

    graph = sfx.random_graph(50, 120, seed=1)
    ptr = np.array([0, 4, 6], dtype=np.int64)
    nodes = np.array([-3, 2, 5, 50, 7, 900], dtype=np.int32)
    cpu = community_scores_cpu(ptr, nodes, graph.indptr, graph.indices, 0)
    dev = torch.device("cuda")
    for tile in (1, 3, None):
        out = hip_ops.community_scores(
            *[torch.from_numpy(a).to(dev) for a in
              (ptr, nodes, graph.indptr, graph.indices)], 0, tile=tile)
        _assert_same(cpu, tuple(t.cpu().numpy() for t in out),
                     f"outside ids tile={tile}")


def test_wrapper_validation(edge):
    from bigclam.ops import hip as hip_ops

    graph, cover, cpu = edge
    a = _device_args(graph, cover)
    max_tile = hip_ops.score_max_tile()
    assert max_tile == 16384 == hip_ops.ensure_loaded().SCORE_MAX_TILE
    for bad in (0, max_tile + 1):
        with pytest.raises(RuntimeError, match="tile"):
            hip_ops.community_scores(*a, 3, tile=bad)
    with pytest.raises(RuntimeError, match="dtype"):
        hip_ops.community_scores(a[0], a[1], a[2], a[3].long(), 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_ops.community_scores(a[0], a[1][::2], a[2], a[3], 3)
    with pytest.raises(RuntimeError, match="GPU"):
        hip_ops.community_scores(a[0], a[1], a[2].cpu(), a[3], 3)
    # the largest allowed tile still launches and agrees
    out = hip_ops.community_scores(
        *a, median_degree_floor(graph.indptr), tile=max_tile)
    _assert_same(cpu, tuple(t.cpu().numpy() for t in out), "max tile")


def test_no_communities(edge):
    from bigclam.ops import hip as hip_ops

    graph, _, _ = edge
    none = Cover.from_members([], graph.num_nodes)
    out = hip_ops.community_scores(*_device_args(graph, none), 3)
    for name, dt, t in zip(NAMES, DTYPES, out):
        assert t.is_cuda and t.numel() == 0, name
        assert t.cpu().numpy().dtype == dt, name
    r = community_scores(graph, none, device="cuda")
    assert r["n_scored"] == 0 and len(r["conductance"]) == 0


def test_fit_scores_device_equals_cpu():
    g, truth = planted_overlap(60, 30, 5, 0.5, 0, seed=42)
    cfg = BigClamConfig(k=60, device="cuda", seed=3, max_sweeps=40)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cuda"))
    assert tr.state.use_hip
    tr.fit(init="seed")
    res = score_trainer(tr)
    from bigclam.engine.extract import extract_communities_sharded

    comms, nodes = extract_communities_sharded(tr)
    det = Cover.from_pairs(comms, nodes, g.num_nodes, num_comms=60)
    ref = community_scores(g, det, device="cpu")
    for key in NAMES + ("size", "cut", "deg") + SCORE_NAMES:
        assert res[key].dtype == ref[key].dtype, key
        np.testing.assert_array_equal(res[key], ref[key], err_msg=key)
    for key in SUMMARY_KEYS:
        assert res[key] == ref[key], key
    assert res["n_scored"] > 0 and res["m2"].sum() > 0

    # a sanity order, not a threshold: the planted communities cut fewer
    # edges than random node sets of the same sizes
    tc = Cover.from_raw_members(truth, g.raw_ids)
    rng = np.random.default_rng(0)
    shuffled = Cover.from_members(
        [rng.choice(g.num_nodes, size=int(s), replace=False)
         for s in tc.sizes], g.num_nodes)
    planted = community_scores(g, tc, device="cuda")
    random_sets = community_scores(g, shuffled, device="cuda")
    np.testing.assert_array_equal(planted["size"], random_sets["size"])
    assert planted["mean_conductance"] < random_sets["mean_conductance"]
