"""K8 (k8_cover_match) on the GPU: bitwise agreement with the CPU
implementation on (best_idx, best_inter) — the selection is integer-exact,
so there is no tolerance — across the single- and multi-tile paths, the
edge shapes, the end-to-end fit evaluation and the wrapper's validation."""
import numpy as np
import pytest
import torch

from bigclam.config import BigClamConfig
from bigclam.engine.evaluate import (
    best_match,
    evaluate_covers,
    evaluate_trainer,
)
from bigclam.engine.trainer import Trainer
from bigclam.io import Cover, planted_overlap

pytestmark = pytest.mark.gpu

N = 3000


def _random_pairs(rng, nodes, ids, max_mem):
    """Each of ``nodes`` joins 0..max_mem distinct communities of ``ids``."""
    comms, who = [], []
    for u in nodes:
        k = min(int(rng.integers(0, max_mem + 1)), len(ids))
        comms.extend(rng.choice(ids, size=k, replace=False).tolist())
        who.extend([u] * k)
    return comms, who


def _both(x, y, tile):
    cpu = best_match(x, y, device="cpu")
    gpu = best_match(x, y, device="cuda", tile=tile)
    return cpu, gpu


def _assert_same(cpu, gpu, what):
    np.testing.assert_array_equal(gpu[0], cpu[0], err_msg=f"{what}: idx")
    np.testing.assert_array_equal(gpu[1], cpu[1], err_msg=f"{what}: inter")
    assert gpu[0].dtype == np.int32 and gpu[1].dtype == np.int32


@pytest.fixture(scope="module")
def random_covers():
    rng = np.random.default_rng(2024)
    cx, ux = _random_pairs(rng, range(N), np.arange(37), 6)
    cy, uy = _random_pairs(rng, range(N), np.arange(200), 6)
    return (Cover.from_pairs(cx, ux, N, num_comms=37),
            Cover.from_pairs(cy, uy, N, num_comms=200))


@pytest.mark.parametrize("tile", [64, None], ids=["tile64", "default-tile"])
def test_random_covers_both_directions(random_covers, tile):
    x, y = random_covers
    # x -> y: Gy = 200 is four tiles of 64; y -> x: Gy = 37 is one
    cpu, gpu = _both(x, y, tile)
    assert (cpu[0] >= 0).any()
    _assert_same(cpu, gpu, "x->y")
    cpu, gpu = _both(y, x, tile)
    _assert_same(cpu, gpu, "y->x")


def test_more_communities_than_the_compiled_tile(random_covers):
    """Gy = 16384 + 37 at the DEFAULT tile: the tile loop runs twice with
    the full 64 KB histogram, and the winners sit on both sides of the
    tile boundary (ids 16380.. straddle it)."""
    x, _ = random_covers
    rng = np.random.default_rng(99)
    gy = 16384 + 37
    cy, uy = _random_pairs(rng, range(N), np.arange(16380, gy), 4)
    c2, u2 = _random_pairs(rng, range(0, N, 3), np.arange(0, 16380), 2)
    y = Cover.from_pairs(cy + c2, uy + u2, N, num_comms=gy)
    cpu, gpu = _both(x, y, None)
    assert (cpu[0] >= 16384).any() and ((cpu[0] >= 0) & (cpu[0] < 16384)).any()
    _assert_same(cpu, gpu, "x->y two default tiles")
    cpu, gpu = _both(y, x, None)  # 16421 blocks, most of them empty
    _assert_same(cpu, gpu, "y->x")


def _edge_covers():
    """Gy = 65 Y-communities; run at tile 16 / 64 (Gy = tile+1) / 65
    (Gy = tile) / default."""
    rng = np.random.default_rng(7)
    yc, yu = [], []

    def add_y(c, nodes):
        yc.extend([c] * len(nodes))
        yu.extend(list(nodes))

    add_y(1, range(20, 40))  # Y1 == Y2: a tie inside one tile
    add_y(2, range(20, 40))
    add_y(5, range(100, 120))  # Y5 == Y64: the tie spans first/last tile
    add_y(64, range(100, 120))
    add_y(3, range(300, 340))  # superset of Y50: overlaps but scores lower
    add_y(50, range(300, 330))  # strict winner in a later tile than Y3
    special = {1, 2, 3, 5, 50, 64}
    rest = np.array([c for c in range(65) if c not in special])
    c, u = _random_pairs(rng, range(400, 2900), rest, 6)
    yc += c
    yu += u  # nodes 2900.. keep zero Y-memberships
    y = Cover.from_pairs(yc, yu, N, num_comms=65)
    xs = [
        np.arange(0, 2000),  # 2000 members: many more than threads
        np.empty(0, dtype=np.int64),  # empty X-community
        np.arange(2900, 2950),  # members without any Y-membership
        np.arange(20, 40),  # tie Y1/Y2 -> 1
        np.arange(100, 120),  # cross-tile tie Y5/Y64 -> 5
        np.arange(300, 330),  # Y50 beats Y3
        np.arange(2890, 2910),  # mixes nodes with and without memberships
    ]
    return Cover.from_members(xs, N), y


@pytest.mark.parametrize("tile", [16, 64, 65, None])
def test_edge_shapes(tile):
    x, y = _edge_covers()
    cpu, gpu = _both(x, y, tile)
    _assert_same(cpu, gpu, "edge x->y")
    idx, inter = gpu
    assert idx[1] == -1 and inter[1] == 0  # empty
    assert idx[2] == -1 and inter[2] == 0  # no overlap
    assert idx[3] == 1 and inter[3] == 20  # in-tile tie -> lower index
    assert idx[4] == 5 and inter[4] == 20  # cross-tile tie -> lower index
    assert idx[5] == 50 and inter[5] == 30  # strict winner in a later tile
    assert idx[0] >= 0 and inter[0] > 0
    # roles swapped: 65 blocks against a 7-community Y side
    cpu, gpu = _both(y, x, tile)
    _assert_same(cpu, gpu, "edge y->x")
    # Gy = 1
    one = Cover.from_members([np.arange(0, 100)], N)
    cpu, gpu = _both(x, one, tile)
    _assert_same(cpu, gpu, "Gy=1")
    assert gpu[0][0] == 0 and gpu[1][0] == 100 and gpu[0][2] == -1


def test_fit_evaluation_device_equals_cpu():
    g, truth = planted_overlap(8, 24, 6, 0.5, 0, seed=11)
    tc = Cover.from_raw_members(truth, g.raw_ids)
    cfg = BigClamConfig(k=8, device="cuda", seed=3, max_sweeps=40)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cuda"))
    assert tr.state.use_hip
    tr.fit(init="random")
    res = evaluate_trainer(tr, tc)
    from bigclam.engine.extract import extract_communities_sharded

    comms, nodes = extract_communities_sharded(tr)
    det = Cover.from_pairs(comms, nodes, g.num_nodes, num_comms=8)
    ref = evaluate_covers(det, tc, device="cpu")
    for side in ("per_detected", "per_truth"):
        for key in ("idx", "inter"):
            np.testing.assert_array_equal(res[side][key], ref[side][key])
    assert abs(res["avg_f1"] - ref["avg_f1"]) <= 1e-12
    assert abs(res["avg_jaccard"] - ref["avg_jaccard"]) <= 1e-12
    assert res["n_truth"] == 8 and res["avg_f1"] > 0.0


def test_wrapper_validation(random_covers):
    from bigclam.ops import hip as hip_ops

    x, y = random_covers
    dev = torch.device("cuda")
    a = [torch.from_numpy(t).to(dev) for t in
         (x.grp_ptr, x.grp_nodes, y.node_ptr, y.node_comm, y.sizes)]
    max_tile = hip_ops.cover_max_tile()
    assert max_tile == 16384
    for bad in (0, -1, max_tile + 1):
        with pytest.raises(RuntimeError, match="tile"):
            hip_ops.cover_best_match(*a, tile=bad)
    with pytest.raises(RuntimeError, match="dtype"):
        hip_ops.cover_best_match(a[0], a[1].long(), a[2], a[3], a[4])
    with pytest.raises(RuntimeError, match="dtype"):
        hip_ops.cover_best_match(a[0].int(), a[1], a[2], a[3], a[4])
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_ops.cover_best_match(a[0], a[1], a[2], a[3][::2], a[4])
    with pytest.raises(RuntimeError, match="GPU"):
        hip_ops.cover_best_match(a[0], a[1], a[2], a[3].cpu(), a[4])
    # the largest allowed tile still launches and agrees
    idx, inter = hip_ops.cover_best_match(*a, tile=max_tile)
    cpu = best_match(x, y, device="cpu")
    np.testing.assert_array_equal(idx.cpu().numpy(), cpu[0])
    np.testing.assert_array_equal(inter.cpu().numpy(), cpu[1])
