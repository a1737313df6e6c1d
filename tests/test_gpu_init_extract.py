"""K5 / K6 / K7 on the device against the exact oracles of tests/oracle.py
(docs/kernels.md, "K5 / K6 / K7 contract").  The three kernels produce
integers, exact 0/1 values or one IEEE division of exact integers, so every
comparison in this file is exact equality.
"""
import numpy as np
import pytest
import torch

import contract_fixtures as cf
import oracle
from bigclam.config import BigClamConfig
from bigclam.core.init import conductance_ranking, conductance_ranking_device
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState
from bigclam.engine.trainer import Trainer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
K7_IDS = [cf.k7_id(t) for t in cf.k7_cases()]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _hip():
    from bigclam.ops import hip as hip_ops

    return hip_ops, hip_ops.ensure_loaded()


# ----------------------------------------------------------------------- K7
def _assert_memberships(tag, names, counts, comms, want):
    wc, wm = want
    counts = np.asarray(counts, dtype=np.int64)
    comms = np.asarray(comms)
    if not np.array_equal(counts, wc):
        u = int(np.flatnonzero(counts != wc)[0])
        raise AssertionError(
            f"{tag}: count of row {u} ({names[u]}) is {counts[u]}, "
            f"oracle {wc[u]}")
    if not np.array_equal(comms, wm):
        off = np.concatenate([[0], np.cumsum(wc)])
        i = int(np.flatnonzero(comms != wm)[0])
        u = int(np.searchsorted(off, i, side="right") - 1)
        raise AssertionError(
            f"{tag}: row {u} ({names[u]}) got "
            f"{comms[off[u]:off[u + 1]][:8].tolist()}, oracle "
            f"{wm[off[u]:off[u + 1]][:8].tolist()}")


@pytest.mark.parametrize("t", cf.k7_cases(), ids=K7_IDS)
def test_k7_matches_oracle(t):
    hip_ops, _ = _hip()
    k_true, kp, dtype = t
    F = cf.k7_rows(*t).to(DEV)
    assert F.shape[1] == kp and F.dtype == DTYPES[dtype]
    counts, comms = hip_ops.extract_membership(F, k_true, cf.K7_DELTA)
    assert counts.dtype == torch.int32 and comms.dtype == torch.int32
    _assert_memberships(cf.k7_id(t), cf.k7_row_names(*t), counts.cpu().numpy(),
                        comms.cpu().numpy(), cf.k7_oracle(*t))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_k7_fill_stays_inside_its_rows(dtype):
    """The fill pass at offsets + G into a buffer of total + 2G: both guard
    regions stay untouched, and a second fill is bitwise identical."""
    _, ext = _hip()
    t = (5000, 5000, dtype)
    assert t in cf.k7_cases()
    G = 1024
    F = cf.k7_rows(*t).to(DEV)
    wc, wm = cf.k7_oracle(*t)
    counts = torch.full((F.shape[0],), -7, device=DEV, dtype=torch.int32)
    ext.extract_count(F, 5000, cf.K7_DELTA, counts)
    np.testing.assert_array_equal(counts.cpu().numpy(), wc)
    offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts.long() + G
    total = int(wc.sum())
    runs = []
    for _ in range(2):
        comms = torch.full((total + 2 * G,), -1, device=DEV, dtype=torch.int32)
        ext.extract_fill(F, 5000, cf.K7_DELTA, offsets, comms)
        runs.append(comms.cpu().numpy())
    assert (runs[0][:G] == -1).all() and (runs[0][G + total:] == -1).all()
    np.testing.assert_array_equal(runs[0][G:G + total], wm)
    np.testing.assert_array_equal(runs[1], runs[0])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_k7_edge_shapes(dtype):
    hip_ops, _ = _hip()
    sd = DTYPES[dtype]
    # all-zero F: no membership at all, empty comms, no error
    counts, comms = hip_ops.extract_membership(
        torch.zeros(5, 16, device=DEV, dtype=sd), 13, cf.K7_DELTA)
    assert counts.tolist() == [0] * 5 and comms.numel() == 0
    # no rows
    counts, comms = hip_ops.extract_membership(
        torch.zeros(0, 16, device=DEV, dtype=sd), 13, cf.K7_DELTA)
    assert counts.numel() == 0 and comms.numel() == 0
    # one column (pads poisoned above the threshold)
    F = torch.full((4, 8), 1.0, dtype=sd)
    F[:, 0] = torch.tensor([0.0, 1.0, 0.125, 0.0]).to(sd)
    counts, comms = hip_ops.extract_membership(F.to(DEV), 1, cf.K7_DELTA)
    assert counts.tolist() == [0, 1, 1, 0] and comms.tolist() == [0, 0]


def test_k7_sharded_extraction_matches_gathered_F():
    """extract_communities_sharded == extract_communities(gather_F) at
    K = 300 (two columns per thread) after two sweeps from a random init."""
    from bigclam.engine.extract import (
        extract_communities,
        extract_communities_sharded,
    )
    from bigclam.io import rmat_graph

    g = rmat_graph(9, 6.0)
    cfg = BigClamConfig(k=300, device="cuda", seed=3)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=DEV)
    tr.init_F("random")
    tr.sweep()
    tr.sweep()
    comms, nodes = extract_communities_sharded(tr)
    members = extract_communities(tr.gather_F(), g.num_edges)
    assert len(members) == 300 and len(comms) > 0
    for c in range(300):
        np.testing.assert_array_equal(nodes[comms == c], np.sort(members[c]))


# ----------------------------------------------------------------------- K5
@pytest.fixture(scope="module")
def k5_device_cond():
    """name -> device cond of every K5 graph (one K5 launch per graph)."""
    hip_ops, _ = _hip()
    return {name: hip_ops.conductance_full_graph(g, DEV)
            for name, g in cf.k5_graphs().items()}


@pytest.mark.parametrize("name", list(cf.k5_graphs()))
def test_k5_bitwise_equal_to_integer_oracle(name, k5_device_cond):
    o = cf.k5_oracle(name)
    got = k5_device_cond[name].cpu().numpy()
    assert got.dtype == np.float64
    if not np.array_equal(got, o["cond"]):
        bad = np.flatnonzero(got != o["cond"])[:8]
        rows = [(int(u), int(o["deg"][u]), int(o["z"][u]), int(o["cut"][u]),
                 float(got[u]), float(o["cond"][u])) for u in bad]
        raise AssertionError(
            f"{name}: cond differs on {len(bad)}+ nodes; (node, deg, z, cut, "
            f"device, oracle) = {rows}")


@pytest.mark.parametrize("name", list(cf.k5_graphs()))
def test_k5_device_ranking_matches_host(name, k5_device_cond):
    g = cf.k5_graphs()[name]
    host = conductance_ranking(g, cond=cf.k5_oracle(name)["cond"])
    cond_t = k5_device_cond[name]
    assert cond_t.is_cuda
    np.testing.assert_array_equal(conductance_ranking_device(g, cond_t), host)


def test_k5_trainer_seeds_match_host_ranking():
    g = cf.k5_graphs()["clique-ladder"]
    cfg = BigClamConfig(k=8, device="cuda")
    tr = Trainer(g, cfg, rank=0, world_size=1, device=DEV)
    assert tr.state.use_hip
    host = conductance_ranking(g, cond=cf.k5_oracle("clique-ladder")["cond"])
    np.testing.assert_array_equal(tr.seeds(), host)


# ----------------------------------------------------------------------- K6
def _compact_adjacency(g, seeds):
    seeds = np.asarray(seeds, dtype=np.int64)
    rows = [g.neighbors(int(s)).astype(np.int64) for s in seeds]
    sindptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    snbrs = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return (torch.from_numpy(sindptr.astype(np.int64)).to(DEV),
            torch.from_numpy(snbrs).to(DEV), torch.from_numpy(seeds).to(DEV))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n_seeds", sorted(cf.K6_KP))
def test_k6_scatter_into_prefilled_F(n_seeds, dtype):
    """ext.seed_init on an F pre-filled with 0.25, every shard and both
    include_seed settings: untouched elements, pad columns and the other
    bf16 half of every written word keep the fill."""
    _, ext = _hip()
    g, _ = cf.ladder_graph("hub")
    kp = cf.K6_KP[n_seeds]
    sindptr, snbrs, seeds = _compact_adjacency(g, cf.k6_seed_lists()[n_seeds])
    for inc in (False, True):
        got = {}
        for a, b in cf.k6_all_shards():
            F = torch.full((b - a, kp), 0.25, device=DEV, dtype=DTYPES[dtype])
            ext.seed_init(F, sindptr, snbrs, seeds, a, b, inc)
            got[(a, b)] = F.double().cpu().numpy()
            want = cf.k6_oracle(n_seeds, (a, b), inc, 0.25)
            if not np.array_equal(got[(a, b)], want):
                r, c = np.argwhere(got[(a, b)] != want)[0]
                raise AssertionError(
                    f"{n_seeds} seeds, rows {a}:{b}, include_seed={inc}: "
                    f"F[{r}, {c}] = {got[(a, b)][r, c]}, oracle {want[r, c]}")
        sh = cf.k6_shards()
        assert got[sh["empty"]].shape == (0, kp)
        assert np.array_equal(np.concatenate([got[s] for s in sh["split"]]),
                              got[sh["full"]])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_k6_through_shard_state(dtype):
    """hip_ops.seed_init_device on a ShardState (one shard, then rank 1 of
    3 with halo rows) == the fill = 0 oracle over all kp columns."""
    hip_ops, _ = _hip()
    g, _ = cf.ladder_graph("hub")
    seeds = cf.k6_seed_lists()[37]
    cfg = BigClamConfig(k=37, device="cuda", dtype=dtype)
    for rank, world in ((0, 1), (1, 3)):
        sh = make_shard(g, rank, world)
        st = ShardState(sh, cfg, device=DEV)
        assert st.kp == 40
        st.F.fill_(0.5)  # the wrapper zeroes F itself
        for inc in (False, True):
            hip_ops.seed_init_device(st, g, seeds, inc)
            want = oracle.seed_scatter(g.indptr, g.indices, seeds, sh.start,
                                       sh.stop, 40, inc, 0.0)
            assert np.array_equal(st.F_local.double().cpu().numpy(), want)
            assert not st.F[sh.n_local:].any()  # halo rows stay zero


# ------------------------------------------------------------ 64-bit offsets
def test_k6_k7_rows_beyond_2_31_elements():
    """Row offsets past 2^31 elements (a 4 GiB bf16 shard): K6 writes and
    K7 reads rows whose first element lies at and beyond 2^31.  Nothing of
    the 4 GiB is copied to the host."""
    hip_ops, ext = _hip()
    kp = 16384
    top = 1 << 17  # row `top` starts at element 2^31
    F = torch.zeros(top + 1, kp, device=DEV, dtype=torch.bfloat16)
    assert F.numel() == (1 << 31) + kp
    # seed kp-1 (column kp-1) has the neighbours 0 and `top`
    sindptr = torch.zeros(kp + 1, dtype=torch.int64)
    sindptr[kp] = 2
    snbrs = torch.tensor([0, top], dtype=torch.int64)
    seeds = torch.full((kp,), 5, dtype=torch.int64)
    ext.seed_init(F, sindptr.to(DEV), snbrs.to(DEV), seeds.to(DEV), 0, top + 1,
                  False)
    for r in (0, top):
        assert F[r, kp - 4:].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert not F[1, :4].any() and not F[top - 1, kp - 4:].any()
    assert not F[top, :4].any() and not F[(1 << 16) - 1:(1 << 16) + 1].any()
    planted = {0: [kp - 1], top - 1: [0, 63, 64, kp - 1],
               top: [1, 8191, kp - 2, kp - 1]}
    for r, cols in planted.items():
        F[r, torch.tensor(cols, device=DEV)] = 1.0
    counts, comms = hip_ops.extract_membership(F, kp, cf.K7_DELTA)
    counts = counts.cpu().numpy()
    want = np.zeros(top + 1, dtype=np.int64)
    for r, cols in planted.items():
        want[r] = len(cols)
    np.testing.assert_array_equal(counts, want)
    assert comms.tolist() == sum((planted[r] for r in sorted(planted)), [])


# ---------------------------------------------------------------- validation
def _raises(match):
    return pytest.raises(RuntimeError, match=match)


def test_k6_binding_validation():
    _, ext = _hip()
    g, _ = cf.ladder_graph("hub")
    sindptr, snbrs, seeds = _compact_adjacency(g, cf.k6_seed_lists()[8])
    n = g.num_nodes
    F = torch.full((n, 8), 0.25, device=DEV)
    ext.seed_init(F.clone(), sindptr, snbrs, seeds, 0, n, False)  # valid
    with _raises("F_local"):
        ext.seed_init(F.view(-1), sindptr, snbrs, seeds, 0, n, False)
    s9, n9, seeds9 = _compact_adjacency(
        g, np.append(cf.k6_seed_lists()[8], 0))
    with _raises("n_seeds"):  # a ninth column would run into the next row
        ext.seed_init(F, s9, n9, seeds9, 0, n, False)
    with _raises("1-D"):
        ext.seed_init(F, sindptr, snbrs, seeds.reshape(1, -1), 0, n, False)
    with _raises("1-D"):
        ext.seed_init(F, sindptr, snbrs.reshape(-1, 1), seeds, 0, n, False)
    with _raises("1-D"):
        ext.seed_init(F, sindptr.reshape(1, -1), snbrs, seeds, 0, n, False)
    with _raises("start"):
        ext.seed_init(F, sindptr, snbrs, seeds, n, 0, False)
    with _raises("sindptr"):
        ext.seed_init(F, sindptr, snbrs[:-1].contiguous(), seeds, 0, n, False)
    torch.cuda.synchronize()
    assert (F == 0.25).all()  # nothing was launched


def test_k7_binding_validation():
    _, ext = _hip()
    F = torch.ones(4, 8, device=DEV)
    counts = torch.full((4,), -7, device=DEV, dtype=torch.int32)
    offsets = torch.zeros(4, device=DEV, dtype=torch.int64)
    comms = torch.full((64,), -1, device=DEV, dtype=torch.int32)
    odd = torch.ones(4, 7, device=DEV, dtype=torch.bfloat16)
    with _raises("F_local"):
        ext.extract_count(F.view(-1), 8, 0.5, counts)
    with _raises("F_local"):
        ext.extract_fill(F.view(-1), 8, 0.5, offsets, comms)
    with _raises("ldF"):
        ext.extract_count(odd, 7, 0.5, counts)
    with _raises("ldF"):
        ext.extract_fill(odd, 7, 0.5, offsets, comms)
    with _raises("counts"):
        ext.extract_count(F, 8, 0.5, counts.reshape(4, 1))
    with _raises("offsets"):
        ext.extract_fill(F, 8, 0.5, offsets.reshape(4, 1), comms)
    torch.cuda.synchronize()
    assert (counts == -7).all() and (comms == -1).all()
    # an odd row stride is fine in fp32
    ext.extract_count(torch.ones(4, 7, device=DEV), 7, 0.5, counts)
    assert counts.tolist() == [7] * 4


def test_k5_binding_validation():
    _, ext = _hip()
    g = cf.k5_graphs()["K3"]
    indptr = torch.from_numpy(g.indptr.astype(np.int64)).to(DEV)
    indices = torch.from_numpy(g.indices.astype(np.int32)).to(DEV)
    cond = torch.full((3,), -1.0, device=DEV, dtype=torch.float64)
    with _raises("indptr"):
        ext.conductance(indptr.reshape(2, 2), indices, cond, 6.0)
    with _raises("indptr"):
        ext.conductance(indptr[:0].contiguous(), indices, cond, 6.0)
    with _raises("cond"):
        ext.conductance(indptr, indices, cond.reshape(3, 1), 6.0)
    torch.cuda.synchronize()
    assert (cond == -1.0).all()
    ext.conductance(indptr, indices, cond, 6.0)
    assert cond.tolist() == [1.0, 1.0, 1.0]
