"""GPU tests (MI355X) of the native sparse-sweep routing (``sparse_route``:
kr_bounds / kr_scan / kr_place), of KFS/KFW reading its node-local int32
prefix, and of the fixed-order stage 2 of the list-based sumF refresh.

The routing reference is ``ShardState.sparse_bounds`` + the torch class key
and stable sort (what ``BIGCLAM_NATIVE_ROUTE=0`` runs); every routing
comparison is exact integer equality.
"""
import functools

import numpy as np
import pytest
import torch

import contract_fixtures as cf
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState
from test_gpu_contract import (DEV, _hip, _state,  # noqa: F401
                               _stop_after_gpu_fault)
from test_gpu_kfs_wave import _check_sweep

pytestmark = pytest.mark.gpu

TILE = 64  # asserted against the extension in test_tile_constant


# ------------------------------------------------------------------ shapes
@functools.lru_cache(maxsize=None)
def _shape(name):
    """(indptr [n_local+1], indices [nnz] int32, n_local, n_rows) on the
    CPU.  Rows past n_local are halo rows: they carry a support count and
    appear as neighbours, but are not routed."""
    if name in ("small", "hub"):
        g, _ = cf.ladder_graph(name)
        ip, ix = np.asarray(g.indptr), np.asarray(g.indices)
        return ip, ix.astype(np.int32), g.num_nodes, g.num_nodes
    if name.startswith("prefix"):  # the first n rows of the hub ladder own
        n = int(name[6:])
        ip, ix, _, n_rows = _shape("hub")
        return ip[: n + 1].copy(), ix[: ip[n]].copy(), n, n_rows
    if name.startswith("hubx"):  # disjoint copies: more than 1024 tiles
        reps = int(name[4:])
        ip, ix, n, _ = _shape("hub")
        nnz = ip[-1]
        ips = np.concatenate(
            [ip[:1]] + [ip[1:] + r * nnz for r in range(reps)])
        ixs = np.concatenate([ix + r * n for r in range(reps)])
        return ips, ixs.astype(np.int32), n * reps, n * reps
    if name.startswith("star"):  # one hub above a whole-block round
        d = int(name[4:])
        ip = np.concatenate([[0, d], d + 1 + np.arange(d)]).astype(np.int64)
        ix = np.concatenate([1 + np.arange(d), np.zeros(d)]).astype(np.int32)
        return ip, ix, d + 1, d + 1
    if name.startswith("shard"):  # world_size = 3 shard of the hub ladder
        g, _ = cf.ladder_graph("hub")
        s = make_shard(g, int(name[5:]), 3)
        return (np.asarray(s.indptr), np.asarray(s.indices, dtype=np.int32),
                s.n_local, s.n_rows)
    raise ValueError(name)


def _order(indptr):
    deg = np.diff(indptr)
    return np.argsort(-deg, kind="stable").astype(np.int32)


def _ref_route(indptr, indices, scount, order, cap, wcap):
    """The torch routing on the CPU: (bound int64, cs, by_class, totals)."""
    n = len(indptr) - 1
    bound, cs = ShardState.sparse_bounds(
        torch.from_numpy(scount), torch.from_numpy(indptr),
        torch.from_numpy(indices.astype(np.int64)), n)
    key = (bound > cap).to(torch.uint8) * 2
    if wcap > 0:
        key += (bound <= wcap).to(torch.uint8)
    o64 = torch.from_numpy(order.astype(np.int64))
    skey, perm = torch.sort(key[o64], stable=True)
    totals = [int((skey == c).sum()) for c in range(3)]
    return bound.numpy(), cs.numpy(), order[perm.numpy()], totals


def _run_route(indptr, indices, scount, order, cap, wcap, kp=8):
    _, ext = _hip()
    n, nnz = len(order), len(indices)
    nt3 = 3 * ((n + TILE - 1) // TILE)
    i32 = dict(device=DEV, dtype=torch.int32)
    # poisoned outputs: an unwritten slot cannot pass for a right one
    epre = torch.full((nnz,), -7, **i32)
    bound = torch.full((n,), -7, **i32)
    cls = torch.full((n,), 9, device=DEV, dtype=torch.uint8)
    tcount, tbase = torch.full((nt3,), -7, **i32), torch.full((nt3,), -7, **i32)
    totals = torch.full((3,), -7, **i32)
    GG = torch.full((1,), -7.0, device=DEV)
    by_class = torch.full((n,), -7, **i32)
    sumF = torch.linspace(-1.0, 2.0, kp, device=DEV)
    got = ext.sparse_route(
        torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV),
        torch.from_numpy(scount).to(DEV), torch.from_numpy(order).to(DEV),
        sumF, cap, wcap, epre, bound, cls, tcount, tbase, totals, GG,
        by_class)
    torch.cuda.synchronize()
    gg64 = float((sumF.double() ** 2).sum())
    assert abs(float(GG[0]) - gg64) <= 4 * kp * 2.0 ** -24 * gg64
    return (epre.cpu().numpy(), bound.cpu().numpy(), by_class.cpu().numpy(),
            [int(x) for x in got], totals.cpu().numpy().tolist())


def _check_route(name, scount, cap, wcap, kp=8):
    indptr, indices, n, n_rows = _shape(name)
    assert scount.shape == (n_rows,) and scount.dtype == np.int32
    order = _order(indptr)
    rb, cs, r_by, r_tot = _ref_route(indptr, indices, scount, order, cap, wcap)
    epre, bound, by_class, got, dev_tot = _run_route(
        indptr, indices, scount, order, cap, wcap, kp)
    np.testing.assert_array_equal(bound, np.minimum(rb, cap + 1))
    assert got == r_tot and dev_tot == r_tot
    np.testing.assert_array_equal(by_class, r_by)
    row = np.repeat(np.arange(n), np.diff(indptr))
    live = (rb <= cap)[row]
    want = cs[:-1] - cs[indptr[:-1]][row]
    np.testing.assert_array_equal(epre[live], want[live])
    return rb, r_tot


def _random_sc(n_rows, seed):
    rng = np.random.default_rng(seed)
    sc = rng.integers(1, 41, size=n_rows)
    sc[rng.random(n_rows) < 0.3] = 0
    return sc.astype(np.int32)


SHAPES = ["small", "hub", f"prefix{TILE - 1}", f"prefix{TILE}",
          f"prefix{TILE + 1}", "hubx110", "star2100", "shard0", "shard1",
          "shard2"]


def test_tile_constant():
    _, ext = _hip()
    assert ext.sparse_route_tile() == TILE


@pytest.mark.parametrize("name", SHAPES)
def test_route_all_zero(name):
    """All-zero counts (the benchmark's state): everything is wave class."""
    n_rows = _shape(name)[3]
    _, tot = _check_route(name, np.zeros(n_rows, np.int32), 1024, 256)
    assert tot[0] == 0 and tot[2] == 0


@pytest.mark.parametrize("name", SHAPES)
def test_route_random(name):
    """Counts in [0, 40] with 30 % zeros (halo rows included): on the
    ladders all three classes are populated at cap=1024, wcap=64."""
    n_rows = _shape(name)[3]
    _, tot = _check_route(name, _random_sc(n_rows, 5), 1024, 64)
    if name in ("small", "hub", "hubx110"):
        assert tot[0] > 0 and tot[1] > 0
    if name in ("hub", "hubx110", "star2100"):
        assert tot[2] > 0


@pytest.mark.parametrize("name", ["small", "hub", "shard1", "star2100"])
def test_route_empty_classes(name):
    """One class empty at a time: no wave class (wcap = 0), all dense, no
    block class (wcap = cap)."""
    n_rows = _shape(name)[3]
    sc = _random_sc(n_rows, 6)
    _, tot = _check_route(name, sc, 1024, 0)
    assert tot[1] == 0 and tot[0] > 0
    _, tot = _check_route(name, np.full(n_rows, 50, np.int32), 40, 16)
    assert tot[0] == 0 and tot[1] == 0
    _, tot = _check_route(name, sc, 1024, 1024)
    assert tot[0] == 0 and tot[1] > 0


@pytest.mark.parametrize("name", ["small", "hub", "hubx110"])
def test_route_boundary(name):
    """Counts of 1 give bound = degree + 1; wcap = 17 has the degree-16
    centre at the bound and the degree-17 centre one above it."""
    n_rows = _shape(name)[3]
    rb, tot = _check_route(name, np.ones(n_rows, np.int32), 64, 17)
    assert (rb == 17).any() and (rb == 18).any()
    assert (rb == 64).any() and (rb == 65).any()  # the same at cap
    assert min(tot) > 0


@pytest.mark.parametrize("name", ["hub", "hubx110", "shard0", "shard1",
                                  "shard2", "star2100"])
def test_route_saturation(name):
    """Every neighbour of the widest local node at 2^30: its true bound
    passes 2^31; the saturated bound is cap + 1, nothing wraps, and the
    node is dense."""
    indptr, indices, n, n_rows = _shape(name)
    hub = int(np.argmax(np.diff(indptr)))
    assert np.diff(indptr)[hub] >= 200
    sc = _random_sc(n_rows, 7)
    sc[indices[indptr[hub]: indptr[hub + 1]]] = 2 ** 30
    rb, tot = _check_route(name, sc, 1024, 256)
    assert rb[hub] >= 200 * 2 ** 30
    order = _order(indptr)
    r_by = _ref_route(indptr, indices, sc, order, 1024, 256)[2]
    assert hub in r_by[tot[0] + tot[1]:].tolist()


# -------------------------------------------------------------- end to end
def _pack_snapshot(st):
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None, "sparse routing did not engage"
    return dict(
        order=pack["order"].cpu().numpy(), nb=int(pack["n_block"]),
        order_d=pack["order_d"].cpu().numpy(),
        go=pack["goffset"].cpu().numpy(), gc=pack["gcount"].cpu().numpy(),
        gi=pack["gidx"].cpu().numpy(), gv=pack["gval"].cpu().numpy(),
        llh=llh.cpu().numpy(), best=best.cpu().numpy())


def _native_vs_torch(case, wcap, tag, monkeypatch):
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", str(wcap))
    monkeypatch.setenv("BIGCLAM_NATIVE_ROUTE", "0")
    _, st_t = _state(case)
    assert not st_t.native_route
    a = _pack_snapshot(st_t)
    monkeypatch.delenv("BIGCLAM_NATIVE_ROUTE")
    cfg, st_n = _state(case)
    assert st_n.native_route
    b = _pack_snapshot(st_n)
    np.testing.assert_array_equal(a["order"], b["order"])
    assert a["nb"] == b["nb"]
    np.testing.assert_array_equal(a["order_d"], b["order_d"])
    nb = a["nb"]
    np.testing.assert_array_equal(a["go"], b["go"])
    wave = a["order"][nb:].astype(np.int64)
    np.testing.assert_array_equal(a["gc"][nb:], b["gc"][nb:])
    sel = np.concatenate(
        [np.arange(0)] +
        [np.arange(o, o + c) for o, c in zip(a["go"][nb:], a["gc"][nb:])]
    ).astype(np.int64)
    np.testing.assert_array_equal(a["gi"][sel], b["gi"][sel])
    np.testing.assert_array_equal(a["gv"][sel].view(np.int32),
                                  b["gv"][sel].view(np.int32))
    np.testing.assert_array_equal(a["llh"][wave].view(np.int64),
                                  b["llh"][wave].view(np.int64))
    np.testing.assert_array_equal(a["best"][wave].view(np.int32),
                                  b["best"][wave].view(np.int32))
    # every node (the block class included) against the fp64 oracle, then
    # the commit: cf.assert_colsum on the stage-2 sumF is part of it
    r = _check_sweep(case, cfg, st_n, wcap, tag)
    assert st_n.sumF.data_ptr() == st_n._sumF_buf.data_ptr()
    return a, r


@pytest.mark.parametrize("wcap", [1024, 64, 0])
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_native_route_sweep(t, wcap, monkeypatch):
    """C5 state (hub ladder, K=512, sparse regime): the native routing and
    the torch routing give the same pack, bitwise on the wave class."""
    case = cf.make_case(*t)
    a, r = _native_vs_torch(case, wcap, f"{case.id}/route/wcap{wcap}",
                            monkeypatch)
    n_s = len(a["order"])
    assert n_s >= 600 and len(a["order_d"]) > 0
    if wcap == 1024:
        assert a["nb"] == 0
    elif wcap == 64:
        assert 0 < a["nb"] < n_s
    else:
        assert a["nb"] == n_s


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_native_route_small_k33(dtype, monkeypatch):
    """Small ladder at K=33, all routed nodes in the wave class: centres of
    degree 65-129 re-read the prefix past the 64-entry edge table; a
    degree-0 node and a degree-1 centre with an empty active set."""
    k = 33
    base = cf.make_case("small", "sparse", dtype, k)
    g, label = base.graph, base.label
    indptr, indices = np.asarray(g.indptr), np.asarray(g.indices)
    F0 = base.F0.copy()
    c1 = int(np.flatnonzero(label == 1)[0])
    iso = int(np.flatnonzero(label == -2)[0])
    F0[[c1, iso, int(indices[indptr[c1]])]] = 0.0
    case = cf.Case(base.kind, base.regime, dtype, k, g, label, base.cfg, F0)
    a, r = _native_vs_torch(case, 1024, f"{case.id}/route", monkeypatch)
    assert a["nb"] == 0
    assert np.diff(indptr)[a["order"]].max() >= 129
    pos = {int(u): b for b, u in enumerate(a["order"])}
    assert a["gc"][pos[c1]] == 0 and a["gc"][pos[iso]] == 0


def test_order_buffers_alternate(monkeypatch):
    """A carried pack's order/order_d survive the next sweep's routing."""
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "64")
    case = cf.make_case("hub", "sparse", "bf16", 512)
    _, st = _state(case)
    assert st._last_nnz is None
    grad, _, best, pack = st.grad_ls_auto(None)
    o0, d0 = pack["order"].clone(), pack["order_d"].clone()
    # the next routing pass (same F) must not write into the carried pack
    _, _, _, pack2 = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack2["order"].data_ptr() != pack["order"].data_ptr()
    assert torch.equal(pack2["order"], o0)
    st._rt["by_class"][st._rt_flip].fill_(-1)  # scribble on the new one
    assert torch.equal(pack["order"], o0) and torch.equal(pack["order_d"], d0)
    assert int(st._last_nnz.item()) == int(st._sp_scount[: st.n_local].sum())
    F_before = st.F_local.clone()
    st.apply_commit(grad, best, pack)  # the carried pack still commits
    torch.cuda.synchronize()
    cf.assert_colsum("carried/sumF", st.sumF.cpu().numpy(), st.F_local)
    assert not torch.equal(F_before, st.F_local)


# ----------------------------------------------------------------- stage 2
@pytest.mark.parametrize("kp", [8, 2048, 5000, 8200])
@pytest.mark.parametrize("n_local", [1, 512, 513, 1537, 40000])
def test_colsum_stage2(n_local, kp):
    """Fixed-order fp32 sum of the [m, kp] stripe partials: within
    (m - 1) * 2^-24 * sum|x| of the fp64 sum per column, and bitwise
    repeatable.  (n_local = 40000 is 79 stripes: more than one pass of the
    32 row groups; kp = 8200 is wider than one KCS_KCH chunk.)"""
    _, ext = _hip()
    m = (n_local + 511) // 512
    gen = torch.Generator().manual_seed(100 * m + kp)
    x = ((torch.rand(m, kp, generator=gen) - 0.5) * 8.0).to(DEV)
    out = [torch.full((kp,), float("nan"), device=DEV) for _ in range(2)]
    for o in out:
        ext.colsum_stage2(x, o)
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    ref = x.double().sum(0)
    tol = (m - 1) * 2.0 ** -24 * x.double().abs().sum(0)
    err = (out[0].double() - ref).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
