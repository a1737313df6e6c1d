"""GPU tests (MI355X) of the packed wave kernel (KFP: four low-bound
wave-class nodes per wave) and of the packed / single split of the wave
class that routing produces for it.

KFP's contract is bitwise: for the same node it writes the gcount, gidx,
gval, llh and best that the one-wave-per-node kernel (KFW) writes, so every
comparison here is exact equality against a sweep with
BIGCLAM_SPARSE_QCAP=0; the oracle rules of tests/test_gpu_kfs_wave.py run
on the packed sweep as well.  Fixture counts come from
tests/kfp_fixtures.py (checked on the CPU in tests/test_kfp_split_cpu.py).
"""
import functools

import numpy as np
import pytest
import torch

import contract_fixtures as cf
import kfp_fixtures as kf
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState
from test_gpu_contract import (DEV, _hip, _Judge, _state,  # noqa: F401
                               _stop_after_gpu_fault)
from test_gpu_kfs_wave import _check_sweep

pytestmark = pytest.mark.gpu

TILE = 64


def _env(mp, qcap, wcap=1024, cap=1024):
    mp.setenv("BIGCLAM_SPARSE", "1")
    mp.setenv("BIGCLAM_SPARSE_CAP", str(cap))
    mp.setenv("BIGCLAM_SPARSE_WCAP", str(wcap))
    mp.setenv("BIGCLAM_SPARSE_QCAP", str(qcap))


def _snapshot(case, sumF=None, commit=True):
    """One routed sweep (+ commit) of a fresh state under the current
    environment: everything the packed path may touch, as numpy."""
    cfg, st = _state(case)
    if sumF is not None:
        st.sumF.fill_(sumF)
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None, "sparse routing did not engage"
    n = int(pack["order"].numel())
    go = pack["goffset"].cpu().numpy()[:n]
    gc = pack["gcount"].cpu().numpy()[:n]
    sel = np.concatenate([np.arange(0)] + [np.arange(o, o + c)
                                           for o, c in zip(go, gc)]).astype(
                                               np.int64)
    routed = pack["order"].long()
    out = dict(
        order=pack["order"].cpu().numpy(), nb=np.int64(pack["n_block"]),
        gc=gc, gi=pack["gidx"].cpu().numpy()[sel],
        gv=pack["gval"].cpu().numpy()[sel].view(np.int32),
        llh=llh[routed].cpu().numpy().view(np.int64),
        best=best[routed].cpu().numpy().view(np.int32))
    meta = dict(n_pack=int(pack["n_pack"]), qcap=st.sparse_qcap,
                n_wave=n - int(pack["n_block"]), st=st, cfg=cfg)
    if commit:
        st.apply_commit(grad, best, pack)
        torch.cuda.synchronize()
        cap = st._sp_cap
        sc = st._sp_scount.cpu().numpy()[: st.n_local]
        rows = pack["order"].cpu().numpy().astype(np.int64)
        lsel = np.concatenate([np.arange(0)] + [
            np.arange(r * cap, r * cap + sc[r]) for r in rows]).astype(
                np.int64)
        out.update(
            F=st.F_local.float().cpu().numpy().view(np.int32),
            scount=sc, sidx=st._sp_sidx.cpu().numpy()[lsel],
            sval=st._sp_sval.cpu().numpy()[lsel].view(np.int32))
    return out, meta


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@functools.lru_cache(maxsize=None)
def _c5_reference(t):
    """The QCAP=0 sweep of a C5 case, computed once."""
    mp = pytest.MonkeyPatch()
    try:
        _env(mp, 0)
        ref, meta = _snapshot(cf.make_case(*t))
    finally:
        mp.undo()
    assert meta["n_pack"] == 0 and meta["qcap"] == 0
    return ref


# ------------------------------------------------------- 1. bitwise, C5
@pytest.mark.parametrize("qcap,n_pack,single", [(64, 39, 572),
                                                (256, 442, 169)])
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_pack_bitwise_c5(t, qcap, n_pack, single, monkeypatch):
    """Hub ladder, K=512, sparse: packed sweep == single-wave sweep on every
    routed output and on the committed F and lists.  QCAP=256 has 11 nodes
    at bound 256 (packed when their degree allows) and 5 at 257 (single)."""
    case = cf.make_case(*t)
    b = kf.case_bounds(case)
    deg = np.diff(np.asarray(case.graph.indptr))
    assert ((b == 256).sum(), (b == 257).sum()) == (11, 5)
    assert kf.eligible(b, deg, 1024, qcap).sum() == n_pack
    ref = _c5_reference(t)
    _env(monkeypatch, qcap)
    got, meta = _snapshot(case)
    assert meta["qcap"] == qcap
    assert meta["n_pack"] == n_pack and meta["n_pack"] > 0
    assert meta["n_wave"] - meta["n_pack"] == single and single > 0
    _assert_same(ref, got)
    if qcap == 256:
        order = got["order"].astype(np.int64)
        ws = meta["st"]._wave_split[0].cpu().numpy()[: meta["n_wave"]]
        packed = set(order[ws[:n_pack]].tolist())
        assert not packed & set(np.flatnonzero(b == 257).tolist())
        at = np.flatnonzero((b == 256) & (deg <= 16))
        assert len(at) and set(at.tolist()) <= packed


# ------------------------------------- 2. degree edge and bitmap edge
@pytest.mark.parametrize("k,qcap,n_pack,dtype", [
    (33, 64, 138, "fp32"), (33, 64, 138, "bf16"), (33, 16, 81, "fp32"),
    (33, 16, 81, "bf16"), (1000, 1000, None, "bf16")])
def test_pack_edge_shapes(k, qcap, n_pack, dtype, monkeypatch):
    """Small ladder with the wave kernel's hand-set rows.  K=33: the
    bitmap's only words are partly used; QCAP=64 packs degrees 0..16 and
    leaves the degree-17 nodes (bound within qcap) single.  K=1000 with
    QCAP=1000 (bf16): the last bitmap word a quarter used."""
    case, hand = kf.edge_case(dtype, k)
    b = kf.case_bounds(case)
    indptr = np.asarray(case.graph.indptr)
    deg = np.diff(indptr)
    el = kf.eligible(b, deg, 1024, qcap)
    if n_pack is not None:
        assert el.sum() == n_pack
    if (k, qcap) == (33, 64):
        assert sorted(set(deg[el].tolist())) == list(range(17))
        assert (deg == 17).any() and (b[deg == 17] <= qcap).all()
    _env(monkeypatch, 0)
    ref, _ = _snapshot(case)
    _env(monkeypatch, qcap)
    got, meta = _snapshot(case)
    assert meta["n_pack"] == el.sum() > 0
    _assert_same(ref, got)
    order = got["order"].astype(np.int64)
    ws = meta["st"]._wave_split[0].cpu().numpy()[: meta["n_wave"]]
    packed = set(order[ws[: meta["n_pack"]]].tolist())
    assert not packed & set(np.flatnonzero(deg > 16).tolist())
    for name in ("c1", "iso", "c2"):
        assert hand[name] in packed
    pos = {int(u): i for i, u in enumerate(order)}
    assert got["gc"][pos[hand["c1"]]] == 0 and got["gc"][pos[hand["iso"]]] == 0
    # the C5 oracle rules on a packed sweep of a fresh state
    cfg, st = _state(case)
    assert st.sparse_qcap == min(qcap, st.sparse_wcap)
    _check_sweep(case, cfg, st, st.sparse_wcap, f"{case.id}/qcap{qcap}")


# --------------------------------------------------------- 3. quad tails
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pack_quad_tails(dtype, monkeypatch):
    """n_pack % 4 in {0, 1, 2, 3} on the edge-shape state with rows zeroed
    (QCAP=16), and the hand-built single quad: a degree-16 node with
    ns == bound == qcap next to degree-0 nodes, then 3, 2, 1 live groups."""
    tails = kf.tail_rows(dtype, 33, 1024, 16)
    assert sorted(tails) == [0, 1, 2, 3]
    for res, rows in sorted(tails.items()):
        case, _ = kf.edge_case(dtype, 33, zero_rows=rows)
        _env(monkeypatch, 0)
        ref, _ = _snapshot(case, commit=False)
        _env(monkeypatch, 16)
        got, meta = _snapshot(case, commit=False)
        assert meta["n_pack"] % 4 == res and meta["n_pack"] > 0
        _assert_same(ref, got)
    for drop in range(4):
        case, hand = kf.quad_case(dtype, drop=drop)
        _env(monkeypatch, 0)
        ref, _ = _snapshot(case, commit=False)
        _env(monkeypatch, 20)
        got, meta = _snapshot(case, commit=False)
        assert meta["n_pack"] == 4 - drop
        _assert_same(ref, got)
        order = got["order"].astype(np.int64)
        ws = meta["st"]._wave_split[0].cpu().numpy()
        quad = order[ws[: meta["n_pack"]]].tolist()
        assert quad[0] == hand["c16"]
        assert set(quad[1:]) <= set(hand["zero_deg"])
        pos = {int(u): i for i, u in enumerate(order)}
        assert got["gc"][pos[hand["c16"]]] == 20  # ns == qcap


# -------------------------------------------------- 4. all-zero state
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("sumF", [0.0, 0.25])
def test_pack_all_zero_state(sumF, dtype, monkeypatch):
    """F all zero on the small ladder: gcount == 0 everywhere.  sumF = 0
    (GG = 0) accepts the first ladder step on every node.  With sumF != 0
    a trial changes nothing and the Armijo margin alpha*s*GG is positive:
    a node without edges (llh 0) accepts no step; a node with edges
    accepts the first step whose margin rounds away against its llh
    (|llh| ~ 9.2 per edge in fp64, the last ladder steps are ~1e-14), which
    the test derives from the returned llh and the kernels' summation
    trees.  QCAP=0 gives the same picks bit for bit."""
    hip_ops, _ = _hip()
    base = cf.make_case("small", "sparse", dtype, 33)
    case = cf.Case(base.kind, base.regime, dtype, 33, base.graph, base.label,
                   base.cfg, np.zeros_like(base.F0))
    _env(monkeypatch, 0)
    ref, _ = _snapshot(case, sumF=sumF, commit=False)
    _env(monkeypatch, 64)
    got, meta = _snapshot(case, sumF=sumF, commit=False)
    deg = np.diff(np.asarray(case.graph.indptr))
    assert meta["n_pack"] == (deg <= 16).sum()
    _assert_same(ref, got)
    assert (got["gc"] == 0).all()
    cfg = meta["cfg"]
    lad = hip_ops._ladder(cfg, DEV).cpu().numpy().astype(np.float32)
    best = got["best"].view(np.float32)
    order = got["order"].astype(np.int64)
    if sumF == 0.0:
        np.testing.assert_array_equal(best, np.full(len(best), lad[0]))
        return
    llh = got["llh"].view(np.float64)
    one = float(llh[np.flatnonzero(deg[order] == 1)[0]])  # one edge's term
    gg = np.float32(meta["st"].kp) * np.float32(sumF) * np.float32(sumF)
    want = np.zeros(len(order), np.float32)
    for i, u in enumerate(order):
        acc = [0.0, 0.0, 0.0, 0.0]
        for e in range(int(deg[u])):
            acc[e & 3] += one
        node_llh = (acc[0] + acc[2]) + (acc[1] + acc[3])
        assert node_llh == llh[i]
        trial = (acc[0] + acc[1]) + (acc[2] + acc[3])
        for s_j in lad:
            margin = np.float32(np.float32(cfg.alpha) * s_j) * gg
            if trial >= node_llh + float(margin):
                want[i] = s_j
                break
    np.testing.assert_array_equal(best, want)
    assert (best[deg[order] == 0] == 0.0).all() and (deg[order] == 0).sum() == 3


# ------------------------------------------------------- 5. the split
@functools.lru_cache(maxsize=None)
def _shape(name):
    """(indptr, indices int32, n_local, n_rows): the small / hub ladders
    and the first n rows of the hub ladder (rows past n_local are halo)."""
    if name in ("small", "hub"):
        g, _ = cf.ladder_graph(name)
        ip, ix = np.asarray(g.indptr), np.asarray(g.indices)
        return ip, ix.astype(np.int32), g.num_nodes, g.num_nodes
    n = int(name[6:])
    ip, ix, _, n_rows = _shape("hub")
    return ip[: n + 1].copy(), ix[: ip[n]].copy(), n, n_rows


def _route(name, scount, cap, wcap, qcap=None):
    _, ext = _hip()
    indptr, indices, n, n_rows = _shape(name)
    order = kf.launch_order(indptr)
    nt = (n + TILE - 1) // TILE
    i32 = dict(device=DEV, dtype=torch.int32)
    # poisoned outputs: an unwritten slot cannot pass for a right one
    bufs = dict(
        epre=torch.full((len(indices),), -7, **i32),
        bound=torch.full((n,), -7, **i32),
        cls=torch.full((n,), 9, device=DEV, dtype=torch.uint8),
        tcount=torch.full((3 * nt,), -7, **i32),
        tbase=torch.full((3 * nt,), -7, **i32),
        totals=torch.full((3,), -7, **i32),
        GG=torch.full((1,), -7.0, device=DEV),
        by_class=torch.full((n,), -7, **i32))
    extra = ()
    if qcap is not None:
        wsplit = torch.full((n,), -7, **i32)
        extra = (qcap, wsplit, torch.full((4 * nt + 1,), -7, **i32))
    got = ext.sparse_route(
        torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV),
        torch.from_numpy(scount).to(DEV), torch.from_numpy(order).to(DEV),
        torch.linspace(-1.0, 2.0, 8, device=DEV), cap, wcap, *bufs.values(),
        *extra)
    torch.cuda.synchronize()
    pinned = {k: v.cpu().numpy() for k, v in bufs.items()}
    pinned["GG"] = pinned["GG"].view(np.int32)
    ws = extra[1].cpu().numpy() if extra else None
    return [int(x) for x in got], pinned, ws


@pytest.mark.parametrize("name", ["small", "hub", f"prefix{TILE - 1}",
                                  f"prefix{TILE}", f"prefix{TILE + 1}"])
def test_route_split(name):
    """wsplit / n_pack == the numpy stable partition of the wave class;
    every pinned routing output is bitwise what a call without the optional
    arguments writes.  Covers qcap = 0, qcap = wcap and an empty packed
    set next to a populated wave class."""
    indptr, indices, n, n_rows = _shape(name)
    deg = np.diff(indptr)
    order = kf.launch_order(indptr)
    rng = np.random.default_rng(5)
    sc = rng.integers(1, 41, size=n_rows)
    sc[rng.random(n_rows) < 0.3] = 0
    sc = sc.astype(np.int32)
    runs = [(sc, 1024, 256, 64), (sc, 1024, 64, 64), (sc, 1024, 256, 0),
            (sc, 1024, 64, 16), (np.zeros(n_rows, np.int32), 1024, 256, 64),
            (np.zeros(n_rows, np.int32), 1024, 64, 64),
            (np.full(n_rows, 50, np.int32), 1024, 256, 8)]
    for scount, cap, wcap, qcap in runs:
        bound, _ = ShardState.sparse_bounds(
            torch.from_numpy(scount), torch.from_numpy(indptr),
            torch.from_numpy(indices.astype(np.int64)), n)
        nb, want, n_pack = kf.split_wave_class(order, bound.numpy(), deg, cap,
                                               wcap, qcap)
        base, pinned0, _ = _route(name, scount, cap, wcap)
        got, pinned1, ws = _route(name, scount, cap, wcap, qcap)
        assert len(base) == 3 and got[:3] == base
        assert got[0] == nb and got[1] == len(want) and got[3] == n_pack
        np.testing.assert_array_equal(ws[: len(want)], want)
        assert (ws[len(want):] == -7).all()  # nothing past the wave class
        _assert_same(pinned0, pinned1)
        if qcap == 0 or (scount == 50).all():
            assert n_pack == 0
        if (scount == 50).all() and name in ("small", "hub"):
            assert len(want) > 0  # a wave class with nothing packable
        if (scount == 0).all() and name in ("small", "hub"):
            assert 0 < n_pack < len(want)  # the degree rule alone splits


# ------------------------------------------------ 6. clamp and switch
def test_pack_cap_clamp(monkeypatch):
    """sparse_qcap is clamped to sparse_wcap and to the 64 KB workgroup by
    the launcher's size function."""
    _, ext = _hip()
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "60000")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "50000")
    monkeypatch.setenv("BIGCLAM_SPARSE_QCAP", "40000")
    for dtype, k in (("fp32", 1000), ("bf16", 1000), ("bf16", 16385)):
        case = cf.make_case("small", "sparse", dtype, k)
        cfg = cf.regime_cfg(case.regime, k, dtype, device="cuda")
        st = ShardState(make_shard(case.graph, 0, 1), cfg, device=DEV)
        q = st.sparse_qcap
        bf = dtype == "bf16"
        assert 0 < q < 40000 and q <= st.sparse_wcap and q % 4 == 0
        assert ext.sparse_pack_lds_bytes(bf, st.kp, q) <= 65536
        assert ext.sparse_pack_lds_bytes(bf, st.kp, q + 4) > 65536
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "128")
    monkeypatch.setenv("BIGCLAM_SPARSE_QCAP", "500")
    assert st.sparse_qcap == st.sparse_wcap == 128
    monkeypatch.setenv("BIGCLAM_SPARSE_QCAP", "0")
    assert st.sparse_qcap == 0
    monkeypatch.setenv("BIGCLAM_SPARSE_QCAP", "64")
    monkeypatch.setenv("BIGCLAM_NATIVE_ROUTE", "0")
    assert st.sparse_qcap == 0


@pytest.mark.parametrize("switch", ["BIGCLAM_SPARSE_QCAP",
                                    "BIGCLAM_NATIVE_ROUTE"])
def test_pack_switch_off(switch, monkeypatch):
    """QCAP=0 and the torch routing both launch no packed kernel: the pack
    reports n_pack == 0 and no split was produced."""
    case = cf.make_case("hub", "sparse", "bf16", 512)
    _env(monkeypatch, 64)
    monkeypatch.setenv(switch, "0")
    got, meta = _snapshot(case, commit=False)
    assert meta["n_pack"] == 0 and meta["qcap"] == 0
    assert meta["st"]._wave_split is None
    ref = _c5_reference(("hub", "sparse", "bf16", 512))
    _assert_same({k: ref[k] for k in got}, got)


# ------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_pack_bitwise_reproducible(t, monkeypatch):
    """Two packed sweeps of the same state are bitwise equal on the packed
    nodes (and on the whole wave class)."""
    _env(monkeypatch, 256)
    case = cf.make_case(*t)
    cfg, st = _state(case)
    runs = []
    for _ in range(2):
        _, llh, best, pack = st.grad_ls_auto(None)
        torch.cuda.synchronize()
        assert int(pack["n_block"]) == 0 and int(pack["n_pack"]) == 442
        ws = st._wave_split[0][: int(pack["n_pack"])].long()
        nodes = pack["order"].long()[ws]
        gc = pack["gcount"][ws].cpu().numpy()
        go = pack["goffset"][ws].cpu().numpy()
        gi, gv = pack["gidx"].cpu().numpy(), pack["gval"].cpu().numpy()
        sel = np.concatenate([np.arange(o, o + c) for o, c in zip(go, gc)])
        runs.append((nodes.cpu().numpy(), llh[nodes].cpu().numpy(),
                     best[nodes].cpu().numpy(), gc, gi[sel],
                     gv[sel].view(np.int32)))
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
