"""GPU tests (MI355X) of the one-wave-per-node sparse sweep kernel (KFW)
and the three-class routing (block kernel | wave kernel | dense).

Same oracle rules as tests/test_gpu_contract.py::test_c5_sparse_routed_sweep
(tests/oracle.py, docs/kernels.md "Numerics contract"): the rebuilt full
gradient, llh and the picks of EVERY node, the K3S commit, the list-based
sumF and the rewritten support lists.
"""
import numpy as np
import pytest
import torch

import contract_fixtures as cf
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState
from test_gpu_contract import (DEV, _Judge, _state,  # noqa: F401
                               _stop_after_gpu_fault)

pytestmark = pytest.mark.gpu


def _bounds(st):
    """Routing bound per local node of the state's CURRENT support counts
    (valid after a grad_ls_auto call)."""
    b, _ = ShardState.sparse_bounds(st._sp_scount, st.indptr, st._indices64,
                                    st.n_local)
    return b.cpu().numpy()


def _fixture_bounds(case):
    """The same bound from the fixture alone (before any kernel ran)."""
    F = case.stored_F().float().numpy()
    sc = torch.from_numpy((F != 0).sum(axis=1).astype(np.int32))
    b, _ = ShardState.sparse_bounds(
        sc, torch.from_numpy(np.asarray(case.graph.indptr)),
        torch.from_numpy(np.asarray(case.graph.indices, dtype=np.int64)),
        case.graph.num_nodes)
    return b.numpy()


def _check_routing(st, pack, wcap):
    """Layout of the routed order: [block class | wave class], each in the
    launch (degree-descending) order, classes decided by the exact bound."""
    n = st.n_local
    cap = st.sparse_cap
    bound = _bounds(st)
    routed = pack["order"].cpu().numpy().astype(np.int64)
    nb = int(pack["n_block"])
    assert len(np.unique(routed)) == len(routed)
    order = st.order.cpu().numpy().astype(np.int64)
    b_o = bound[order]
    want_block = order[(b_o > wcap) & (b_o <= cap)]
    want_wave = order[b_o <= wcap] if wcap > 0 else order[:0]
    np.testing.assert_array_equal(routed[:nb], want_block)
    np.testing.assert_array_equal(routed[nb:], want_wave)
    dense = np.setdiff1d(np.arange(n), routed)
    assert (bound[dense] > cap).all()
    return routed, nb, dense, bound


def _check_sweep(case, cfg, st, wcap, tag):
    """One routed sweep + commit against the oracle (the C5 rules)."""
    bf = case.dtype == "bf16"
    n, kp = st.n_local, st.kp
    assert st.sparse_wcap == wcap
    J = _Judge(st.F, st.sumF, st.shard.indptr, st.shard.indices, cfg,
               case.label, case.k, case.dtype)
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None, "sparse routing did not engage"
    routed, nb, dense, bound = _check_routing(st, pack, wcap)
    assert len(routed) >= 64
    go = pack["goffset"].cpu().numpy()
    gc = pack["gcount"].cpu().numpy()
    gi = pack["gidx"].cpu().numpy()
    gv = pack["gval"].cpu().numpy()
    full = grad.cpu().numpy().copy()
    s32 = st.sumF.cpu().numpy()
    for b, u in enumerate(routed):
        assert 0 <= gc[b] <= (st.sparse_cap if b < nb else wcap)
        ks = gi[go[b]: go[b] + gc[b]]
        assert len(np.unique(ks)) == len(ks) and (ks < kp).all()
        assert (np.diff(ks) > 0).all()  # ascending columns
        full[u] = -s32
        full[u, ks] = gv[go[b]: go[b] + gc[b]]
    full_t = torch.from_numpy(full)
    flags = np.zeros(n, dtype=bool)
    flags[dense] = bf  # dense remainder: MFMA phase B on bf16
    J.check(tag, full_t, llh, best, bf16_candidates=flags)
    # commit: list-based sumF refresh and rewritten support lists
    F_before = st.F_local.clone()
    st.apply_commit(grad, best, pack)
    torch.cuda.synchronize()
    cf.assert_commit(tag + "/k3s", F_before, st.F_local, full_t, best, cfg)
    cf.assert_colsum(tag + "/sumF", st.sumF.cpu().numpy(), st.F_local)
    assert st._kaf_valid
    cap = st._sp_cap
    clean = (st._dirty[:n] == 0).cpu().numpy()
    assert clean[routed].all()
    sc = st._sp_scount.clone()
    sidx = st._sp_sidx.cpu().numpy().copy()
    sval = st._sp_sval.cpu().numpy().copy()
    st._kaf_valid = False  # force a full rescan of the same F
    st.grad_ls_auto(None)
    torch.cuda.synchronize()
    scn, scf = sc.cpu().numpy()[:n], st._sp_scount.cpu().numpy()[:n]
    np.testing.assert_array_equal(scn[clean], scf[clean])
    Fh = st.F_local.float().cpu().numpy()
    nnz = (Fh != 0).sum(axis=1)
    fits = nnz <= cap
    np.testing.assert_array_equal(scf[fits], nnz[fits])
    b_i, b_v = st._sp_sidx.cpu().numpy(), st._sp_sval.cpu().numpy()
    for r in np.flatnonzero(clean & fits & (nnz > 0)):
        sl = slice(r * cap, r * cap + int(nnz[r]))
        np.testing.assert_array_equal(sidx[sl], b_i[sl])
        np.testing.assert_array_equal(sval[sl], b_v[sl])
        np.testing.assert_array_equal(sval[sl], Fh[r, sidx[sl]])
    return dict(routed=routed, nb=nb, bound=bound, gc=gc, gi=gi, go=go,
                dense=dense)


def _boundary_wcap(case):
    """A cap value b with routed nodes at bound == b AND bound == b + 1."""
    ub = np.unique(_fixture_bounds(case))
    pairs = [int(x) for x in ub if x + 1 in ub and 32 <= x < 1024]
    assert pairs, "fixture has no adjacent pair of bounds"
    return pairs[len(pairs) // 2]


# ------------------------------------------------------------- 1. contract
@pytest.mark.parametrize("wcap", [1024, 64, "boundary"])
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_wave_contract(t, wcap, monkeypatch):
    """C5 cases (hub ladder, K=512, sparse regime).  WCAP=1024: every
    routed node runs the wave kernel; WCAP=64 and the boundary value: both
    kernels run in one sweep.  The boundary value b has nodes at bound b
    (wave kernel) and b + 1 (block kernel)."""
    case = cf.make_case(*t)
    boundary = wcap == "boundary"
    if boundary:
        wcap = _boundary_wcap(case)
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", str(wcap))
    cfg, st = _state(case)
    r = _check_sweep(case, cfg, st, wcap, f"{case.id}/wcap{wcap}")
    routed, nb, bound = r["routed"], r["nb"], r["bound"]
    assert len(r["dense"]) > 0  # hubs stay on the dense kernel
    if wcap == 1024:
        assert nb == 0 and len(routed) >= 600
        deg = np.diff(np.asarray(case.graph.indptr))
        assert deg[routed].max() > 16  # more than 4 rounds of 4 edge slots
    else:
        assert 0 < nb < len(routed), "both classes must be non-empty"
    if boundary:
        wave = set(routed[nb:].tolist())
        block = set(routed[:nb].tolist())
        at, above = np.flatnonzero(bound == wcap), np.flatnonzero(
            bound == wcap + 1)
        assert len(at) and len(above)
        assert set(at.tolist()) <= wave and set(above.tolist()) <= block


# ---------------------------------------------------------- 2. edge shapes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k,wcap", [(33, 1024), (33, 16), (1000, 1024),
                                    (1000, 256)])
def test_wave_edge_shapes(k, wcap, dtype, monkeypatch):
    """Small ladder (degrees 0-5, 15-17, 31-33, 63-65, 127-129): K=33 pads
    to 36 (fp32) / 40 (bf16) — the bitmap's last word is partly used;
    K=1000 leaves the last word a quarter used.  Hand-set rows give a
    routed node with an empty active set and edges (ns == 0, degree 1), an
    isolated all-zero node, and columns 0 and K-1 on a wave-class node."""
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", str(wcap))
    base = cf.make_case("small", "sparse", dtype, k)
    g, label = base.graph, base.label
    indptr, indices = np.asarray(g.indptr), np.asarray(g.indices)
    F0 = base.F0.copy()
    c1 = int(np.flatnonzero(label == 1)[0])  # centre of degree 1
    leaf = int(indices[indptr[c1]])
    iso = int(np.flatnonzero(label == -2)[0])
    c2 = int(np.flatnonzero(label == 2)[0])
    F0[[c1, iso]] = 0.0
    # the degree-1 centre's only neighbour: zero as well -> ns == 0 there
    F0[leaf] = 0.0
    F0[c2] = 0.0
    F0[c2, 0] = 0.75
    F0[c2, k - 1] = 0.5
    case = cf.Case(base.kind, base.regime, dtype, k, g, label, base.cfg, F0)
    cfg, st = _state(case)
    assert st.kp == cf.padded_k(k, dtype)
    r = _check_sweep(case, cfg, st, wcap, f"{case.id}/edge/wcap{wcap}")
    routed, nb, gc, gi, go = r["routed"], r["nb"], r["gc"], r["gi"], r["go"]
    pos = {int(u): b for b, u in enumerate(routed)}
    if wcap == 1024:
        assert nb == 0
        deg = np.diff(indptr)
        # K=33: the edge loops iterate past one wave's 64 table entries
        assert deg[routed].max() >= (129 if k == 33 else 17)
    else:
        assert 0 < nb < len(routed)
    # both hand-set empty nodes are in the wave class with gcount == 0
    for u in (c1, iso):
        assert pos[u] >= nb and gc[pos[u]] == 0
    b2 = pos[c2]
    assert b2 >= nb
    ks = gi[go[b2]: go[b2] + gc[b2]]
    assert ks[0] == 0 and k - 1 in ks.tolist()


# ---------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_wave_bitwise_reproducible(t, monkeypatch):
    """Two sweeps of the same state: the wave-class nodes' llh, best,
    gcount and gidx/gval up to gcount are bitwise equal (no float atomics
    on the wave path)."""
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "1024")
    case = cf.make_case(*t)
    cfg, st = _state(case)
    runs = []
    for _ in range(2):
        _, llh, best, pack = st.grad_ls_auto(None)
        torch.cuda.synchronize()
        nb = int(pack["n_block"])
        wave = pack["order"][nb:].long()
        gc = pack["gcount"][nb:].cpu().numpy()
        go = pack["goffset"][nb:].cpu().numpy()
        gi, gv = pack["gidx"].cpu().numpy(), pack["gval"].cpu().numpy()
        sel = np.concatenate([np.arange(o, o + c) for o, c in zip(go, gc)])
        runs.append((wave.cpu().numpy(), llh[wave].cpu().numpy(),
                     best[wave].cpu().numpy(), gc, gi[sel],
                     gv[sel].view(np.int32)))
    assert len(runs[0][0]) >= 600
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


# --------------------------------------------------------------- 4. switch
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_wave_switch_off(t, monkeypatch):
    """BIGCLAM_SPARSE_WCAP=0: every routed node runs the block kernel, in
    the order the two-class routing produced (the launch order filtered by
    bound <= cap), and the sweep meets the contract."""
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "0")
    case = cf.make_case(*t)
    cfg, st = _state(case)
    r = _check_sweep(case, cfg, st, 0, f"{case.id}/wcap0")
    assert r["nb"] == len(r["routed"])
    order = st.order.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(
        r["routed"], order[_fixture_bounds(case)[order] <= 1024])


def test_wave_cap_clamp(monkeypatch):
    """The per-wave cap is clamped in ShardState to sparse_cap and to the
    64 KB wave workgroup; the clamped value's LDS size (as the launcher
    computes it) fits."""
    from bigclam.ops import hip as hip_ops

    ext = hip_ops.ensure_loaded()
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "60000")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "50000")
    for dtype, k in (("fp32", 1000), ("bf16", 1000), ("bf16", 16385)):
        case = cf.make_case("small", "sparse", dtype, k)
        cfg = cf.regime_cfg(case.regime, k, dtype, device="cuda")
        st = ShardState(make_shard(case.graph, 0, 1), cfg, device=DEV)
        w = st.sparse_wcap
        bf = dtype == "bf16"
        assert 0 < w < 50000
        assert ext.sparse_wave_lds_bytes(bf, st.kp, w) <= 65536
        assert ext.sparse_wave_lds_bytes(bf, st.kp, w + 1) > 65536
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "128")
    assert st.sparse_wcap == 128
