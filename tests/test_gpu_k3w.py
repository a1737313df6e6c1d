"""GPU tests (MI355X) of the one-wave-per-node sparse commit (K3W), the
list modes of the dense commit (K3) and of the support scan (KAF), and the
state plumbing that keeps the persistent support lists current without a
full-grid launch.

Every comparison here is exact (atol = 0): the commit is element-wise
(fmaf, v_med3_f32, RNE pack), so the wave commit, the block commit and the
listed dense commit must agree bit for bit; F itself is also held to the
fp64 oracle by ``cf.assert_commit`` (tests/oracle.py, docs/kernels.md
"Numerics contract").
"""
import numpy as np
import pytest
import torch

import contract_fixtures as cf
from bigclam.config import BigClamConfig
from test_gpu_contract import (DEV, _hip, _state,  # noqa: F401
                               _stop_after_gpu_fault)

pytestmark = pytest.mark.gpu

CAP = 1024
SENT_I = -77  # sentinel for scount / sidx slots nobody may write
SENT_V = -77.0
SENT_D = 7  # sentinel dirty flag


def _sd(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _bits(F):
    return F.view(torch.int16 if F.dtype == torch.bfloat16 else torch.int32)


_rescan = cf.rescan  # moved to the shared fixtures (sharded tests)
_assert_lists = cf.assert_lists


# ------------------------------------------- 1. wave commit == block commit
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_wave_commit_equals_block_commit(t, monkeypatch):
    """One sweep's pack (every routed node in the wave class, so every
    gcount <= 1024) committed twice on clones: all K3S and all K3W."""
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", str(CAP))
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", str(CAP))
    case = cf.make_case(*t)
    cfg, st = _state(case)
    _, ext = _hip()
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None and int(pack["n_block"]) == 0
    n, kp, cap = st.n_local, st.kp, st._sp_cap
    assert cap == CAP
    order = pack["order"]
    routed = order.cpu().numpy().astype(np.int64)
    n_s = len(routed)
    assert n_s >= 600
    gc = pack["gcount"].cpu().numpy()
    go = pack["goffset"].cpu().numpy()
    gi = pack["gidx"].cpu().numpy()
    gv = pack["gval"].cpu().numpy()
    print(f"{case.id}: {n_s} routed, gcount max {gc.max()}")
    assert 64 < gc.max() <= CAP  # several ballot rounds
    # some routed rows rejected, most accepted; dense rows are not
    # committed here (their step is zeroed for the oracle check too)
    steps = best.clone()
    steps[order[::5].long()] = 0.0
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[order.long()] = True
    steps[~mask] = 0.0
    s_np = steps.cpu().numpy()
    assert (s_np[routed] > 0).sum() >= 64 and (s_np[routed] == 0).sum() >= 64

    def commit(n_block):
        F = st.F_local.clone()
        sidx, sval = st._sp_sidx.clone(), st._sp_sval.clone()
        scount = st._sp_scount.clone()
        dirty = torch.full((st.F.shape[0],), SENT_D, device=DEV,
                           dtype=torch.uint8)
        ext.sparse_commit(F, order, pack["goffset"], pack["gidx"],
                          pack["gval"], pack["gcount"], steps,
                          st._sp_soffset, sidx, sval, scount, cap, cfg.min_f,
                          cfg.max_f, n_block, CAP, dirty)
        torch.cuda.synchronize()
        return F, sidx.cpu().numpy(), sval.cpu().numpy(), \
            scount.cpu().numpy(), dirty.cpu().numpy()

    F_before = st.F_local.clone()
    sc_before = st._sp_scount.cpu().numpy()
    Fb, ib, vb, cb, db = commit(n_s)  # all K3S
    Fw, iw, vw, cw, dw = commit(0)  # all K3W
    assert torch.equal(_bits(Fb), _bits(Fw))
    np.testing.assert_array_equal(cb, cw)
    np.testing.assert_array_equal(db, dw)
    assert (dw[routed] == 0).all()
    unrouted = np.setdiff1d(np.arange(st.F.shape[0]), routed)
    assert (dw[unrouted] == SENT_D).all()
    for r in routed:
        sl = slice(r * cap, r * cap + int(cw[r]))
        np.testing.assert_array_equal(ib[sl], iw[sl])
        np.testing.assert_array_equal(vb[sl].view(np.int32),
                                      vw[sl].view(np.int32))
    # rows with step 0: F, count and list bitwise untouched
    idle = np.flatnonzero(s_np <= 0)
    assert torch.equal(_bits(Fw)[idle], _bits(F_before)[idle])
    np.testing.assert_array_equal(cw[idle], sc_before[idle])
    i0, v0 = st._sp_sidx.cpu().numpy(), st._sp_sval.cpu().numpy()
    for r in idle:
        if 0 < sc_before[r] <= cap:
            sl = slice(r * cap, r * cap + int(sc_before[r]))
            np.testing.assert_array_equal(iw[sl], i0[sl])
            np.testing.assert_array_equal(vw[sl].view(np.int32),
                                          v0[sl].view(np.int32))
    # F against the fp64 oracle, lists against a rescan of the new F
    full = np.zeros((n, kp), dtype=np.float32)
    s32 = st.sumF.cpu().numpy()
    for b, u in enumerate(routed):
        full[u] = -s32
        full[u, gi[go[b]: go[b] + gc[b]]] = gv[go[b]: go[b] + gc[b]]
    cf.assert_commit(case.id + "/k3w", F_before, Fw, torch.from_numpy(full),
                     steps, cfg)
    Fh = Fw.float().cpu().numpy()
    _assert_lists(case.id + "/k3w", Fh, routed[s_np[routed] > 0], cw, iw, vw,
                  cap)


# --------------------------------------------------- 2. hand-built packs
NS_ALL = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)


def _hand_commit(ext, k, dtype, ns_list, mode, seed):
    """Commit one hand-built wave-class pack (no sweep): rows 1..n_wave of
    an (n_wave + 2)-row F are routed in reversed order, row 0 and the last
    row are bystanders.  Returns what the checks need."""
    kp = cf.padded_k(k, dtype)
    max_f = 0.5 if mode == "capped" else 1000.0
    cfg = BigClamConfig(k=k, dtype=dtype, max_f=max_f)
    lad = np.asarray(cfg.ladder(), dtype=np.float32)
    rng = np.random.default_rng(seed)
    n_wave = len(ns_list)
    n_rows = n_wave + 2
    hi = 0.5 if mode == "capped" else 2.0
    F0 = rng.uniform(0.05, hi, size=(n_rows, kp))
    F0[rng.random((n_rows, kp)) < 0.5] = 0.0
    if mode == "capped":
        F0[rng.random((n_rows, kp)) < 0.1] = 0.5
    F0[:, k:] = 0.0
    order = np.arange(n_wave, 0, -1).astype(np.int32)  # rows n_wave .. 1
    # active sets: ascending, columns 0 and K-1 always in when ns >= 2; a
    # routed row's support lies inside its active set (S_u ⊇ supp(F_u))
    active = []
    for b, u in enumerate(order):
        ns = int(ns_list[b])
        assert ns <= k
        if ns >= 2:
            mid = rng.choice(np.arange(1, k - 1), size=ns - 2, replace=False)
            ks = np.sort(np.concatenate([[0, k - 1], mid]))
        else:
            ks = np.sort(rng.choice(k, size=ns, replace=False))
        active.append(ks.astype(np.int64))
        off = np.ones(kp, dtype=bool)
        off[ks] = False
        F0[u, off] = 0.0
    Ft = torch.from_numpy(F0).to(_sd(dtype))
    F0 = Ft.float().numpy()
    # steps cycle through {1, smallest rung, 0}; position 0 always accepts
    choice = (lad[0], lad[-1], 0.0)
    steps = np.zeros(n_rows, dtype=np.float32)
    steps[:] = lad[3]  # bystanders hold a positive step: must be ignored
    for b, u in enumerate(order):
        steps[u] = choice[(b + seed) % 3] if b else lad[0]
    gidx = np.full(n_wave * CAP, SENT_I, dtype=np.int32)
    gval = np.full(n_wave * CAP, np.nan, dtype=np.float32)
    gcount = np.asarray(ns_list, dtype=np.int32)
    goffset = np.arange(n_wave, dtype=np.int64) * CAP
    full = np.zeros((n_rows, kp), dtype=np.float32)
    for b, u in enumerate(order):
        ns, ks = int(ns_list[b]), active[b]
        s = max(float(steps[u]), float(lad[-1]))
        if mode == "zero":  # every entry clamps to zero
            g = -(F0[u, ks] + 1.0) / s
        elif mode == "capped":  # entries land exactly on 0 and on 0.5
            g = rng.choice([-2.0, 2.0, 0.25], size=ns) / s
        else:
            g = rng.normal(0, 1.5, size=ns) / s
            g[rng.random(ns) < 0.3] = -4.0 / s  # clamp to zero
        gidx[b * CAP: b * CAP + ns] = ks
        gval[b * CAP: b * CAP + ns] = g
        full[u, ks] = g.astype(np.float32)
    soffset = torch.arange(n_rows, dtype=torch.int64) * CAP
    sidx = torch.full((n_rows * CAP,), SENT_I, dtype=torch.int32)
    sval = torch.full((n_rows * CAP,), SENT_V, dtype=torch.float32)
    scount = torch.full((n_rows,), SENT_I, dtype=torch.int32)
    dirty = torch.full((n_rows,), SENT_D, dtype=torch.uint8)
    Fd = Ft.clone().to(DEV)
    dev = [torch.from_numpy(a).to(DEV)
           for a in (order, goffset, gidx, gval, gcount, steps)]
    out = [a.to(DEV) for a in (soffset, sidx, sval, scount, dirty)]
    ext.sparse_commit(Fd, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5],
                      out[0], out[1], out[2], out[3], CAP, cfg.min_f,
                      cfg.max_f, 0, CAP, out[4])
    torch.cuda.synchronize()
    return dict(cfg=cfg, F_before=Ft, F_after=Fd.cpu(), full=full,
                steps=steps, order=order, sidx=out[1].cpu().numpy(),
                sval=out[2].cpu().numpy(), scount=out[3].cpu().numpy(),
                dirty=out[4].cpu().numpy(), n_rows=n_rows)


def _check_hand(tag, r, mode):
    order, steps = r["order"], r["steps"]
    # only routed rows commit: the bystanders' positive steps are ignored
    s_eff = np.zeros_like(steps)
    s_eff[order] = steps[order]
    cf.assert_commit(tag, r["F_before"], r["F_after"],
                     torch.from_numpy(r["full"]), torch.from_numpy(s_eff),
                     r["cfg"])
    Fh = r["F_after"].float().numpy()
    sidx, sval, scount = r["sidx"], r["sval"], r["scount"]
    acc = [int(u) for u in order if steps[u] > 0]
    _assert_lists(tag, Fh, acc, scount, sidx, sval, CAP)
    for u in range(r["n_rows"]):
        if u in acc:
            c = int(scount[u])
            assert (np.diff(sidx[u * CAP: u * CAP + c]) > 0).all()
            if mode == "zero":
                assert c == 0 and not Fh[u][r["full"][u] != 0].any()
        else:
            # rejected and bystander rows: count and whole slot untouched
            c = 0
            assert scount[u] == SENT_I, f"{tag}: row {u} count written"
        tail = slice(u * CAP + c, (u + 1) * CAP)
        assert (sidx[tail] == SENT_I).all(), f"{tag}: row {u} slot"
        assert (sval[tail] == SENT_V).all(), f"{tag}: row {u} slot"
    want_d = np.full(r["n_rows"], SENT_D, dtype=np.uint8)
    want_d[order] = 0  # every routed position, accepted or not
    np.testing.assert_array_equal(r["dirty"], want_d)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n_wave", [1, 3, 4, 5])
@pytest.mark.parametrize("k", [33, 1000])
def test_wave_commit_edge_shapes(k, n_wave, dtype):
    """Ballot-round boundaries (ns 63/64/65 ... 257, 1000 = 16 rounds),
    tail waves of the last block (n_wave 1, 3, 4, 5), columns 0 and K-1,
    steps {1, smallest rung, 0}; then every entry clamping to zero, and
    max_f = 0.5 with entries landing exactly on 0 and 0.5."""
    _, ext = _hip()
    ns_all = [v for v in NS_ALL if v <= k] + ([32, 33] if k == 33 else [])
    groups = [[ns_all[(g + j) % len(ns_all)] for j in range(n_wave)]
              for g in range(0, len(ns_all), n_wave)]
    assert {v for g in groups for v in g} == set(ns_all)
    for gi_, ns_list in enumerate(groups):
        tag = f"k3w-hand-k{k}-{dtype}-w{n_wave}-g{gi_}"
        r = _hand_commit(ext, k, dtype, ns_list, "mixed", seed=gi_)
        _check_hand(tag, r, "mixed")
    # largest active sets, position 0 (which always takes step 1) first
    top = sorted((ns_all * n_wave)[-n_wave:], reverse=True)
    r = _hand_commit(ext, k, dtype, top, "zero", seed=11)
    _check_hand(f"k3w-zero-k{k}-{dtype}-w{n_wave}", r, "zero")
    r = _hand_commit(ext, k, dtype, top, "capped", seed=12)
    _check_hand(f"k3w-capped-k{k}-{dtype}-w{n_wave}", r, "capped")
    u0 = int(r["order"][0])  # step 1: the +-2/s gradients saturate
    row = r["F_after"].float().numpy()[u0]
    touched = r["full"][u0] != 0
    assert (row[touched] == 0).any() and (row[touched] == 0.5).any()


# --------------------------------------------------- 3. listed dense commit
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kp", [8, 2048, 2056])
def test_listed_dense_commit(kp, dtype):
    """K3 in list mode against the five-argument call with the steps masked
    to the list: listed rows bitwise equal, unlisted rows bitwise unchanged
    although all eight steps are positive, dirty = (s > 0) at listed rows."""
    _, ext = _hip()
    n = 8
    rng = np.random.default_rng(kp)
    cfg = BigClamConfig(k=kp, dtype=dtype)
    lad = np.asarray(cfg.ladder(), dtype=np.float32)
    F0 = rng.uniform(0, 2.0, size=(n, kp))
    F0[rng.random((n, kp)) < 0.3] = 0.0
    Fb = torch.from_numpy(F0).to(_sd(dtype)).to(DEV)
    grad = torch.from_numpy(
        rng.normal(0, 3.0, size=(n, kp)).astype(np.float32)).to(DEV)
    all_pos = lad[rng.integers(0, 5, size=n)]
    for rows in ([], [5], [6, 0, 3]):
        for reject in (False, True):
            if reject and not rows:
                continue
            steps = all_pos.copy()
            if reject:
                steps[rows[-1]] = 0.0  # a listed row that accepted no step
            st_t = torch.from_numpy(steps).to(DEV)
            masked = np.zeros(n, dtype=np.float32)
            masked[rows] = steps[rows]
            want = Fb.clone()
            ext.apply_step(want, grad, torch.from_numpy(masked).to(DEV),
                           cfg.min_f, cfg.max_f)
            got = Fb.clone()
            dirty = torch.full((n,), SENT_D, device=DEV, dtype=torch.uint8)
            rl = torch.tensor(rows, dtype=torch.int32, device=DEV)
            ext.apply_step(got, grad, st_t, cfg.min_f, cfg.max_f, rows=rl,
                           dirty=dirty)
            torch.cuda.synchronize()
            tag = f"k3-list-{kp}-{dtype}-{rows}-{reject}"
            assert torch.equal(_bits(got), _bits(want)), tag
            unl = np.setdiff1d(np.arange(n), rows)
            assert torch.equal(_bits(got)[unl], _bits(Fb)[unl]), tag
            if rows and not reject:
                assert not torch.equal(_bits(got)[rows], _bits(Fb)[rows])
            want_d = np.full(n, SENT_D, dtype=np.uint8)
            want_d[rows] = steps[rows] > 0
            np.testing.assert_array_equal(dirty.cpu().numpy(), want_d, tag)
            cf.assert_commit(tag, Fb, got, grad, torch.from_numpy(masked),
                             cfg)


# ------------------------------------------------------- 4. list-mode KAF
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_listed_support_scan(dtype):
    """KAF over a row list: listed dirty rows equal a full scan; listed
    clean rows and unlisted rows keep their sentinels; an over-cap listed
    row gets a count only; an empty list is a no-op."""
    _, ext = _hip()
    n, kp, cap = 8, 264, 64
    rng = np.random.default_rng(5)
    F0 = rng.uniform(0.1, 2.0, size=(n, kp))
    F0[rng.random((n, kp)) < 0.9] = 0.0
    F0[2] = 0.0  # an all-zero listed row
    F0[4, :100] = 1.0  # over cap
    F0[6, 0] = 0.5
    F0[6, kp - 1] = 0.25
    F = torch.from_numpy(F0).to(_sd(dtype)).to(DEV)
    Fh = F.float().cpu().numpy()
    nnz = (Fh != 0).sum(axis=1)
    assert nnz[4] > cap and (np.delete(nnz, 4) <= cap).all()
    soffset = torch.arange(n, device=DEV, dtype=torch.int64) * cap
    none = torch.empty(0, device=DEV, dtype=torch.uint8)

    def fresh():
        return (torch.full((n,), SENT_I, device=DEV, dtype=torch.int32),
                torch.full((n * cap,), SENT_I, device=DEV, dtype=torch.int32),
                torch.full((n * cap,), SENT_V, device=DEV,
                           dtype=torch.float32))

    sc_f, si_f, sv_f = fresh()
    ext.sparse_support(F, soffset, sc_f, si_f, sv_f, cap, True, none)
    listed = [6, 1, 4, 2, 3]
    dirty = torch.zeros(n, device=DEV, dtype=torch.uint8)
    dirty[[6, 4, 2, 1, 7]] = 1  # 3 listed but clean; 7 dirty but unlisted
    sc, si, sv = fresh()
    rl = torch.tensor(listed, dtype=torch.int32, device=DEV)
    ext.sparse_support(F, soffset, sc, si, sv, cap, True, dirty, rows=rl)
    torch.cuda.synchronize()
    sc_n, si_n, sv_n = (a.cpu().numpy() for a in (sc, si, sv))
    scf, sif, svf = (a.cpu().numpy() for a in (sc_f, si_f, sv_f))
    np.testing.assert_array_equal(scf, nnz)
    for r in range(n):
        sl = slice(r * cap, (r + 1) * cap)
        if r in (6, 1, 2):  # listed and dirty: equal to the full scan
            assert sc_n[r] == nnz[r]
            np.testing.assert_array_equal(si_n[sl], sif[sl])
            np.testing.assert_array_equal(sv_n[sl], svf[sl])
            ks, vs = _rescan(Fh, r)
            np.testing.assert_array_equal(si_n[sl][: len(ks)], ks)
            np.testing.assert_array_equal(sv_n[sl][: len(ks)], vs)
        elif r == 4:  # over cap: the count, no list entry
            assert sc_n[r] == nnz[r]
            assert (si_n[sl] == SENT_I).all() and (sv_n[sl] == SENT_V).all()
        else:  # listed clean (3) and unlisted (0, 5, 7)
            assert sc_n[r] == SENT_I
            assert (si_n[sl] == SENT_I).all() and (sv_n[sl] == SENT_V).all()
    # empty list: nothing launched, nothing written — with and without mask
    for d in (dirty.fill_(1), none):
        sc, si, sv = fresh()
        ext.sparse_support(F, soffset, sc, si, sv, cap, True, d,
                           rows=rl[:0])
        torch.cuda.synchronize()
        assert (sc == SENT_I).all() and (si == SENT_I).all()
        assert (sv == SENT_V).all()


# --------------------------------------- 5. lists stay current across sweeps
def _check_state_lists(tag, st):
    n, cap = st.n_local, st._sp_cap
    Fh = st.F_local.float().cpu().numpy()
    nnz = (Fh != 0).sum(axis=1)
    fits = np.flatnonzero(nnz <= cap)
    _assert_lists(tag, Fh, fits, st._sp_scount.cpu().numpy()[:n],
                  st._sp_sidx.cpu().numpy(), st._sp_sval.cpu().numpy(), cap)
    return len(fits)


@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_lists_current_across_sweeps(t, monkeypatch):
    """Three routed sweeps with both routed classes and a non-empty dense
    class, then a pack-less dense commit (the untrusted-list fallback) and
    one more routed sweep.  After every commit + support scan the counts
    and lists of every local row with nnz <= cap equal numpy's, and sumF
    equals the column sums of F."""
    # cap 4096: the first commit fills the rows in (median bound 180 ->
    # ~2200, q90 ~5800), and at cap 1024 too few nodes route from the
    # second sweep on for the sparse path to engage.  At 4096 every sweep
    # routes ~480 of 627 nodes, a few of them in the wave class, and
    # leaves ~140 to the dense class.
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "4096")
    monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", "64")
    case = cf.make_case(*t)
    cfg, st = _state(case)
    n = st.n_local
    grad, llh, best, pack = st.grad_ls_auto(None)
    dense_accepted = 0
    for i in range(3):
        assert pack is not None, "sparse routing did not engage"
        nb, n_s = int(pack["n_block"]), int(pack["order"].numel())
        # both routed classes and a dense class, every sweep
        assert 0 < nb < n_s and pack["order_d"].numel() > 0
        order_d = pack["order_d"].long()
        dense_accepted += int((best[order_d] > 0).sum())
        st.apply_commit(grad, best, pack)
        torch.cuda.synchronize()
        tag = f"{case.id}/sweep{i}"
        cf.assert_colsum(tag + "/sumF", st.sumF.cpu().numpy(), st.F_local)
        # the dirty flags without a torch write: dense-class accepted rows
        want_d = np.zeros(n, dtype=np.uint8)
        od = order_d.cpu().numpy()
        want_d[od] = best[order_d].cpu().numpy() > 0
        np.testing.assert_array_equal(st._dirty[:n].cpu().numpy(), want_d)
        assert st._kaf_rows is not None  # the next scan runs in list mode
        grad, llh, best, pack = st.grad_ls_auto(None)
        torch.cuda.synchronize()
        assert _check_state_lists(tag, st) >= 600
    assert dense_accepted > 0, "no dense-class row accepted a step"
    # untrusted list: a dense sweep committed without a pack
    g, l, b = st.fused_grad_ls_overlap(None)
    st.apply_commit(g, b, None)
    torch.cuda.synchronize()
    assert int((b > 0).sum()) > 0
    assert st._kaf_rows is None  # the next scan falls back to the full grid
    cf.assert_colsum(case.id + "/dense/sumF", st.sumF.cpu().numpy(),
                     st.F_local)
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None
    assert _check_state_lists(case.id + "/after-dense", st) >= 600
    st.apply_commit(grad, best, pack)
    torch.cuda.synchronize()
    cf.assert_colsum(case.id + "/last/sumF", st.sumF.cpu().numpy(),
                     st.F_local)
    st.grad_ls_auto(None)
    torch.cuda.synchronize()
    _check_state_lists(case.id + "/last", st)
