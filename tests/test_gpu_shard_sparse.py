"""GPU tests (MI355X) of the sparse sweep on row shards (docs/kernels.md,
C6): three ``ShardState`` ranks of the hub ladder driven in lockstep in one
process (tests/shard_lockstep.py), four sweeps, every node of every sweep
judged against the fp64 oracle of the GLOBAL state with the constants of
tests/oracle.py.

What only a sharded state reaches: the support scan of the halo section
(``F[n_loc:]`` with the full pools), KFS/KFW reading the lists of halo rows,
pools of two sizes, the commit / column sums / list-mode scan over
``F_local`` while the dirty flags cover ``n_rows``, and the halo wait in the
middle of the scan.  Every test runs with warnings as errors, so the silent
dense fallback of ``grad_ls_auto`` fails the test.

The fixture and why it differs from C5 (ladder length, seed, cap / wcap) is
described in tests/shard_lockstep.py; its conditions are asserted on the CPU
in tests/test_shard_lockstep_oracle.py and again here from the kernels' own
routing.
"""
import warnings

import numpy as np
import pytest
import torch

import contract_fixtures as cf
import shard_lockstep as sl
from test_gpu_contract import DEV, _stop_after_gpu_fault  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = sl.c6_cases()


@pytest.fixture(autouse=True)
def _warnings_are_errors():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        yield


def _env(monkeypatch, cap, wcap=None):
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", str(cap))
    if wcap is not None:
        monkeypatch.setenv("BIGCLAM_SPARSE_WCAP", str(wcap))


def _pools(st):
    torch.cuda.synchronize()
    return (st._sp_scount.cpu().numpy(), st._sp_sidx.cpu().numpy(),
            st._sp_sval.cpu().numpy())


def _check_lists(tag, st):
    """After the support scan every row of the rank's buffer — owned rows
    and, past n_local, halo rows — has the count of the row as it is in F
    now and, up to cap, its ascending columns and values."""
    sc, si, sv = _pools(st)
    Fh = st.F.float().cpu().numpy()
    assert sc.shape[0] == Fh.shape[0] > st.n_local
    cf.assert_lists(tag, Fh, range(Fh.shape[0]), sc, si, sv, st._sp_cap)
    return sc, si, sv


def _rebuild(tag, st, out):
    """Full gradient rows of one rank: the routed nodes' compact gradient
    (gval at gidx, -sumF elsewhere, as in C5), the dense class's rows of
    ``grad`` as they are."""
    grad, llh, best, pack = out
    kp = st.kp
    routed = pack["order"].cpu().numpy().astype(np.int64)
    nb = int(pack["n_block"])
    assert len(np.unique(routed)) == len(routed)
    go = pack["goffset"].cpu().numpy()
    gc = pack["gcount"].cpu().numpy()
    gi = pack["gidx"].cpu().numpy()
    gv = pack["gval"].cpu().numpy()
    full = grad.cpu().numpy().copy()
    s32 = st.sumF.cpu().numpy()
    for b, u in enumerate(routed):
        lim = st.sparse_cap if b < nb else int(pack["wcap"])
        assert 0 <= gc[b] <= lim, f"{tag}: gcount of node {u}"
        ks = gi[go[b]: go[b] + gc[b]]
        assert (np.diff(ks) > 0).all() and (ks < kp).all() and (ks >= 0).all()
        full[u] = -s32
        full[u, ks] = gv[go[b]: go[b] + gc[b]]
    return full, routed, nb


def _sweep(L, tag, stats, mode="nowait", colsum=True, grad_fn=None):
    """One lockstep sweep with every per-rank and global check of C6.
    ``mode``: "nowait" (rows in place, counting handle), "late" (halo
    section poisoned, the rows arrive inside wait()), "none" (no handle).
    Returns per rank dict(wave, block, dense, sc)."""
    case, cfg, bf = L.case, L.cfg, L.case.dtype == "bf16"
    G = L.global_F()
    info, fulls = [], []
    flags = np.zeros(case.graph.num_nodes, dtype=bool)
    for r, st in enumerate(L.states):
        nl, sh = st.n_local, st.shard
        rows = L.halo_rows(r, G)
        if mode == "late":
            st.F[nl:] = 7.0  # every column, pads included
            handle = sl.LateHalo(st.F[nl:], rows)
        else:
            st.F[nl:].copy_(rows)
            handle = sl.NoWait() if mode == "nowait" else None
        out = (grad_fn or L.grad_ls)(r, handle)
        torch.cuda.synchronize()
        rt = f"{tag}/r{r}"
        assert out[3] is not None, f"{rt}: sparse routing did not engage"
        if handle is not None:
            assert handle.calls >= 1, f"{rt}: the halo handle was not waited"
        assert torch.equal(sl.bits(st.F[nl:]), sl.bits(rows)), (
            f"{rt}: halo rows are not the owners' rows")
        assert not bool((st.F.float() == 7.0).any())
        sc, si, sv = _check_lists(rt + "/lists", st)
        cap = st._sp_cap
        cnt = np.where(sc <= cap, sc, 0)
        live = np.arange(cap)[None, :] < cnt[:, None]
        assert not (sv.reshape(-1, cap)[live] == 7.0).any(), (
            f"{rt}: a poisoned halo row reached the support lists")
        full, routed, nb = _rebuild(rt, st, out)
        fulls.append(full)
        pack = out[3]
        dense = pack["order_d"].cpu().numpy().astype(np.int64)
        wave, block = routed[nb:], routed[:nb]
        # the classes are those of the exact bound over owned AND halo rows
        em = sl.emulated_classes(st, st.sparse_cap, st.sparse_wcap)
        for name, got in (("wave", wave), ("block", block), ("dense", dense)):
            np.testing.assert_array_equal(np.sort(got), em[name],
                                          err_msg=f"{rt}: {name} class")
        assert len(routed) >= max(64, nl // 4), rt
        assert len(wave) and len(dense), rt
        hh = sl.row_has_halo(sh)
        stats["wave_halo"] += int(hh[wave].sum())
        stats["block_halo"] += int(hh[block].sum())
        stats["block_ranks"].append(int(len(block) > 0))
        best = out[2].cpu().numpy()
        stats["dense_accepted"] += int((best[dense] > 0).sum())
        flags[sh.start + dense] = bf  # dense class: MFMA phase B on bf16
        info.append(dict(wave=wave, block=block, dense=dense, sc=sc))
    # ---- every node of every rank against the oracle of the global state
    J = L.judge()
    eg, el, nd = J.check(tag, *L.stitched(grads=fulls), bf16_candidates=flags)
    stats["grad"] = max(stats["grad"], eg)
    stats["llh"] = max(stats["llh"], el)
    stats["differ"].append(nd)
    # ---- commit
    for r, st in enumerate(L.states):
        nl = st.n_local
        rt = f"{tag}/r{r}"
        grad, llh, best, pack = L.outs[r]
        F_before = st.F.clone()
        L.commit(r)
        torch.cuda.synchronize()
        assert torch.equal(sl.bits(st.F[nl:]), sl.bits(F_before[nl:])), (
            f"{rt}: the commit touched halo rows")
        cf.assert_commit(rt + "/commit", F_before[:nl], st.F_local,
                         torch.from_numpy(fulls[r]), best, cfg)
        # st.sumF is this rank's partial until reduce_sumF
        cf.assert_colsum(rt + "/partial", st.sumF.cpu().numpy(), st.F_local)
        dense = info[r]["dense"]
        want_d = np.zeros(nl, dtype=np.uint8)
        want_d[dense] = best.cpu().numpy()[dense] > 0
        np.testing.assert_array_equal(st._dirty[:nl].cpu().numpy(), want_d,
                                      err_msg=f"{rt}: dirty flags")
        assert st._dirty.numel() == st.F.shape[0] and st._kaf_valid
        if colsum:
            assert st._kaf_rows is not None, rt
            np.testing.assert_array_equal(
                st._kaf_rows.cpu().numpy().astype(np.int64), dense)
        else:
            assert st._kaf_rows is None, rt
    total = L.reduce_sumF()
    cf.assert_colsum(tag + "/sumF", total.cpu().numpy(), L.global_F())
    return info


def _stats():
    return dict(wave_halo=0, block_halo=0, block_ranks=[], dense_accepted=0,
                grad=0.0, llh=0.0, differ=[])


# ------------------------------------------------------------- 1. sweeps
@pytest.mark.parametrize("config", list(sl.CONFIGS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_shard_sparse_sweeps(dtype, config, monkeypatch):
    """Four routed sweeps on three shards at both cap / wcap settings."""
    cap, wcap = sl.CONFIGS[config]
    _env(monkeypatch, cap, wcap)
    case = sl.c6_case(dtype)
    L = sl.Lockstep(case, device=DEV)
    assert [st.n_local for st in L.states] == [190, 181, 256]
    assert [st.shard.n_halo for st in L.states] == [370, 383, 369]
    stats = _stats()
    nnz = [(L.global_F().float() != 0).sum(dim=1).cpu().numpy()]
    for i in range(sl.SWEEPS):
        for st in L.states:  # sweep 0: full grid; later: the list mode
            assert (st._kaf_rows is None) == (i == 0)
        _sweep(L, f"{case.id}/{config}/sweep{i}", stats)
        assert sum(stats["block_ranks"][-sl.WORLD:]) >= 2
        nnz.append((L.global_F().float() != 0).sum(dim=1).cpu().numpy())
        assert (nnz[-1] > nnz[-2]).sum() >= 20, "too few rows grew"
        assert (nnz[-1] < nnz[-2]).sum() >= 20, "too few rows shrank"
    print(f"{case.id}/{config}: max grad {stats['grad']:.1f} llh "
          f"{stats['llh']:.1f} picks differing {stats['differ']}")
    assert stats["wave_halo"] >= 20 and stats["block_halo"] >= 20
    if config == "tight":
        assert stats["dense_accepted"] >= 1


# ---------------------------------------------------------- 2. late halo
@pytest.mark.parametrize("mode", ["late", "none"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_late_halo(dtype, mode, monkeypatch):
    """The halo section holds 7.0 in every column until the handle's
    ``wait()`` copies the true rows in: sweep 0 takes the full-grid branch
    with a handle, sweep 1 the list-mode branch; ``mode="none"`` is the
    remaining branch (no handle, rows installed beforehand).  A scan of the
    halo section before the wait would put 512-entry lists of 7.0 (under
    the cap of 4096) into the pools."""
    cap, wcap = sl.CONFIGS["wide"]
    _env(monkeypatch, cap, wcap)
    case = sl.c6_case(dtype)
    L = sl.Lockstep(case, device=DEV)
    stats = _stats()
    for i in range(2):
        for st in L.states:
            assert (st._kaf_rows is None) == (i == 0)
        _sweep(L, f"{case.id}/{mode}/sweep{i}", stats, mode=mode)


# ------------------------------------------------------ 3. over-cap halo
@pytest.mark.parametrize("dtype", DTYPES)
def test_over_cap_halo(dtype, monkeypatch):
    """Leaf rows densified to 400 non-zeros at cap 256: their halo copies
    carry the full count and no list, and every owned neighbour of one is
    in the dense class."""
    _env(monkeypatch, sl.OVER_CAP)
    case = sl.over_cap_case(dtype)
    L = sl.Lockstep(case, device=DEV)
    stats = _stats()
    info = _sweep(L, f"{case.id}/over-cap", stats)
    leaves = set(sl.over_cap_leaves())
    for r, st in enumerate(L.states):
        nl, sh = st.n_local, st.shard
        assert st._sp_cap == sl.OVER_CAP
        sc = info[r]["sc"]
        over = np.flatnonzero(sc[nl:] > sl.OVER_CAP) + nl
        assert len(over) >= 3
        assert set(sh.halo_globals[over - nl].tolist()) <= leaves
        assert (sc[over] == sl.OVER_NNZ).all()
        src = np.repeat(np.arange(nl), np.diff(sh.indptr))
        nb = np.unique(src[np.isin(sh.indices, over)])
        assert len(nb) and np.isin(nb, info[r]["dense"]).all()


# ------------------------------------------------------------ 4. switches
def _snapshot(out):
    grad, llh, best, pack = out
    torch.cuda.synchronize()
    return dict(
        order=pack["order"].cpu().numpy(), nb=int(pack["n_block"]),
        order_d=pack["order_d"].cpu().numpy(),
        go=pack["goffset"].cpu().numpy(), gc=pack["gcount"].cpu().numpy(),
        gi=pack["gidx"].cpu().numpy(), gv=pack["gval"].cpu().numpy(),
        llh=llh.cpu().numpy(), best=best.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_and_colsum_switches(dtype, monkeypatch):
    """The first two sweeps again with the torch routing and with the
    dense column-sum fallback."""
    cap, wcap = sl.CONFIGS["tight"]
    _env(monkeypatch, cap, wcap)
    case = sl.c6_case(dtype)
    # ---- BIGCLAM_NATIVE_ROUTE=0 on the SAME state as the native routing
    # (the block class has float atomics, so two separate runs need not
    # hold bitwise equal F in sweep 1): same order, n_block and order_d,
    # and the wave class bitwise equal; the sweep then commits the
    # torch-routed pack.
    L = sl.Lockstep(case, device=DEV)

    def both(r, handle):
        st = L.states[r]
        assert st.native_route
        a = _snapshot(L.grad_ls(r, handle))
        monkeypatch.setenv("BIGCLAM_NATIVE_ROUTE", "0")
        assert not st.native_route
        out = L.grad_ls(r, handle)
        monkeypatch.delenv("BIGCLAM_NATIVE_ROUTE")
        b = _snapshot(out)
        np.testing.assert_array_equal(a["order"], b["order"])
        assert a["nb"] == b["nb"]
        np.testing.assert_array_equal(a["order_d"], b["order_d"])
        nb = a["nb"]
        wave = a["order"][nb:].astype(np.int64)
        assert len(wave)
        np.testing.assert_array_equal(a["go"], b["go"])
        np.testing.assert_array_equal(a["gc"][nb:], b["gc"][nb:])
        sel = np.concatenate(
            [np.arange(o, o + c) for o, c in zip(a["go"][nb:], a["gc"][nb:])]
        ).astype(np.int64)
        np.testing.assert_array_equal(a["gi"][sel], b["gi"][sel])
        np.testing.assert_array_equal(a["gv"][sel].view(np.int32),
                                      b["gv"][sel].view(np.int32))
        np.testing.assert_array_equal(a["llh"][wave].view(np.int64),
                                      b["llh"][wave].view(np.int64))
        np.testing.assert_array_equal(a["best"][wave].view(np.int32),
                                      b["best"][wave].view(np.int32))
        return out

    stats = _stats()
    for i in range(2):
        _sweep(L, f"{case.id}/torch-route/sweep{i}", stats, grad_fn=both)
    # ---- BIGCLAM_SPARSE_COLSUM=0: full-grid dense commit, torch-written
    # dirty flags, no row list; the lists are still current after the next
    # scan (the third one included)
    monkeypatch.setenv("BIGCLAM_SPARSE_COLSUM", "0")
    L = sl.Lockstep(case, device=DEV)
    stats = _stats()
    for i in range(2):
        for st in L.states:
            assert st._kaf_rows is None
        _sweep(L, f"{case.id}/colsum0/sweep{i}", stats, colsum=False)
    L.exchange()
    for r, st in enumerate(L.states):
        assert L.grad_ls(r, sl.NoWait())[3] is not None
        _check_lists(f"{case.id}/colsum0/after/r{r}", st)
    assert stats["dense_accepted"] >= 1
