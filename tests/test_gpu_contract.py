"""GPU contract tests (MI355X): every sweep-kernel template, degree class,
clamp regime and shard against the vectorised fp64 oracle.

The rules, scales and measured constants live in tests/oracle.py
(``vec_*``, ``C_GRAD/C_LLH/C_MARGIN``) and docs/kernels.md ("Numerics
contract"); the fixtures in tests/contract_fixtures.py.  The same rules are
applied to the fp32 torch reference on the CPU in tests/test_oracle.py.

Line search is judged on the kernel's OWN grad/llh (upcast), so phase B is
checked separately from phase A, and EVERY node is judged — no head count.
"""
import numpy as np
import pytest
import torch

import contract_fixtures as cf
import oracle
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def _stop_after_gpu_fault():
    """A faulted device poisons every later launch: end the session
    instead of starting more work on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def _hip():
    from bigclam.ops import hip as hip_ops

    return hip_ops, hip_ops.ensure_loaded()


def _state(case):
    cfg = cf.regime_cfg(case.regime, case.k, case.dtype, device="cuda")
    st = ShardState(make_shard(case.graph, 0, 1), cfg, device=DEV)
    st.set_local_F(torch.from_numpy(case.F0))
    return cfg, st


_Judge = cf.Judge  # moved to the shared fixtures: the CPU lockstep tests use it too


def _run_paths(case, monkeypatch, extras):
    """Every path the launchers allow at this (dtype, K)."""
    hip_ops, ext = _hip()
    cfg, st = _state(case)
    bf = case.dtype == "bf16"
    kp, n = st.kp, st.n_local
    assert kp == case.kp and st.F.shape[1] == kp
    tag = case.id
    # ---- dispatch: which path the defaults take at this K
    fused_cap = 16384 if bf else 8192
    assert st.fused_ok == (kp <= fused_cap), tag
    assert st.n_mfma == (n if (bf and kp <= 8192) else 0), tag
    assert hip_ops._use_chunked_k1(st.F) == (kp > fused_cap), tag
    J = _Judge(st.F, st.sumF, st.shard.indptr, st.shard.indices, cfg,
               case.label, case.k, case.dtype)
    args = (st.F, st.indptr, st.indices, st.sumF, st.order, cfg)

    # ---- separate K1 (one-pass template) -> K2
    g1 = l1 = None
    if (not bf) or kp <= 16384:  # the bf16 one-pass K1 stops at 16384
        monkeypatch.setenv("BIGCLAM_K1_CHUNKED", "0")
        assert not hip_ops._use_chunked_k1(st.F)
        g1, l1 = st.grad_llh()
        J.check(tag + "/k1", g1, l1)
    # ---- forced chunked K1 (kd_dot_t + kw_grad_t)
    monkeypatch.setenv("BIGCLAM_K1_CHUNKED", "1")
    assert hip_ops._use_chunked_k1(st.F)
    gc, lc = st.grad_llh()
    J.check(tag + "/k1_chunked", gc, lc)
    monkeypatch.delenv("BIGCLAM_K1_CHUNKED")
    if g1 is None:
        g1, l1 = gc, lc
    best = st.linesearch(g1, l1)
    J.check(tag + "/k2", g1, l1, best)
    if extras:
        monkeypatch.setenv("BIGCLAM_K2_NOSTAGE", "1")
        J.check(tag + "/k2_nostage", g1, l1, st.linesearch(g1, l1))
        monkeypatch.delenv("BIGCLAM_K2_NOSTAGE")
        if not bf:
            monkeypatch.setenv("BIGCLAM_K2_TILED", "1")
            J.check(tag + "/k2_tiled", g1, l1, st.linesearch(g1, l1))
            monkeypatch.delenv("BIGCLAM_K2_TILED")
    # ---- fused, direct phase B
    if kp <= fused_cap:
        g, l, b = hip_ops.fused_grad_ls(*args, n_mfma=0)
        J.check(tag + "/fused_direct", g, l, b)
    # ---- fused, MFMA phase B for every node (bf16 rounds candidates)
    if kp <= (26000 if bf else 8192):
        g, l, b = hip_ops.fused_grad_ls(*args, n_mfma=n)
        J.check(tag + "/fused_mfma", g, l, b, bf16_candidates=bf)
    # ---- the default sweep entry point takes the asserted dispatch
    g, l, b = st.fused_grad_ls_overlap(None)
    J.check(tag + "/default", g, l, b,
            bf16_candidates=bf and st.fused_ok and st.n_mfma > 0)
    # ---- K4, per node
    l4 = torch.empty(n, device=DEV, dtype=torch.float64)
    ext.llh_only(st.F, st.indptr, st.indices, st.sumF, st.order, l4,
                 cfg.min_p, cfg.max_p)
    J.check(tag + "/k4", g1, l4, check_grad=False)
    tot = float(hip_ops.full_llh(*args))
    assert abs(tot - J.o["llh"].sum()) <= (
        oracle.C_LLH * oracle.EPS32 * J.o["L"].sum()), tag + "/k4 total"


_C1 = cf.c1_cases()
# one K per dtype also runs the unstaged / tiled K2 variants
_C1_EXTRAS = {("small", "dense", "fp32", 1025), ("small", "dense", "bf16", 2049)}


@pytest.mark.parametrize("t", _C1, ids=[cf.case_id(t) for t in _C1])
def test_c1_k_matrix(t, monkeypatch):
    """Every NSLOT template of K1/KF/KF-MFMA (fp32 1/2/4/8, bf16 1/2/4/8/0),
    the generic and chunked K1, staged/unstaged K2 and K4, on the small
    degree ladder (isolated nodes, partial MFMA tiles, K tails)."""
    _run_paths(cf.make_case(*t), monkeypatch, extras=t in _C1_EXTRAS)


_C2 = cf.c2_cases()


@pytest.mark.parametrize("t", _C2, ids=[cf.case_id(t) for t in _C2])
def test_c2_degree_matrix(t, monkeypatch):
    """Hub ladder (degrees to 600: the 256-edge kw_grad_t and 512-edge
    k2_ls_tiled tiles) under the no-clamp, min_p, max_f and short-ladder
    regimes; a failure names the degree class."""
    _run_paths(cf.make_case(*t), monkeypatch, extras=True)


# ------------------------------------------------------------------ C3
@pytest.mark.parametrize("kp", [8, 2048, 2056])
@pytest.mark.parametrize("n", [1, 511, 512, 513])
def test_c3_commit(n, kp):
    """K3 (fp32, bf16) and the fused K3+colsum called directly: stripe
    boundary rows (512), k-chunk boundary (2048), both F-clamps."""
    from bigclam.config import BigClamConfig

    _, ext = _hip()
    rng = np.random.default_rng(100 * n + kp)
    lad = np.asarray(BigClamConfig().ladder(), dtype=np.float32)
    for max_f in (1000.0, 0.5):
        cfg = BigClamConfig(k=kp, max_f=max_f)
        F0 = rng.uniform(0, max_f, size=(n, kp))
        sel = rng.random((n, kp))
        F0[sel < 0.1] = 0.0
        F0[sel > 0.9] = max_f
        # gradients large enough that both clamps act at the larger steps
        grad = rng.normal(0, 4 * max_f, size=(n, kp)).astype(np.float32)
        steps = lad[rng.integers(0, 5, size=n)]
        steps[rng.random(n) < 0.4] = 0.0
        steps[-1] = 0.0
        steps[0] = 1.0
        want = oracle.vec_commit(F0, grad, steps, cfg)
        if n >= 2:
            assert (want == 0).any() and (want == max_f).any()
        gt = torch.from_numpy(grad).to(DEV)
        stt = torch.from_numpy(steps).to(DEV)
        for sd in (torch.float32, torch.bfloat16):
            Fb = torch.from_numpy(F0).to(sd).to(DEV)
            tag = f"k3-{n}x{kp}-{sd}-maxf{max_f}"
            Fa = Fb.clone()
            ext.apply_step(Fa, gt, stt, cfg.min_f, cfg.max_f)
            torch.cuda.synchronize()
            cf.assert_commit(tag, Fb, Fa, gt, stt, cfg)
            if sd == torch.bfloat16:
                Fc = Fb.clone()
                parts = torch.full(((n + 511) // 512, kp), float("nan"),
                                   device=DEV, dtype=torch.float32)
                ext.apply_step_colsum(Fc, gt, stt, parts, cfg.min_f,
                                      cfg.max_f)
                torch.cuda.synchronize()
                assert torch.equal(Fc.view(torch.int16), Fa.view(torch.int16))
                cf.assert_colsum(tag + "/colsum",
                                 parts.double().sum(0).cpu().numpy(), Fc)


# ------------------------------------------------------------------ C4
class _NoWait:
    """Stand-in halo work handle: the halo rows are already in place."""

    def wait(self):
        pass


@pytest.mark.parametrize("t", cf.c4_cases(),
                         ids=[cf.case_id(t) for t in cf.c4_cases()])
def test_c4_shards_in_one_process(t, monkeypatch):
    """world_size = 3 shards built in one process, halo rows filled by
    hand: kernels index F with halo rows, K3 leaves them alone, K6 skips
    off-shard rows.  Judged against the GLOBAL oracle's rows."""
    from bigclam.core.init import seed_init_local_F
    from bigclam.engine.extract import local_memberships, membership_threshold

    hip_ops, ext = _hip()
    case = cf.make_case(*t)
    g, k, bf = case.graph, case.k, case.dtype == "bf16"
    if not bf:
        # fp32 defaults to the direct kernel: split at degree 16 so the
        # per-subset MFMA prefixes are exercised as well
        monkeypatch.setenv("BIGCLAM_MFMA_DEG", "16")
    cfg = cf.regime_cfg(case.regime, k, case.dtype, device="cuda")
    F0 = case.stored_F()
    sumF = F0.float().sum(dim=0)
    J = _Judge(F0, sumF, g.indptr, g.indices, cfg, case.label, k, case.dtype)
    N = g.num_nodes
    out = {name: (np.zeros((N, case.kp), np.float32), np.zeros(N),
                  np.zeros(N, np.float32)) for name in ("fused", "sep")}
    k4_total = 0.0
    saw_halo = saw_split = False
    saw_prefix = bf
    rng = np.random.default_rng(5)
    seeds = rng.permutation(np.flatnonzero(g.degrees() > 0))[:k]
    delta = membership_threshold(N, g.num_edges)
    for r in range(3):
        sh = make_shard(g, r, 3)
        st = ShardState(sh, cfg, device=DEV)
        a, b, nl = sh.start, sh.stop, sh.n_local
        st.F[:nl] = F0[a:b].to(DEV)
        st.F[nl:] = F0[torch.from_numpy(sh.halo_globals)].to(DEV)
        st.sumF = sumF.to(DEV)
        F_init = st.F.clone()
        saw_halo |= sh.n_halo > 0
        split = st.order_boundary.numel() > 0 and st.order_interior.numel() > 0
        saw_split |= split
        if not bf:  # per-subset MFMA prefixes = the deg >= 16 nodes
            hi = int((sh.degrees() >= 16).sum())
            assert st.n_mfma_interior + st.n_mfma_boundary == hi
            saw_prefix |= split and 0 < hi < nl
        # fused sweep through the interior/boundary split
        gr, ll, be = st.fused_grad_ls_overlap(_NoWait())
        torch.cuda.synchronize()
        for dst, src in zip(out["fused"], (gr, ll, be)):
            dst[a:b] = src.cpu().numpy()
        # separate K1 (split) and K2
        gr2, ll2 = st.grad_llh_overlap(_NoWait())
        be2 = st.linesearch(gr2, ll2)
        torch.cuda.synchronize()
        for dst, src in zip(out["sep"], (gr2, ll2, be2)):
            dst[a:b] = src.cpu().numpy()
        # K4 of this rank (no all-reduce: one process)
        k4_total += float(hip_ops.full_llh(st.F, st.indptr, st.indices,
                                           st.sumF, st.order, cfg))
        # K7 on the shard == the torch predicate
        c_h, m_h = local_memberships(st.F_local, k, delta, use_hip=True)
        c_t, m_t = local_memberships(st.F_local_k, k, delta, use_hip=False)
        np.testing.assert_array_equal(c_h, c_t)
        np.testing.assert_array_equal(m_h, m_t)
        assert c_t.sum() > 0
        # K3 commits the owned rows and leaves halo rows bitwise unchanged
        assert torch.equal(st.F, F_init)
        if bf:
            parts = torch.empty((nl + 511) // 512, st.kp, device=DEV,
                                dtype=torch.float32)
            ext.apply_step_colsum(st.F_local, gr, be, parts, cfg.min_f,
                                  cfg.max_f)
            cf.assert_colsum(f"{case.id}/r{r}/colsum",
                             parts.double().sum(0).cpu().numpy(), st.F_local)
        else:
            hip_ops.apply_step(st.F_local, gr, be, cfg)
        torch.cuda.synchronize()
        it = torch.int16 if bf else torch.int32
        assert torch.equal(st.F[nl:].view(it), F_init[nl:].view(it)), (
            f"rank {r}: K3 touched halo rows")
        cf.assert_commit(f"{case.id}/r{r}/k3", F_init[:nl], st.F[:nl], gr, be,
                         cfg)
        assert (be > 0).any()
        # K6 at this rank == the host slice (off-shard rows skipped)
        hip_ops.seed_init_device(st, g, seeds, False)
        torch.cuda.synchronize()
        host = seed_init_local_F(g, k, a, b, seeds=seeds)
        np.testing.assert_array_equal(
            st.F_local_k.float().cpu().numpy(), host)
        assert not st.F[nl:].any() and not st.F[:, k:].any()
        if r > 0:
            assert host.any()
    assert saw_halo and saw_split and saw_prefix
    for name, bfc in (("fused", bf), ("sep", False)):
        gr, ll, be = out[name]
        tag = f"{case.id}/{name}"
        cf.assert_grad_llh(tag, J.o, g.indptr, case.label, k, gr, ll)
        cf.assert_picks(tag, J.margins(gr, ll), g.indptr, case.label, cfg,
                        case.dtype, be, bf16_candidates=bfc)
    assert abs(k4_total - J.o["llh"].sum()) <= (
        oracle.C_LLH * oracle.EPS32 * J.o["L"].sum())


# ------------------------------------------------------------------ C5
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_c5_sparse_routed_sweep(t, monkeypatch):
    """KAF/KFS/K3S on the hub ladder: ALL routed nodes against the oracle
    (llh, compact gradient at gidx, picks), then the list-based sumF and
    the rewritten support lists."""
    monkeypatch.setenv("BIGCLAM_SPARSE", "1")
    monkeypatch.setenv("BIGCLAM_SPARSE_CAP", "1024")
    case = cf.make_case(*t)
    bf = case.dtype == "bf16"
    cfg, st = _state(case)
    n, kp = st.n_local, st.kp
    J = _Judge(st.F, st.sumF, st.shard.indptr, st.shard.indices, cfg,
               case.label, case.k, case.dtype)
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None, "sparse routing did not engage"
    routed = pack["order"].cpu().numpy().astype(np.int64)
    assert len(routed) >= 64 and len(np.unique(routed)) == len(routed)
    dense = np.setdiff1d(np.arange(n), routed)
    assert len(dense) > 0  # hubs stay on the dense kernel
    # the routed nodes' gradient is compact: gval at gidx, and -sumF (with
    # fu = fv = 0 there) on every other column — rebuild the full rows
    go = pack["goffset"].cpu().numpy()
    gc = pack["gcount"].cpu().numpy()
    gi = pack["gidx"].cpu().numpy()
    gv = pack["gval"].cpu().numpy()
    full = grad.cpu().numpy().copy()
    s32 = st.sumF.cpu().numpy()
    for b, u in enumerate(routed):
        assert 0 <= gc[b] <= st.sparse_cap
        ks = gi[go[b]: go[b] + gc[b]]
        assert len(np.unique(ks)) == len(ks) and (ks < kp).all()
        full[u] = -s32
        full[u, ks] = gv[go[b]: go[b] + gc[b]]
    full_t = torch.from_numpy(full)
    flags = np.zeros(n, dtype=bool)
    flags[dense] = bf  # dense remainder: MFMA phase B on bf16
    J.check(case.id + "/sparse", full_t, llh, best, bf16_candidates=flags)
    # commit: list-based sumF refresh and rewritten support lists
    F_before = st.F_local.clone()
    st.apply_commit(grad, best, pack)
    torch.cuda.synchronize()
    cf.assert_commit(case.id + "/k3s", F_before, st.F_local, full_t, best, cfg)
    cf.assert_colsum(case.id + "/sumF", st.sumF.cpu().numpy(), st.F_local)
    assert st._kaf_valid
    # K3S rewrote the routed rows' lists in place; rows the dense kernel
    # committed are marked dirty (rescanned next sweep), the rest are
    # untouched.  Every non-dirty row must equal a full rescan.
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
    assert (scf[~fits] > cap).all()
    b_i, b_v = st._sp_sidx.cpu().numpy(), st._sp_sval.cpu().numpy()
    checked = 0
    for r in np.flatnonzero(clean & fits & (nnz > 0)):
        sl = slice(r * cap, r * cap + int(nnz[r]))
        np.testing.assert_array_equal(sidx[sl], b_i[sl])
        np.testing.assert_array_equal(sval[sl], b_v[sl])
        np.testing.assert_array_equal(np.sort(sidx[sl]), np.flatnonzero(Fh[r]))
        np.testing.assert_array_equal(sval[sl], Fh[r, sidx[sl]])
        checked += 1
    assert checked >= 64
