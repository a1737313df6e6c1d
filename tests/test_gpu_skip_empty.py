"""GPU tests (MI355X) of the empty-item rule of the sparse sweep: an edge
with an empty neighbour list, a node with an empty active set and a
rejected node in the wave commit cost a lane-parallel test, not a walk —
and change no result.  The list-based column sum is held to its contract
on empty, dirty and over-cap rows as well.

KFW / KFP: BIGCLAM_SPARSE_SKIP=1 against =0, exact equality on every routed
output and on the committed F and lists (the _snapshot / _assert_same
pattern of tests/test_gpu_kfp_pack.py); the fp64 oracle rules of C5 run on
the SKIP=1 sweep as well.  K3W against K3S on the same pack: exact
equality.  kcs_lists_t: the column-sum rule of the contract, and exact
equality where a column has at most one contributor.  The states come from
tests/skip_fixtures.py (checked on the CPU in
tests/test_skip_fixtures_cpu.py).
"""
import numpy as np
import pytest
import torch

import contract_fixtures as cf
import kfp_fixtures as kf
import skip_fixtures as sf
from test_gpu_contract import (DEV, _hip, _state,  # noqa: F401
                               _stop_after_gpu_fault)
from test_gpu_kfp_pack import _assert_same, _env, _snapshot
from test_gpu_kfs_wave import _check_sweep

pytestmark = pytest.mark.gpu


def _on_off(case, monkeypatch, qcap, wcap=1024, cap=1024, **kw):
    """(SKIP=0 snapshot, SKIP=1 snapshot, SKIP=1 meta) of fresh states."""
    _env(monkeypatch, qcap, wcap, cap)
    monkeypatch.setenv("BIGCLAM_SPARSE_SKIP", "0")
    ref, meta0 = _snapshot(case, **kw)
    assert not meta0["st"].sparse_skip
    monkeypatch.setenv("BIGCLAM_SPARSE_SKIP", "1")
    got, meta = _snapshot(case, **kw)
    assert meta["st"].sparse_skip
    assert meta["n_pack"] == meta0["n_pack"]
    return ref, got, meta


def _oracle(case, monkeypatch, qcap, tag):
    """The C5 oracle rules on a SKIP=1 sweep of a fresh state."""
    _env(monkeypatch, qcap)
    monkeypatch.setenv("BIGCLAM_SPARSE_SKIP", "1")
    cfg, st = _state(case)
    assert st.sparse_skip
    return _check_sweep(case, cfg, st, st.sparse_wcap, tag)


# ------------------------------------------------------ 1. bitwise on / off
@pytest.mark.parametrize("qcap", [64, 0])
@pytest.mark.parametrize("t", cf.c5_cases(),
                         ids=[cf.case_id(t) for t in cf.c5_cases()])
def test_skip_bitwise_c5(t, qcap, monkeypatch):
    """Hub ladder, K=512, sparse, WCAP 1024: packed + single (QCAP 64) and
    all single (QCAP 0)."""
    ref, got, meta = _on_off(cf.make_case(*t), monkeypatch, qcap)
    assert (meta["n_pack"] > 0) == (qcap > 0)
    _assert_same(ref, got)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("k,qcap", [(33, 64), (33, 0), (1000, 1000),
                                    (1000, 0)])
def test_skip_bitwise_small(k, qcap, dtype, monkeypatch):
    """Small ladder with the hand-set rows (an edge whose both ends are
    zero, an isolated zero node): partly used bitmap words."""
    case, hand = kf.edge_case(dtype, k)
    ref, got, meta = _on_off(case, monkeypatch, qcap)
    _assert_same(ref, got)
    pos = {int(u): i for i, u in enumerate(got["order"])}
    assert got["gc"][pos[hand["c1"]]] == 0 and got["gc"][pos[hand["iso"]]] == 0


# ------------------------------------------------------- 2. mixed content
@pytest.mark.parametrize("qcap", [sf.QCAP, 0])
@pytest.mark.parametrize("stride", [2, 8])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_skip_mixed_edges(dtype, stride, qcap, monkeypatch):
    """Empty and non-empty edges interleaved, packed nodes with bound 0
    next to live ones in every group position, a tail quad."""
    case, info = sf.mixed_case(dtype, stride)
    ref, got, meta = _on_off(case, monkeypatch, qcap)
    if qcap:
        assert meta["n_pack"] == len(info["order"])
        ws = meta["st"]._wave_split[0].cpu().numpy()[: meta["n_pack"]]
        np.testing.assert_array_equal(
            got["order"].astype(np.int64)[ws], info["order"])
    _assert_same(ref, got)
    pos = {int(u): i for i, u in enumerate(got["order"])}
    zero = np.flatnonzero(info["bound"] == 0)
    assert all(got["gc"][pos[int(u)]] == 0 for u in zero)
    # the oracle rules on the same edge pattern without the bound-0 run
    # (sf.mixed_case: those nodes are degenerate for the pick statistic)
    plain, _ = sf.mixed_case(dtype, stride, quads=False)
    _oracle(plain, monkeypatch, qcap, f"{case.id}/mixed{stride}/q{qcap}")


@pytest.mark.parametrize("d,p", sf.SURVIVORS,
                         ids=[f"deg{d}-pos{p}" for d, p in sf.SURVIVORS])
def test_skip_lone_edge(d, p, monkeypatch):
    """All leaves zero but one: the centre's only non-empty edge at a named
    CSR position (lane 0, both sides of the accumulator classes, the last
    lane, both sides of the 64-edge chunk, the hub's far edges)."""
    for dtype in ("fp32", "bf16"):
        case, info = sf.survivor_case(dtype, d, p)
        ref, got, meta = _on_off(case, monkeypatch, sf.QCAP)
        _assert_same(ref, got)
        c = info["centre"]
        pos = {int(u): i for i, u in enumerate(got["order"])}
        ws = meta["st"]._wave_split[0].cpu().numpy()[: meta["n_pack"]]
        packed = set(got["order"].astype(np.int64)[ws].tolist())
        assert (c in packed) == (d <= 16)
        assert got["gc"][pos[c]] > 0
    _oracle(case, monkeypatch, sf.QCAP, f"{case.id}/lone{d}-{p}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_skip_all_edges_empty(dtype, monkeypatch):
    """Every leaf zero: each centre, the 600-hub included, keeps its own
    support and has nothing but empty edges."""
    case = sf.no_leaf_case(dtype)
    for qcap in (sf.QCAP, 0):
        ref, got, meta = _on_off(case, monkeypatch, qcap)
        _assert_same(ref, got)
    hub = sf.centre(case.label, 600)
    assert hub in set(got["order"].tolist())
    _oracle(case, monkeypatch, sf.QCAP, f"{case.id}/noleaf")


# ------------------------------------------------ 3. all-zero hub ladder
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("sumF", [0.0, 0.25])
def test_skip_all_zero_hub(sumF, dtype, monkeypatch):
    """F all zero on the hub ladder (degrees up to 600): every node takes
    the shortcut.  llh equals the four-accumulator tree of the one-edge
    term c0 (read from a degree-1 node), the picks follow from it."""
    hip_ops, _ = _hip()
    base = cf.make_case("hub", "sparse", dtype, 512)
    case = cf.Case(base.kind, base.regime, dtype, 512, base.graph,
                   base.label, base.cfg, np.zeros_like(base.F0))
    ref, got, meta = _on_off(case, monkeypatch, 64, sumF=sumF, commit=False)
    _assert_same(ref, got)
    assert (got["gc"] == 0).all()
    deg = np.diff(np.asarray(case.graph.indptr))
    assert meta["n_pack"] == (deg <= 16).sum() and deg.max() == 600
    cfg = meta["cfg"]
    lad = hip_ops._ladder(cfg, DEV).cpu().numpy().astype(np.float32)
    best = got["best"].view(np.float32)
    order = got["order"].astype(np.int64)
    llh = got["llh"].view(np.float64)
    one = float(llh[np.flatnonzero(deg[order] == 1)[0]])  # c0
    gg = np.float32(meta["st"].kp) * np.float32(sumF) * np.float32(sumF)
    want = np.zeros(len(order), np.float32)
    seen = set()
    for i, u in enumerate(order):
        acc = [0.0, 0.0, 0.0, 0.0]
        for e in range(int(deg[u])):
            acc[e & 3] += one
        node_llh = (acc[0] + acc[2]) + (acc[1] + acc[3])
        assert node_llh == llh[i], int(deg[u])
        seen.add(int(deg[u]))
        trial = (acc[0] + acc[1]) + (acc[2] + acc[3])
        for s_j in lad:
            margin = np.float32(np.float32(cfg.alpha) * s_j) * gg
            if trial >= node_llh + float(margin):
                want[i] = s_j
                break
    assert {255, 256, 257, 511, 512, 513, 600} <= seen
    np.testing.assert_array_equal(best, want)
    if sumF == 0.0:
        np.testing.assert_array_equal(best, np.full(len(best), lad[0]))


# --------------------------------------------------- 4. K3W against K3S
def _commit_both(st, pack, steps, cfg):
    """The pack committed on clones by K3S alone (every position a block)
    and with its wave class on K3W; dirty pre-filled with 1."""
    _, ext = _hip()
    out = []
    for n_block in (int(pack["order"].numel()), int(pack["n_block"])):
        F = st.F_local.clone()
        sidx, sval = st._sp_sidx.clone(), st._sp_sval.clone()
        scount = st._sp_scount.clone()
        dirty = torch.ones(st.F.shape[0], device=DEV, dtype=torch.uint8)
        ext.sparse_commit(F, pack["order"], pack["goffset"], pack["gidx"],
                          pack["gval"], pack["gcount"], steps,
                          st._sp_soffset, sidx, sval, scount, st._sp_cap,
                          cfg.min_f, cfg.max_f, n_block, st.sparse_wcap, dirty)
        torch.cuda.synchronize()
        it = torch.int16 if F.dtype == torch.bfloat16 else torch.int32
        out.append(dict(F=F.view(it).cpu().numpy(),
                        scount=scount.cpu().numpy(),
                        sidx=sidx.cpu().numpy(),
                        sval=sval.cpu().numpy().view(np.int32),
                        dirty=dirty.cpu().numpy()))
    return out


def _assert_commit_same(tag, a, b, routed, cap):
    np.testing.assert_array_equal(a["F"], b["F"], err_msg=tag)
    np.testing.assert_array_equal(a["scount"], b["scount"], err_msg=tag)
    np.testing.assert_array_equal(a["dirty"], b["dirty"], err_msg=tag)
    assert (b["dirty"][routed] == 0).all(), tag
    for r in routed:
        sl = slice(r * cap, r * cap + int(b["scount"][r]))
        np.testing.assert_array_equal(a["sidx"][sl], b["sidx"][sl], err_msg=tag)
        np.testing.assert_array_equal(a["sval"][sl], b["sval"][sl], err_msg=tag)


def _patterns(n_wave, g):
    """name -> bool [n_wave]: which wave-class positions accept."""
    pats = {"none": np.zeros(n_wave, bool), "all": np.ones(n_wave, bool),
            "alternating": np.arange(n_wave) % 2 == 0}
    for name, i in (("first", 0), ("last", n_wave - 1), ("g-1", g - 1),
                    ("g", g), ("g+1", g + 1)):
        if 0 <= i < n_wave:
            pats[name] = np.arange(n_wave) == i
    return pats


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", ["below", "equal", "ragged", "c5"])
def test_wave_commit_groups(size, dtype, monkeypatch):
    """K3W (a wave per group of positions) bitwise K3S on F, counts, list
    entries and cleared dirty flags, for accept patterns that put the
    accepted nodes on every side of a group, on wave classes smaller than
    a group, equal to it and not a multiple of it."""
    _, ext = _hip()
    g = int(ext.sparse_commit_group())
    assert g == sf.K3W_G
    if size == "c5":
        case, wcap = cf.make_case("hub", "sparse", dtype, 512), 1024
    else:
        case = sf.staircase_case(dtype)
        wcap = {"below": 1, "equal": g - 2, "ragged": g}[size]
    _env(monkeypatch, 0, wcap)
    cfg, st = _state(case)
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    assert pack is not None
    order = pack["order"].cpu().numpy().astype(np.int64)
    nb = int(pack["n_block"])
    n_wave = len(order) - nb
    want = {"below": 3, "equal": g, "ragged": g + 2}.get(size)
    assert n_wave == want if want else n_wave > 4 * g and n_wave % g != 0
    gc = pack["gcount"].cpu().numpy()[nb:]
    assert (gc > 0).any()
    if size != "c5":
        assert (gc == 0).sum() == 2  # accepted with nothing to commit
    step = float(cfg.ladder()[2])
    for name, pat in _patterns(n_wave, g).items():
        steps = torch.zeros_like(best)
        acc = order[nb:][pat]
        steps[torch.from_numpy(acc).to(DEV)] = step
        if nb:  # the block class commits too, by K3S in both runs
            steps[torch.from_numpy(order[:nb:2].copy()).to(DEV)] = step
        a, b = _commit_both(st, pack, steps, cfg)
        _assert_commit_same(f"{case.id}/{size}/{name}", a, b, order,
                            st._sp_cap)
        # rejected wave-class rows: F and count untouched
        F0 = st.F_local.view(torch.int16 if dtype == "bf16" else torch.int32)
        idle = order[nb:][~pat]
        np.testing.assert_array_equal(b["F"][idle], F0.cpu().numpy()[idle])
        np.testing.assert_array_equal(
            b["scount"][idle], st._sp_scount.cpu().numpy()[idle])
        if name == "all":
            Fh = torch.from_numpy(b["F"]).view(
                torch.bfloat16 if dtype == "bf16" else torch.float32
            ).float().numpy()
            cf.assert_lists(f"{case.id}/{size}", Fh, order[nb:], b["scount"],
                            b["sidx"], b["sval"].view(np.float32),
                            st._sp_cap)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wave_commit_accept_empty(dtype, monkeypatch):
    """The all-zero state with sumF = 0: every node accepts the first step
    with gcount == 0; the commit leaves F zero, every count 0 and every
    routed dirty flag cleared, as K3S does."""
    base = cf.make_case("hub", "sparse", dtype, 512)
    case = cf.Case(base.kind, base.regime, dtype, 512, base.graph,
                   base.label, base.cfg, np.zeros_like(base.F0))
    _env(monkeypatch, 64)
    cfg, st = _state(case)
    st.sumF.fill_(0.0)
    grad, llh, best, pack = st.grad_ls_auto(None)
    torch.cuda.synchronize()
    order = pack["order"].cpu().numpy().astype(np.int64)
    assert (pack["gcount"].cpu().numpy() == 0).all()
    assert (best[pack["order"].long()] > 0).all()
    st._sp_scount[: st.n_local] = 5  # the commit must store the zeros
    a, b = _commit_both(st, pack, best, cfg)
    _assert_commit_same(case.id + "/accept-empty", a, b, order, st._sp_cap)
    assert not b["F"].any() and (b["scount"][order] == 0).all()


# ------------------------------------------------------- 5. kcs_lists_t
def _list_colsum(F, cap, dirty_rows=(), stale=True):
    """sumF of ``F`` [n, kp] (torch, storage dtype) from cap-strided lists
    built by a numpy rescan; ``dirty_rows`` are flagged and (``stale``)
    their lists spoilt, so only a dense read of the row gives its sum."""
    _, ext = _hip()
    Fh = F.float().numpy()
    n, kp = Fh.shape
    scount = np.zeros(n, np.int32)
    sidx = np.full(n * cap, -1, np.int32)
    sval = np.full(n * cap, 1e9, np.float32)
    for r in range(n):
        ks, vs = cf.rescan(Fh, r)
        scount[r] = len(ks)
        if len(ks) <= cap:  # an over-cap row keeps its count only
            sidx[r * cap: r * cap + len(ks)] = ks
            sval[r * cap: r * cap + len(ks)] = vs
    dirty = np.zeros(n, np.uint8)
    for r in dirty_rows:
        dirty[r] = 1
        if stale:
            scount[r] = min(cap, 3)
            sidx[r * cap: r * cap + 3] = (0, 1, 2)
            sval[r * cap: r * cap + 3] = 77.0
    ns = (n + 511) // 512
    partials = torch.full((ns, kp), 5e8, device=DEV)
    out = torch.full((kp,), 5e8, device=DEV)
    ext.sparse_colsum(F.to(DEV), torch.arange(n, device=DEV) * cap,
                      torch.from_numpy(sidx).to(DEV),
                      torch.from_numpy(sval).to(DEV),
                      torch.from_numpy(scount).to(DEV),
                      torch.from_numpy(dirty).to(DEV), cap, partials)
    ext.colsum_stage2(partials, out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), scount


def _check_colsum(tag, F, cap, **kw):
    got, scount = _list_colsum(F, cap, **kw)
    cf.assert_colsum(tag, got, F)
    Fd = F.double().numpy()
    single = (Fd != 0).sum(axis=0) <= 1
    np.testing.assert_array_equal(got[single], Fd.sum(axis=0)[single],
                                  err_msg=tag)
    return got, scount


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_list_colsum_empty_rows(dtype):
    """627 rows (a stripe of 512 and one of 115): all rows empty (exactly
    0), a single non-empty row at each end of each stripe, alternating
    empty rows — every column has one contributor at most: exact."""
    n = sf._base(dtype).graph.num_nodes
    assert n == 627
    for rows in ((), (0,), (511,), (512,), (n - 1,), tuple(range(0, n, 2)),
                 tuple(range(1, n, 2))):
        F = sf.row_state(dtype, rows).stored_F()
        got, scount = _check_colsum(f"{dtype}/rows{rows[:2]}x{len(rows)}", F,
                                    64)
        assert (scount > 0).sum() == len(rows)
        if not rows:
            assert not got.any()
        assert (F.double().numpy() != 0).sum(axis=0).max() <= 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("cap", [8, 64])
def test_list_colsum_mixed_rows(cap, dtype):
    """Empty rows mixed with current lists, dirty rows whose lists are
    stale, and over-cap rows (densified leaves, count only)."""
    case, _ = sf.mixed_case(dtype, 2)
    F0 = case.F0.copy()
    rng = np.random.default_rng(11)
    leaves = sf.leaves_of(case.label)
    dense = leaves[5::40]
    F0[dense] = rng.uniform(0.25, 1.0, size=(len(dense), case.k)).astype(
        np.float32)
    F = cf.Case(case.kind, case.regime, dtype, case.k, case.graph,
                case.label, case.cfg, F0).stored_F()
    nnz = (F.float().numpy() != 0).sum(axis=1)
    empty = np.flatnonzero(nnz == 0)
    assert len(empty) > 64 and (nnz > cap).sum() >= len(dense)
    if cap == 64:  # at cap 8 nearly every non-empty row is over cap
        assert ((nnz > 0) & (nnz <= cap)).sum() > 32
    # dirty: empty rows, listed rows and an over-cap row, in both stripes
    dirty = [int(empty[0]), int(empty[-1]), int(dense[0]),
             int(np.flatnonzero(nnz > 0)[0]), int(np.flatnonzero(nnz > 0)[-1])]
    _check_colsum(f"{case.id}/cap{cap}", F, cap, dirty_rows=dirty)
    _check_colsum(f"{case.id}/cap{cap}/clean", F, cap)
