"""CPU tests of the three-shard lockstep driver (tests/shard_lockstep.py)
and of the C6 fixture (docs/kernels.md): the driver on the fp32 torch
reference equals the single-shard reference run and meets the contract on
every sweep; the fixture reaches the sharded sparse-sweep paths it is meant
to (asserted from ``ShardState.sparse_bounds``, so a fixture that stops
exercising them fails here, before a GPU is needed); and a driver with one
sharding defect fails the judge.
"""
import functools

import numpy as np
import pytest
import torch

import contract_fixtures as cf
import oracle
import shard_lockstep as sl
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState

DTYPES = sl.c6_cases()


@functools.lru_cache(maxsize=None)
def _trajectory(dtype):
    """The lockstep reference run of the C6 case, judged on every sweep,
    next to the single-shard run given the same reduced sumF.  Per sweep:
    dict(classes[config][rank], halo, best, nnz, G, fig) (shared: do not modify)."""
    case = sl.c6_case(dtype)
    L = sl.Lockstep(case)
    one = ShardState(make_shard(case.graph, 0, 1), L.cfg, device="cpu")
    one.F[:] = case.stored_F()
    recs = []
    for i in range(sl.SWEEPS):
        L.exchange()
        for st in L.states:  # every halo row is its owner's row, bitwise
            hg = torch.from_numpy(st.shard.halo_globals)
            assert torch.equal(sl.bits(st.F[st.n_local:]),
                               sl.bits(L.global_F()[hg]))
        rec = dict(
            classes={name: [sl.emulated_classes(st, cap, wcap)
                            for st in L.states]
                     for name, (cap, wcap) in sl.CONFIGS.items()},
            G=L.global_F().float().numpy(),
            halo=[sl.row_has_halo(st.shard) for st in L.states],
            nnz=(L.global_F().float() != 0).sum(dim=1).numpy())
        for r in range(L.ws):
            L.grad_ls(r, sl.NoWait())
        assert all(o[3] is None for o in L.outs)  # the reference: no pack
        rec["best"] = [o[2].numpy().copy() for o in L.outs]
        rec["fig"] = L.judge().check(f"{case.id}/lockstep/sweep{i}",
                                     *L.stitched())
        # the single-shard run of the same state with the same sumF
        one.sumF = L.sumF.clone()
        g1, l1, b1, _ = one.grad_ls_auto(None)
        g3, l3, b3 = L.stitched()
        assert torch.equal(g1.view(torch.int32), g3.view(torch.int32))
        # llh: torch's fp32 matrix-vector product of the node term depends
        # on the number of rows, so it is judged (above), not compared
        assert torch.equal(b1, b3)
        F_before = [st.F.clone() for st in L.states]
        for r in range(L.ws):
            L.commit(r)
        one.apply_commit(g1, b1, None)
        for st, Fb in zip(L.states, F_before):  # halo rows: not committed
            assert torch.equal(sl.bits(st.F[st.n_local:]),
                               sl.bits(Fb[st.n_local:]))
        parts = [st.sumF.clone() for st in L.states]
        total = L.reduce_sumF()
        assert torch.equal(total, (parts[0] + parts[1]) + parts[2])
        for st in L.states:
            assert torch.equal(st.sumF, total)
            assert st.sumF.data_ptr() != total.data_ptr()
        assert torch.equal(sl.bits(L.global_F()), sl.bits(one.F_local)), (
            f"{case.id}: sweep {i}: lockstep F differs from the "
            "single-shard reference")
        cf.assert_colsum(f"{case.id}/sweep{i}/sumF", total.numpy(),
                         L.global_F())
        recs.append(rec)
    return recs


# ------------------------------------------------------ driver correctness
@pytest.mark.parametrize("dtype", DTYPES)
def test_lockstep_equals_single_shard_reference(dtype):
    """Four lockstep sweeps on the reference: grad, picks and the
    committed F bitwise equal to the single-shard run, every sweep inside
    the contract — and, like every reference measurement behind the
    constants (tests/oracle.py), inside C/8, which leaves the kernels
    their 8x."""
    recs = _trajectory(dtype)
    assert len(recs) == sl.SWEEPS
    for i, rec in enumerate(recs):
        eg, el, nd = rec["fig"]
        assert eg <= oracle.C_GRAD / 8 and el <= oracle.C_LLH / 8, (i, eg, el)
        # the reference alone stays well inside the pick cap
        assert nd <= 2, (i, nd)


# ------------------------------------------------------ fixture conditions
def test_shard_shapes():
    g, _ = cf.ladder_graph("hub")
    sh = [make_shard(g, r, sl.WORLD) for r in range(sl.WORLD)]
    assert [s.n_local for s in sh] == [190, 181, 256]
    assert [s.n_halo for s in sh] == [370, 383, 369]


def _changed_reads(recs, config, i):
    """Per rank: (routed node, halo row) edges of sweep i whose halo row
    changed in the commit of sweep i - 1, as (rank, node, local row)."""
    changed = (recs[i]["G"] != recs[i - 1]["G"]).any(axis=1)
    g = sl.c6_case("fp32").graph
    out = []
    for r in range(sl.WORLD):
        sh = make_shard(g, r, sl.WORLD)
        c = recs[i]["classes"][config][r]
        routed = np.concatenate([c["wave"], c["block"]])
        src = np.repeat(np.arange(sh.n_local), np.diff(sh.indptr))
        m = np.isin(src, routed) & (sh.indices >= sh.n_local)
        m[m] = changed[sh.halo_globals[sh.indices[m] - sh.n_local]]
        out += [(r, int(u), int(v)) for u, v in zip(src[m], sh.indices[m])]
    return out


@pytest.mark.parametrize("config", list(sl.CONFIGS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_fixture_conditions(dtype, config):
    """What tests/test_gpu_shard_sparse.py relies on, from the reference
    trajectory and sparse_bounds at both cap / wcap settings."""
    recs = _trajectory(dtype)
    wave_halo = block_halo = dense_accepted = 0
    for i, rec in enumerate(recs):
        for r, (c, hh, best) in enumerate(
                zip(rec["classes"][config], rec["halo"], rec["best"])):
            n_local = len(c["bound"])
            n_s = len(c["wave"]) + len(c["block"])
            assert n_s >= max(64, n_local // 4), (i, r, n_s)
            # all three classes on every rank, every sweep
            for name in ("wave", "block", "dense"):
                assert len(c[name]) >= (16 if config == "tight" else 1), (
                    i, r, name, len(c[name]))
            wave_halo += int(hh[c["wave"]].sum())
            block_halo += int(hh[c["block"]].sum())
            dense_accepted += int((best[c["dense"]] > 0).sum())
            # the routed nodes read halo lists: nearly all of them have a
            # halo neighbour (the isolated nodes have no neighbour at all)
            routed = np.concatenate([c["wave"], c["block"]])
            assert hh[routed].sum() >= 0.75 * len(routed), (i, r)
            assert (c["nnz"] <= 512).all()
        accepted = sum(int((b > 0).sum()) for b in rec["best"])
        assert accepted >= 100, (i, accepted)  # a sweep that moves F
    assert wave_halo >= 20 and block_halo >= 20
    if config == "tight":
        assert dense_accepted >= 20
    else:
        # routed nodes that read a halo list rewritten since the last sweep
        reads = [e for i in range(1, sl.SWEEPS)
                 for e in _changed_reads(recs, config, i)]
        assert len(reads) >= 20 and len({e[0] for e in reads}) >= 2, reads
    # the rows, and so the halo lists, really change between sweeps
    for a, b in zip(recs[:-1], recs[1:]):
        grow = int((b["nnz"] > a["nnz"]).sum())
        shrink = int((b["nnz"] < a["nnz"]).sum())
        assert grow >= 20 and shrink >= 20, (grow, shrink)


@pytest.mark.parametrize("dtype", DTYPES)
def test_over_cap_fixture(dtype):
    """The densified leaves: every rank sees at least three over-cap halo
    rows at cap 256 and still routes, and every owned neighbour of such a
    row is in the dense class by its bound."""
    case = sl.over_cap_case(dtype)
    leaves = np.asarray(sl.over_cap_leaves())
    assert (case.label[leaves] == -1).all()
    nnz = (case.stored_F().float().numpy() != 0).sum(axis=1)
    assert (nnz[leaves] == sl.OVER_NNZ).all() and sl.OVER_NNZ > sl.OVER_CAP
    L = sl.Lockstep(case)
    for r, st in enumerate(L.states):
        c = sl.emulated_classes(st, sl.OVER_CAP, sl.OVER_CAP)
        nl = st.n_local
        over = np.flatnonzero(c["nnz"][nl:] > sl.OVER_CAP) + nl
        assert len(over) >= 3, (r, len(over))
        assert set(st.shard.halo_globals[over - nl]) <= set(leaves.tolist())
        n_s = len(c["wave"]) + len(c["block"])
        assert n_s >= max(64, nl // 4), (r, n_s)
        ip, ix = st.shard.indptr, st.shard.indices
        src = np.repeat(np.arange(nl), np.diff(ip))
        nb = np.unique(src[np.isin(ix, over)])
        assert len(nb) and np.isin(nb, c["dense"]).all()
    # one reference sweep of this state meets the contract
    L.sweep(case.id + "/over-cap")


# ---------------------------------------------------------------- sharpness
class _StaleHalo(sl.Lockstep):
    """Halo rows not refreshed after sweep 0."""

    n_exchanges = 0

    def exchange(self):
        if self.n_exchanges == 0:
            super().exchange()
        self.n_exchanges += 1


class _PartialSumF(sl.Lockstep):
    """sumF left as the local partial on rank 1."""

    def reduce_sumF(self):
        part = self.states[1].sumF.clone()
        total = super().reduce_sumF()
        self.states[1].sumF = part
        return total


class _ShiftedHalo(sl.Lockstep):
    """Halo rows installed shifted by one position."""

    def exchange(self):
        super().exchange()
        for st in self.states:
            st.F[st.n_local:] = torch.roll(st.F[st.n_local:], 1, dims=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", [_StaleHalo, _PartialSumF, _ShiftedHalo])
def test_driver_defect_fails_the_judge(defect, dtype):
    """The reference run through a driver with one sharding defect must
    fail the judge: sweep 0 where the defect acts at once, else sweep 1."""
    case = sl.c6_case(dtype)
    L = defect(case)
    first_bad = 0 if defect is _ShiftedHalo else 1
    for i in range(first_bad):
        L.sweep(f"{case.id}/{defect.__name__}/sweep{i}")
    with pytest.raises(AssertionError, match="outside|breaks|differ"):
        L.sweep(f"{case.id}/{defect.__name__}/sweep{first_bad}")


def _changed_halo_row(case):
    """(rank, local halo row) that changed in sweep 0 and that a node
    routed at the wide setting reads in sweep 1."""
    reads = _changed_reads(_trajectory(case.dtype), "wide", 1)
    assert reads, "no routed node reads a changed halo row"
    return reads[0][0], reads[0][2]


def test_list_stand_in_and_stale_halo_list():
    """The list-based stand-in (gradient from rows rebuilt from per-row
    support lists, halo rows included) meets the contract and its lists
    pass ``cf.assert_lists`` past n_local; with ONE halo row's list kept
    from the previous sweep it fails both."""
    case = sl.c6_case("fp32")
    rank, row = _changed_halo_row(case)
    cap = sl.CONFIGS["wide"][0]
    good = sl.ListLockstep(case, cap=cap)
    bad = sl.ListLockstep(case, cap=cap, stale=[(rank, row)])
    for L in (good, bad):
        L.sweep(f"{case.id}/lists/sweep0")
        L.exchange()
        for r in range(L.ws):
            L.grad_ls(r, sl.NoWait())
    for r, st in enumerate(good.states):
        sc, si, sv = good.lists[r]
        cf.assert_lists(f"lists/r{r}", st.F.float().numpy(),
                        range(st.F.shape[0]), sc, si, sv, good.cap)
    good.judge().check(f"{case.id}/lists/sweep1", *good.stitched())
    st = bad.states[rank]
    assert row >= st.n_local
    sc, si, sv = bad.lists[rank]
    with pytest.raises(AssertionError):
        cf.assert_lists("stale", st.F.float().numpy(), [row], sc, si, sv,
                        bad.cap)
    with pytest.raises(AssertionError, match="outside|breaks|differ"):
        bad.judge().check(f"{case.id}/stale-list/sweep1", *bad.stitched())
