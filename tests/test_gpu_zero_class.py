"""GPU tests (MI355X) of the zero class of the sparse sweep: packed nodes
with bound 0 are not run through KFP one by one; routing names one
representative per degree, KFP runs those, and kz_fill copies their llh and
step to the rest.

The contract is bitwise: BIGCLAM_SPARSE_ZERO=1 against =0 on the same
inputs, exact equality on every routed output (the _snapshot / _assert_same
pattern of tests/test_gpu_kfp_pack.py), for both dtypes and both settings of
BIGCLAM_SPARSE_SKIP.  The routing's split and representatives are held,
integer for integer, to the numpy statement in tests/zero_fixtures.py
(checked on the CPU in tests/test_zero_class_cpu.py).  ``wsplit`` itself
stays the two-way split [packed | single]; the routing lists its packed
part once more as [bound > 0 | zero class] (``zsplit``, the tail of the
zero-class buffer), which is what the three-segment statement is held to.

``pack["n_pack"]`` counts the nodes of the packed path, zero class
included, with the switch on and off; the routing's own counts
(``st._wave_split``) are what splits: n_pack + n_zero (on) == n_pack (off).
"""
import numpy as np
import pytest
import torch

import shard_lockstep as sl
import zero_fixtures as zf
from test_gpu_contract import (DEV, _hip, _state,  # noqa: F401
                               _stop_after_gpu_fault)
from test_gpu_kfp_pack import _assert_same, _env, _snapshot

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")


def _routing(st):
    """What the last routing pass of ``st`` left: counts, split and
    representatives, as numpy."""
    _, ext = _hip()
    ws, n_pack, n_zero, n_rep, zscr = st._wave_split
    at_rep, at_node, at_tiles = (int(x) for x in ext.sparse_zero_layout())
    z = zscr.cpu().numpy()
    tiles = (st.n_local + int(ext.sparse_route_tile()) - 1) // int(
        ext.sparse_route_tile())
    return dict(ws=ws.cpu().numpy(), zs=z[at_tiles + 6 * tiles:],
                n_pack=int(n_pack), n_zero=int(n_zero),
                n_rep=int(n_rep), zrep=z[at_rep: at_rep + 17],
                zrep_node=z[at_node: at_node + 17])


def _check_routing(case, st, n_wave, zero=True):
    want = zf.expected(case, zero=zero)
    got = _routing(st)
    assert (got["n_pack"], got["n_zero"]) == (want["n_pack"], want["n_zero"])
    assert got["n_rep"] == len(want["zrep"])
    # wsplit: the two-way split, whatever the switch; zsplit: its packed
    # part again as [bound > 0 | zero class]
    n_all = want["n_pack"] + want["n_zero"]
    np.testing.assert_array_equal(got["ws"][:n_wave], want["wsplit2"])
    np.testing.assert_array_equal(got["zs"][:n_all], want["wsplit"][:n_all])
    assert len(got["zs"]) == st.n_local
    np.testing.assert_array_equal(got["zrep"][: got["n_rep"]], want["zrep"])
    assert (got["zrep"][got["n_rep"]:] == -1).all()
    np.testing.assert_array_equal(got["zrep_node"], want["zrep_node"])
    return got


def _on_off(case, monkeypatch, skip, **kw):
    """(ZERO=0 snapshot, ZERO=1 snapshot, their metas); the routing of both
    against the numpy split."""
    _env(monkeypatch, zf.QCAP, zf.WCAP, zf.CAP)
    monkeypatch.setenv("BIGCLAM_SPARSE_SKIP", skip)
    monkeypatch.setenv("BIGCLAM_SPARSE_ZERO", "0")
    ref, meta0 = _snapshot(case, **kw)
    assert not meta0["st"].sparse_zero
    r0 = _check_routing(case, meta0["st"], meta0["n_wave"], zero=False)
    monkeypatch.setenv("BIGCLAM_SPARSE_ZERO", "1")
    got, meta = _snapshot(case, **kw)
    assert meta["st"].sparse_zero
    assert meta["st"].sparse_skip == (skip == "1")
    r1 = _check_routing(case, meta["st"], meta["n_wave"])
    assert r1["n_pack"] + r1["n_zero"] == r0["n_pack"] and r0["n_zero"] == 0
    assert meta["n_pack"] == meta0["n_pack"] == r0["n_pack"]
    _assert_same(ref, got)  # order, n_block, gcount, live gidx / gval, llh,
    return got, meta, r1    # best; committed F and lists


# ------------------------------------------------ 1. on == off, cases a - g
# every pair of (dtype, skip) and of (dtype, K)
COMBOS = (("fp32", 64, "1"), ("bf16", 129, "1"), ("bf16", 64, "0"),
          ("fp32", 129, "0"))


@pytest.mark.parametrize("dtype,k,skip", COMBOS)
@pytest.mark.parametrize("name", zf.NAMES)
def test_zero_bitwise(name, dtype, k, skip, monkeypatch):
    case = zf.make(name, dtype, k)
    deg = np.diff(np.asarray(case.graph.indptr))
    got, meta, r = _on_off(case, monkeypatch, skip)
    order = got["order"].astype(np.int64)
    n_pack, n_zero = r["n_pack"], r["n_zero"]
    zero_nodes = order[r["zs"][n_pack: n_pack + n_zero]]
    single = order[r["ws"][n_pack + n_zero: meta["n_wave"]]]
    pos = {int(u): i for i, u in enumerate(order)}
    assert all(got["gc"][pos[int(u)]] == 0 for u in zero_nodes)
    if name in ("a_all_zero", "b_far_row", "g_odd_count"):
        # the degree-17 node stays one wave per node
        assert deg[single].tolist() == [17]
    if name == "a_all_zero":
        assert n_zero == (deg <= 16).sum() and n_pack == 0
    if name == "d_one_zero":
        assert n_zero == 1 and r["n_rep"] == 1
    if name == "e_none":
        assert n_zero == 0 and r["n_rep"] == 0 and n_pack > 0
    if name == "f_single_runs":
        assert n_zero == r["n_rep"] == 17
        assert sorted(deg[zero_nodes].tolist()) == list(range(17))
    if name == "g_odd_count":
        assert n_zero > zf.KZ_BLOCK and n_zero % zf.KZ_BLOCK and n_zero % 4
    # within one degree every zero node holds the same llh and step
    llh = dict(zip(order.tolist(), got["llh"].tolist()))
    best = dict(zip(order.tolist(), got["best"].tolist()))
    for d in set(deg[zero_nodes].tolist()):
        us = [int(u) for u in zero_nodes if deg[u] == d]
        assert len({(llh[u], best[u]) for u in us}) == 1


# ----------------------------------------- 2. two full rounds, cases b and c
@pytest.mark.parametrize("skip", ["1", "0"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["b_far_row", "c_mixed"])
def test_zero_two_rounds(name, dtype, skip, monkeypatch):
    """Two rounds of grad_ls_auto + apply_commit, on == off bit for bit.
    The second round reads the first one's sumF, and the list-based column
    sum adds a column's entries by LDS atomics, in no fixed order where a
    column has three or more contributors (docs/kernels.md; it differs
    between two runs of one build).  So the rounds run with
    BIGCLAM_SPARSE_COLSUM=0, the fixed-order column sum; the list-based
    refresh after a zero-class sweep is held bitwise on its inputs (F and
    the rewritten lists) by test_zero_bitwise."""
    case = zf.make(name, dtype, 64)
    _env(monkeypatch, zf.QCAP, zf.WCAP, zf.CAP)
    monkeypatch.setenv("BIGCLAM_SPARSE_COLSUM", "0")
    monkeypatch.setenv("BIGCLAM_SPARSE_SKIP", skip)
    runs = []
    for zero in ("0", "1"):
        monkeypatch.setenv("BIGCLAM_SPARSE_ZERO", zero)
        cfg, st = _state(case)
        out = []
        for _ in range(2):
            grad, llh, best, pack = st.grad_ls_auto(None)
            assert pack is not None
            assert (int(pack["n_zero"]) > 0) == (zero == "1")
            routed = pack["order"].long()
            out += [llh[routed].clone(), best[routed].clone(),
                    pack["order"].clone(), pack["gcount"].clone()]
            st.apply_commit(grad, best, pack)
            out += [sl.bits(st.F_local).clone(), st.sumF.clone(),
                    st._sp_scount[: st.n_local].clone()]
        torch.cuda.synchronize()
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------ 3. row shards
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_row_shards(dtype, monkeypatch):
    """Three ranks in lockstep, two sweeps: ranks 0 and 1 hold a zero-class
    node whose every neighbour is a halo row; on == off per rank."""
    case = zf.shard_case(dtype)
    _env(monkeypatch, zf.QCAP, zf.WCAP, zf.CAP)
    monkeypatch.setenv("BIGCLAM_SPARSE_COLSUM", "0")  # see two_rounds
    runs = []
    for zero in ("0", "1"):
        monkeypatch.setenv("BIGCLAM_SPARSE_ZERO", zero)
        L = sl.Lockstep(case, device=DEV)
        out = []
        for sweep in range(2):
            L.exchange()
            for r, st in enumerate(L.states):
                grad, llh, best, pack = L.grad_ls(r, sl.NoWait())
                assert pack is not None, "sparse routing did not engage"
                n_pack, n_zero = st._wave_split[1:3]
                assert (n_zero > 0) == (zero == "1")
                routed = pack["order"].long()
                if zero == "1" and sweep == 0 and r < 2:
                    zs = torch.from_numpy(_routing(st)["zs"]).to(DEV)
                    zn = routed[zs[n_pack: n_pack + n_zero].long()].tolist()
                    mine = zf.halo_only_zero(case, r)
                    assert mine and set(mine) <= set(zn)
                out += [pack["order"].clone(), pack["gcount"].clone(),
                        llh[routed].clone(), best[routed].clone(),
                        torch.tensor([n_pack + n_zero, pack["n_block"]])]
            for r in range(L.ws):
                L.commit(r)
            L.reduce_sumF()
            out += [sl.bits(st.F_local).clone() for st in L.states]
            out.append(L.sumF.clone())
        torch.cuda.synchronize()
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------ 4. the switch
def test_zero_switch(monkeypatch):
    """Off whenever the packed kernel is off; the pack then reports no zero
    class and no split is produced."""
    case = zf.make("a_all_zero", "bf16", 64)
    _env(monkeypatch, zf.QCAP, zf.WCAP, zf.CAP)
    _, st = _state(case)
    assert st.sparse_zero
    monkeypatch.setenv("BIGCLAM_SPARSE_ZERO", "0")
    assert not st.sparse_zero
    monkeypatch.setenv("BIGCLAM_SPARSE_ZERO", "1")
    for switch in ("BIGCLAM_SPARSE_QCAP", "BIGCLAM_NATIVE_ROUTE"):
        monkeypatch.setenv(switch, "0")
        assert not st.sparse_zero
        _, st2 = _state(case)
        _, _, _, pack = st2.grad_ls_auto(None)
        torch.cuda.synchronize()
        assert pack["n_zero"] == 0 and pack["n_pack"] == 0
        assert st2._wave_split is None
        monkeypatch.delenv(switch)
