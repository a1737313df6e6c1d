"""CPU checks of the zero-class fixtures (tests/zero_fixtures.py): the numpy
split [packed, bound > 0 | zero class | single] and its representatives
against a plain loop, and that every named state of
tests/test_gpu_zero_class.py holds the condition it is named for."""
import numpy as np
import pytest

import contract_fixtures as cf
import kfp_fixtures as kf
import zero_fixtures as zf
from bigclam.core.shard import make_shard


def _loop_split(order, bound, deg, cap, wcap, qcap):
    """Segments in launch order, one node at a time; a representative is
    the first node of its degree met in the zero segment."""
    n_block = sum(1 for u in order if wcap < bound[u] <= cap) if wcap > 0 \
        else sum(1 for u in order if bound[u] <= cap)
    pk, zr, sg, rank = [], [], [], 0
    zrep, zrep_node = [], [-1] * 17
    for u in order:
        if wcap > 0 and bound[u] <= wcap:
            ok = qcap > 0 and bound[u] <= qcap and deg[u] <= 16
            if ok and bound[u] == 0:
                zr.append(n_block + rank)
                if zrep_node[deg[u]] < 0:
                    zrep_node[deg[u]] = u
                    zrep.append(n_block + rank)
            else:
                (pk if ok else sg).append(n_block + rank)
            rank += 1
    return (n_block, np.array(pk + zr + sg, np.int32), len(pk), len(zr),
            np.array(zrep, np.int32), np.array(zrep_node, np.int64))


@pytest.mark.parametrize("cap,wcap,qcap", [(1024, 256, 64), (1024, 64, 64),
                                           (1024, 256, 0), (40, 16, 8)])
def test_split_helper(cap, wcap, qcap):
    g, _ = cf.ladder_graph("hub")
    indptr = np.asarray(g.indptr)
    deg = np.diff(indptr)
    rng = np.random.default_rng(3)
    bound = rng.integers(0, 120, size=g.num_nodes) * (deg + 1) // 4
    bound[rng.random(g.num_nodes) < 0.4] = 0
    order = kf.launch_order(indptr)
    got = zf.split_zero(order, bound, deg, cap, wcap, qcap)
    nb, ws, npk, nz, zrep, zrn = _loop_split(order.tolist(), bound, deg, cap,
                                             wcap, qcap)
    assert (got["n_block"], got["n_pack"], got["n_zero"]) == (nb, npk, nz)
    np.testing.assert_array_equal(got["wsplit"], ws)
    np.testing.assert_array_equal(got["zrep"], zrep)
    np.testing.assert_array_equal(got["zrep_node"], zrn)
    assert (nz > 0) == (qcap > 0)
    # the zero class off: the two-way split, the single part where it was
    _, ws2, n_all = kf.split_wave_class(order, bound, deg, cap, wcap, qcap)
    off = zf.split_zero(order, bound, deg, cap, wcap, qcap, zero=False)
    np.testing.assert_array_equal(off["wsplit"], ws2)
    assert (off["n_pack"], off["n_zero"]) == (n_all, 0) and n_all == npk + nz
    np.testing.assert_array_equal(ws[n_all:], ws2[n_all:])
    assert sorted(ws[:n_all].tolist()) == sorted(ws2[:n_all].tolist())
    # representatives: segment order is degree-descending
    routed = got["routed"]
    d = deg[routed[zrep]]
    assert (np.diff(d) < 0).all()


@pytest.mark.parametrize("k", zf.KS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fixture_conditions(dtype, k):
    want = {}
    for name in zf.NAMES:
        case = zf.make(name, dtype, k)
        deg = np.diff(np.asarray(case.graph.indptr))
        b = kf.case_bounds(case)
        # values survive the storage rounding: the stored support is F0's
        assert ((case.stored_F().float().numpy()[:, :k] != 0)
                == (case.F0 != 0)).all()
        e = zf.expected(case)
        assert e["n_block"] == 0 and (b <= zf.WCAP).all()
        want[name] = e
        zero = set(e["routed"][e["wsplit"][e["n_pack"]: e["n_pack"]
                                           + e["n_zero"]]].tolist())
        assert zero == set(np.flatnonzero((b == 0) & (deg <= 16)).tolist())
    g, label = zf.forest()
    deg = np.diff(np.asarray(g.indptr))
    assert 200 <= g.num_nodes <= 400
    assert all((deg == d).sum() >= 2 for d in range(17))
    assert (deg == 17).sum() == 1 and deg.max() == 17
    a, b_, c, d, e, f, gg = (want[n] for n in zf.NAMES)
    assert a["n_zero"] == (deg <= 16).sum() and a["n_pack"] == 0
    assert len(a["zrep"]) == 17
    assert b_["n_pack"] == 2 and b_["n_zero"] == a["n_zero"] - 2
    # c: zero rows with bound > 0 (next to a non-zero row) stay out
    case = zf.make("c_mixed", dtype, k)
    bc = kf.case_bounds(case)
    zrow = ~(case.F0 != 0).any(axis=1)
    assert (zrow & (bc > 0) & (deg <= 16)).sum() >= 27
    assert c["n_zero"] > 100 and c["n_pack"] > 40
    # degrees 3, 8 and 16 have no zero node left: holes in the table
    assert len(c["zrep"]) == 14 and (c["zrep_node"][[3, 8, 16]] == -1).all()
    assert (d["n_zero"], len(d["zrep"])) == (1, 1) and d["n_pack"] > 0
    assert e["n_zero"] == 0 and e["n_pack"] > 0 and len(e["zrep"]) == 0
    assert (e["zrep_node"] == -1).all()
    assert f["n_zero"] == 17 == len(f["zrep"])  # every node represents
    n = gg["n_zero"]
    assert n > zf.KZ_BLOCK and n % zf.KZ_BLOCK and n % 4


def test_shard_fixture():
    """Ranks 0 and 1 hold a zero-class node whose every neighbour is a halo
    row (global nodes 0 and 180); every rank has zero and non-zero packed
    nodes."""
    case = zf.shard_case("fp32")
    g = case.graph
    b = kf.case_bounds(case)
    deg = np.diff(np.asarray(g.indptr))
    for r, u in ((0, 0), (1, 180)):
        sh = make_shard(g, r, 3)
        assert u - sh.start in zf.halo_only_zero(case, r)
    for r in range(3):
        sh = make_shard(g, r, 3)
        own = slice(sh.start, sh.stop)
        el = (deg[own] <= 16)
        assert sh.n_local >= 64
        assert ((b[own] == 0) & el).sum() > 17
        assert ((b[own] > 0) & el).sum() > 0
