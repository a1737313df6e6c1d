"""CPU checks of the packed-kernel test fixtures (tests/kfp_fixtures.py):
the numpy partition helper against a plain loop, and the eligibility
counts that tests/test_gpu_kfp_pack.py asserts on the GPU."""
import numpy as np
import pytest

import contract_fixtures as cf
import kfp_fixtures as kf


def _loop_split(order, bound, deg, cap, wcap, qcap):
    n_block = sum(1 for u in order if wcap < bound[u] <= cap) if wcap > 0 \
        else sum(1 for u in order if bound[u] <= cap)
    pk, sg, rank = [], [], 0
    for u in order:
        if wcap > 0 and bound[u] <= wcap:
            ok = qcap > 0 and bound[u] <= qcap and deg[u] <= 16
            (pk if ok else sg).append(n_block + rank)
            rank += 1
    return n_block, np.array(pk + sg, np.int32), len(pk)


@pytest.mark.parametrize("cap,wcap,qcap", [(1024, 256, 64), (1024, 64, 64),
                                           (1024, 256, 0), (40, 16, 8),
                                           (1024, 0, 0)])
def test_partition_helper(cap, wcap, qcap):
    g, _ = cf.ladder_graph("hub")
    indptr = np.asarray(g.indptr)
    deg = np.diff(indptr)
    rng = np.random.default_rng(3)
    bound = rng.integers(0, 120, size=g.num_nodes) * (deg + 1) // 4
    order = kf.launch_order(indptr)
    nb, ws, npk = kf.split_wave_class(order, bound, deg, cap, wcap, qcap)
    nb2, ws2, npk2 = _loop_split(order.tolist(), bound, deg, cap, wcap, qcap)
    assert (nb, npk) == (nb2, npk2)
    np.testing.assert_array_equal(ws, ws2)
    assert sorted(ws.tolist()) == list(range(nb, nb + len(ws)))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fixture_counts(dtype):
    case = cf.make_case("hub", "sparse", dtype, 512)
    indptr = np.asarray(case.graph.indptr)
    deg = np.diff(indptr)
    b = kf.case_bounds(case)
    order = kf.launch_order(indptr)
    for qcap, n_pack, single, dmax in ((64, 39, 572, 1), (256, 442, 169, 7)):
        nb, ws, npk = kf.split_wave_class(order, b, deg, 1024, 1024, qcap)
        assert (nb, npk, len(ws) - npk) == (0, n_pack, single)
        el = kf.eligible(b, deg, 1024, qcap)
        assert sorted(set(deg[el].tolist())) == list(range(dmax + 1))
    assert ((b == 256).sum(), (b == 257).sum()) == (11, 5)

    case, _ = kf.edge_case(dtype, 33)
    b = kf.case_bounds(case)
    deg = np.diff(np.asarray(case.graph.indptr))
    assert len(b) == 149
    el = kf.eligible(b, deg, 1024, 64)
    assert el.sum() == 138
    assert sorted(set(deg[el].tolist())) == list(range(17))
    assert (b[deg == 17] <= 64).all() and (deg == 17).any()
    assert kf.eligible(b, deg, 1024, 16).sum() == 81
    tails = kf.tail_rows(dtype, 33, 1024, 16)
    assert sorted(tails) == [0, 1, 2, 3]
    for drop in range(4):
        c, h = kf.quad_case(dtype, drop=drop)
        b = kf.case_bounds(c)
        el = kf.eligible(b, deg, 1024, 20)
        assert el.sum() == 4 - drop and el[h["c16"]] and b[h["c16"]] == 20
        assert sorted(deg[el].tolist()) == [0] * (3 - drop) + [16]
