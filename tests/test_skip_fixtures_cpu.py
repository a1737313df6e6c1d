"""CPU checks of the empty-item fixtures (tests/skip_fixtures.py): every
condition the GPU tests of tests/test_gpu_skip_empty.py rely on occurs in
the states they sweep — nodes with bound 0, nodes with some but not all
edges empty, the named positions of a lone non-empty edge, the quad
patterns of the packed kernel, the wave-class sizes around the commit
kernel's group, and the row patterns of the list-based column sum."""
import numpy as np
import pytest

import kfp_fixtures as kf
import skip_fixtures as sf


def _per_node(case):
    indptr = np.asarray(case.graph.indptr)
    deg = np.diff(indptr)
    empty = sf.edge_empty(case)
    n_empty = np.add.reduceat(np.append(empty, False).astype(np.int64),
                              np.minimum(indptr[:-1], len(empty)))
    n_empty[deg == 0] = 0
    return indptr, deg, empty, n_empty


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_survivor_positions(dtype):
    """The centre's only non-empty edge sits at the named CSR position;
    packed (degree <= 16, bound <= QCAP) or single as the list says."""
    for d, p in sf.SURVIVORS:
        case, info = sf.survivor_case(dtype, d, p)
        indptr, deg, empty, n_empty = _per_node(case)
        c = info["centre"]
        assert deg[c] == d and 0 <= p < d
        row = empty[indptr[c]: indptr[c + 1]]
        assert np.flatnonzero(~row).tolist() == [p], (d, p)
        b = kf.case_bounds(case)
        assert 0 < b[c] <= sf.CAP
        el = kf.eligible(b, deg, sf.WCAP, sf.QCAP)
        assert el[c] == (d <= 16), (d, p, b[c])
        # every other centre: one non-empty edge or none
        cen = np.flatnonzero(case.label >= 0)
        assert ((deg[cen] - n_empty[cen]) <= 1).all()
    assert {p for d, p in sf.SURVIVORS if d == 16} == {0, 3, 4, 15}
    assert {p for d, p in sf.SURVIVORS if d == 129} >= {63, 64, 65, 128}
    assert {p for d, p in sf.SURVIVORS if d == 65} == {63, 64}
    assert any(d == 600 and p > 64 for d, p in sf.SURVIVORS)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_leaf_state(dtype):
    case = sf.no_leaf_case(dtype)
    indptr, deg, empty, n_empty = _per_node(case)
    cen = np.flatnonzero(case.label >= 0)
    assert (n_empty[cen] == deg[cen]).all()
    b = kf.case_bounds(case)
    hub = sf.centre(case.label, 600)
    assert 0 < b[hub] <= sf.WCAP  # all-empty hub with own support, routed


@pytest.mark.parametrize("stride", [2, 8])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mixed_state(dtype, stride):
    case, info = sf.mixed_case(dtype, stride)
    indptr, deg, empty, n_empty = _per_node(case)
    b = info["bound"]
    np.testing.assert_array_equal(b, kf.case_bounds(case))
    routed = b <= sf.CAP
    # bound 0 on packed and on single-wave nodes alike is not required;
    # packed ones are, and in number
    order = info["order"]
    assert (b[order] == 0).sum() >= 20
    part = (n_empty > 0) & (n_empty < deg) & routed
    el = kf.eligible(b, deg, sf.WCAP, sf.QCAP)
    assert (part & el).sum() >= 3, "packed nodes with mixed edges"
    if stride == 8:
        wide = part & ~el & (deg > 64)
        assert {65, 129} <= set(deg[wide].tolist()), "wide nodes, mixed edges"
    assert (part & ~el & (deg > 16) & (deg <= 64)).any()
    # empty and non-empty edges interleave inside one 16-edge window
    c = next(int(u) for u in np.flatnonzero(part & el) if deg[u] >= 4)
    row = empty[indptr[c]: indptr[c + 1]]
    assert row.any() and (~row).any()
    # the quads: one lit group at position i in quad run + i, then all empty
    run, lit = info["run"], info["lit"]
    for i in range(5):
        quad = order[4 * (run + i): 4 * (run + i) + 4]
        live = b[quad] > 0
        want = np.arange(4) == i if i < 4 else np.zeros(4, bool)
        np.testing.assert_array_equal(live, want)
        if i < 4:
            assert quad[i] == lit[i] and n_empty[lit[i]] == deg[lit[i]] == 1
    assert len(order) % 4 != 0  # a tail quad
    # quads whose four groups are all non-empty exist as well
    full = [q for q in range(len(order) // 4)
            if (b[order[4 * q: 4 * q + 4]] > 0).all()]
    assert full


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wave_class_sizes(dtype):
    """Wave caps that give the commit kernel a wave class below its group,
    equal to it and not a multiple of it, for every group it may use."""
    case = sf.staircase_case(dtype)
    g = sf.K3W_G
    got = [sf.wcap_for_wave_size(case, want) for want in (
        lambda n: 0 < n < g, lambda n: n == g,
        lambda n: n > g + 1 and n % g != 0)]
    assert got == [(1, 3), (g - 2, g), (g, g + 2)]


def test_row_states():
    n = sf._base("bf16").graph.num_nodes
    assert n == 627 and n - 512 == 115  # one full stripe and a short one
    for rows in ((), (0,), (511,), (512,), (n - 1,), tuple(range(0, n, 2))):
        case = sf.row_state("bf16", rows)
        nz = (case.F0 != 0)
        assert nz.any(axis=1).sum() == len(rows)
        assert (nz.sum(axis=0) <= 1).all() or len(rows) > sf.K
