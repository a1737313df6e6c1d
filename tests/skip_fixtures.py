"""CPU-side fixtures of the empty-item tests (tests/test_gpu_skip_empty.py):
states of the hub ladder in which edges, nodes and rows are EMPTY in
controlled places, built by zeroing rows of the C5 state
(``cf.make_case("hub", "sparse", dtype, 512)``).  Every edge of the ladder
joins a centre and a pool leaf, so zeroing leaf rows empties chosen edges
of the centres, in CSR position.  Nothing here touches a GPU;
tests/test_skip_fixtures_cpu.py asserts that each named condition occurs.
"""
import functools

import numpy as np

import contract_fixtures as cf
import kfp_fixtures as kf

K = 512
CAP = WCAP = 1024
QCAP = 256  # packs the low-degree centres with a few non-empty edges

# (centre degree, CSR position of the one non-empty edge).  Degree <= 16
# runs packed (KFP): first lane, both sides of the accumulator classes
# (3 | 4), the last lane, deg - 1.  Above: one wave per node (KFW) with
# both sides of the 64-edge chunk, and the hub with its only non-empty
# edge past the first chunk.
SURVIVORS = ((16, 0), (16, 3), (16, 4), (16, 15), (5, 4), (1, 0),
             (65, 63), (65, 64), (129, 63), (129, 64), (129, 65), (129, 128),
             (600, 63), (600, 64), (600, 65), (600, 599))


def _base(dtype):
    return cf.make_case("hub", "sparse", dtype, K)


def _case(base, F0):
    return cf.Case(base.kind, base.regime, base.dtype, base.k, base.graph,
                   base.label, base.cfg, F0)


def centre(label, d):
    return int(np.flatnonzero(label == d)[0])


def leaves_of(label):
    return np.flatnonzero(label == -1)


@functools.lru_cache(maxsize=None)
def survivor_case(dtype, d, p):
    """Every leaf row zero but the one at CSR position ``p`` of the
    degree-``d`` centre: each centre that joins it has exactly one
    non-empty edge, every other centre none (bound == own support)."""
    base = _base(dtype)
    g, label = base.graph, base.label
    indptr, indices = np.asarray(g.indptr), np.asarray(g.indices)
    c = centre(label, d)
    leaf = int(indices[indptr[c] + p])
    F0 = base.F0.copy()
    if not F0[leaf].any():  # one of the base state's all-zero rows
        donor = next(int(v) for v in leaves_of(label) if base.F0[v].any())
        F0[leaf] = base.F0[donor]
    keep = F0[leaf].copy()
    F0[leaves_of(label)] = 0.0
    F0[leaf] = keep
    return _case(base, F0), dict(centre=c, leaf=leaf, pos=p)


@functools.lru_cache(maxsize=None)
def no_leaf_case(dtype):
    """Every leaf row zero: all edges of all centres are empty while the
    centres keep their own support (the 600-hub all-empty, routed)."""
    base = _base(dtype)
    F0 = base.F0.copy()
    F0[leaves_of(base.label)] = 0.0
    return _case(base, F0)


def edge_empty(case):
    """bool [nnz]: the edge's neighbour row is all zero as stored."""
    nz = (case.stored_F().float().numpy() != 0).any(axis=1)
    return ~nz[np.asarray(case.graph.indices, dtype=np.int64)]


def packed_order(case, qcap=QCAP, wcap=WCAP, cap=CAP):
    """Node ids of the packed positions, in the order KFP takes them
    (four consecutive ones per wave), and the routing bounds."""
    indptr = np.asarray(case.graph.indptr)
    deg = np.diff(indptr)
    b = kf.case_bounds(case)
    order = kf.launch_order(indptr).astype(np.int64)
    nb, ws, n_pack = kf.split_wave_class(order, b, deg, cap, wcap, qcap)
    assert nb == 0
    # wsplit holds positions in the routed order [block | wave]: with no
    # block class that is the launch order without the dense nodes
    routed = order[b[order] <= wcap]
    return routed[ws[:n_pack]], b


@functools.lru_cache(maxsize=None)
def mixed_case(dtype, stride=2, quads=True):
    """Only the leaves of pool index 1 (mod ``stride``) keep their rows:
    stride 2 zeroes the leaves of even pool index (the centres see empty
    and non-empty edges interleaved; centres up to degree 33 stay routed),
    stride 8 leaves one edge in eight non-empty, so the centres of degree
    63..129 stay routed with mixed edges on both sides of the 64-edge
    chunk.  The 600-hub and its private leaves (pool index >=
    513, degree 1) zero, which gives a long run of packed nodes with bound
    0; inside that run five whole quads are shaped: quad i < 4 gets its
    own row back at group position i only, quad 4 stays all empty.  One
    private leaf gets QCAP + 1 columns if needed (it leaves the packed
    set), so the last quad is a tail quad.  Returns (case, info).

    ``quads=False`` keeps the hub and its private leaves as they are (no
    run of bound-0 nodes): the state for the fp64 oracle rules, whose cap
    on the share of picks that differ from the exact pick assumes few
    degenerate nodes.  A bound-0 node is degenerate by construction (no
    trial changes anything, the exact Armijo test never passes, the fp32
    margin rounds away at the last rungs); its llh and pick are pinned
    bit for bit by the all-zero tests instead."""
    base = _base(dtype)
    g, label = base.graph, base.label
    pool = cf._hub_pool()
    F0 = base.F0.copy()
    keep = np.zeros(len(pool), bool)
    keep[1::stride] = True
    F0[pool[~keep]] = 0.0
    if not quads:
        case = _case(base, F0)
        order, b = packed_order(case)
        return case, dict(order=order, bound=b)
    F0[pool[513:]] = 0.0
    F0[centre(label, 600)] = 0.0
    order, b = packed_order(_case(base, F0))
    if len(order) % 4 == 0:  # one private leaf leaves the packed set
        F0[pool[-1], : QCAP + 1] = 0.5
        order, b = packed_order(_case(base, F0))
    assert len(order) % 4 != 0
    private = set(pool[513:].tolist())
    quads = [q for q in range(len(order) // 4)
             if set(order[4 * q: 4 * q + 4].tolist()) <= private]
    run = next(q for q in quads if all(q + i in quads for i in range(5)))
    lit = []
    for i in range(4):
        u = int(order[4 * (run + i) + i])
        donor = next(int(v) for v in pool[keep] if base.F0[v].any())
        F0[u] = base.F0[u] if base.F0[u].any() else base.F0[donor]
        lit.append(u)
    case = _case(base, F0)
    order2, b2 = packed_order(case)
    np.testing.assert_array_equal(order, order2)  # the packed set held
    return case, dict(order=order2, bound=b2, run=run, lit=lit)


# ------------------------------------------------- wave-class sizes for K3W
K3W_G = 16  # positions per wave of the wave commit (ext.sparse_commit_group)


@functools.lru_cache(maxsize=None)
def staircase_case(dtype):
    """Bounds one apart: every leaf row zero, the two isolated rows zero,
    and the i-th centre (by degree) holding its first i + 1 columns.  The
    centres' bounds are then 1..25, the isolated nodes' 0 and every
    leaf's at least 25 (its neighbours include the 600-hub, which holds
    25), so a wave cap w < 25 gives a wave class of exactly w + 2 nodes."""
    base = _base(dtype)
    label = base.label
    F0 = np.zeros_like(base.F0)
    for i, c in enumerate(np.flatnonzero(label >= 0)[
            np.argsort(label[label >= 0], kind="stable")]):
        F0[int(c), : i + 1] = 0.5 + 0.0625 * i
    return _case(base, F0)


def wcap_for_wave_size(case, want, cap=CAP):
    """A BIGCLAM_SPARSE_WCAP value at which the wave class of ``case`` has
    ``want(n_wave)`` true, and that size; the smallest such cap."""
    b = kf.case_bounds(case)
    for w in np.unique(b[b > 0]):
        n_wave = int((b <= w).sum())
        if want(n_wave):
            return int(w), n_wave
    raise AssertionError("no wave cap gives the wanted class size")


# ---------------------------------------------------- kcs_lists_t row states
def row_state(dtype, rows, k=K):
    """The hub ladder (627 rows = a stripe of 512 + 115) with only ``rows``
    non-zero; row r holds one column (r, or 2k - 1 - r past k), so every column has at
    most one contributor when the rows are all even or all odd."""
    base = _base(dtype)
    n = base.graph.num_nodes
    F0 = np.zeros((n, k), np.float32)
    for r in rows:
        r = int(r)
        col = r if r < k else 2 * k - 1 - r  # other parity than r
        F0[r, col] = 0.5 + 0.25 * (r % 3)
    return _case(base, F0)
