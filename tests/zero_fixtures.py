"""CPU-side fixtures of the zero-class tests (tests/test_gpu_zero_class.py):
the numpy statement of the routing's three-way split of the wave class
[packed, bound > 0 | zero class | single] with the zero class's
representatives, and small star-forest states in which the zero class is
empty, one node, one node per degree, or nearly everything.  Nothing here
touches a GPU; tests/test_zero_class_cpu.py checks the helper against a
plain loop and that each named condition occurs.
"""
import functools

import numpy as np

import contract_fixtures as cf
import kfp_fixtures as kf

CAP = WCAP = 1024
QCAP = 64
KS = (64, 129)
REPS = 2  # stars per degree in the forest


def split_zero(order, bound, deg, cap, wcap, qcap, zero=True):
    """The wave class of a launch order in three stable segments.

    Returns dict(n_block, wsplit, wsplit2, n_pack, n_zero, zrep, zrep_node;
    wsplit2 = the two-way split of ``kfp_fixtures.split_wave_class``):
    ``wsplit[:n_pack]`` the pack positions of the packable nodes with
    bound > 0, ``wsplit[n_pack : n_pack + n_zero]`` those with bound 0 (the
    zero class), then the single part, each in launch order.  ``zrep``: the
    pack position of the first node of every degree run of the zero segment,
    in segment order; ``zrep_node[d]``: that node's id, -1 without one.
    ``zero=False``: the zero class stays empty (today's two-way split)."""
    order = np.asarray(order, dtype=np.int64)
    nb, ws, n_all = kf.split_wave_class(order, bound, deg, cap, wcap, qcap)
    routed = np.concatenate([order[(bound[order] > wcap) & (bound[order] <= cap)],
                             order[bound[order] <= wcap]]) if wcap > 0 \
        else order[bound[order] <= cap]
    packed = ws[:n_all]
    isz = (bound[routed[packed]] == 0) & zero
    wsplit = np.concatenate([packed[~isz], packed[isz], ws[n_all:]])
    n_zero = int(isz.sum())
    seg = packed[isz]
    d = deg[routed[seg]]
    first = np.ones(len(seg), bool)
    first[1:] = d[1:] != d[:-1]
    zrep_node = np.full(kf.KFP_DEG + 1, -1, np.int64)
    zrep_node[d[first]] = routed[seg[first]]
    return dict(n_block=nb, wsplit=wsplit.astype(np.int32), wsplit2=ws,
                n_pack=n_all - n_zero, n_zero=n_zero,
                zrep=seg[first].astype(np.int32), zrep_node=zrep_node,
                routed=routed)


# ------------------------------------------------------------------ graphs
@functools.lru_cache(maxsize=None)
def forest(seed=11):
    """Star forest: REPS stars of every degree 0..16 and one star of degree
    17, every leaf private (degree 1); ids permuted.  Returns (Graph,
    label): label = the centre's degree, -1 for leaves."""
    degs = [d for d in range(kf.KFP_DEG + 1) for _ in range(REPS)] + [17]
    n = sum(d + 1 for d in degs)
    perm = np.random.default_rng(seed).permutation(n)
    label = np.full(n, -1, np.int64)
    src, dst, at = [], [], 0
    for d in degs:
        c, leaves = perm[at], perm[at + 1: at + 1 + d]
        label[c] = d
        src += [np.full(d, c), leaves]
        dst += [leaves, np.full(d, c)]
        at += d + 1
    g = cf._csr_graph(n, np.concatenate(src), np.concatenate(dst))
    assert (np.diff(np.asarray(g.indptr))[label >= 0] == label[label >= 0]).all()
    return g, label


@functools.lru_cache(maxsize=None)
def spoiled_forest(seed=12):
    """One star per degree 0..16 whose leaves all join one more node, the
    spoiler (degree 136): with only the spoiler's row non-zero every leaf
    has bound > 0 and the 17 centres are the zero class, one per degree.
    label: centre degree, -1 leaves, -3 the spoiler."""
    degs = list(range(kf.KFP_DEG + 1))
    n = sum(d + 1 for d in degs) + 1
    perm = np.random.default_rng(seed).permutation(n)
    label = np.full(n, -1, np.int64)
    sp = perm[-1]
    label[sp] = -3
    src, dst, at = [], [], 0
    for d in degs:
        c, leaves = perm[at], perm[at + 1: at + 1 + d]
        label[c] = d
        src += [np.full(d, c), leaves, leaves, np.full(d, sp)]
        dst += [leaves, np.full(d, c), np.full(d, sp), leaves]
        at += d + 1
    return cf._csr_graph(n, np.concatenate(src), np.concatenate(dst)), label


def _case(name, g, label, dtype, k, F0):
    return cf.Case(name, "sparse", dtype, k, g, label,
                   cf.regime_cfg("sparse", k, dtype), F0.astype(np.float32))


def _row(rng, k, m):
    """A row with m non-zero columns (values exact in bf16)."""
    r = np.zeros(k, np.float32)
    r[rng.choice(k, size=m, replace=False)] = rng.integers(2, 9, size=m) / 8.0
    return r


def centre(label, d, i=0):
    return int(np.flatnonzero(label == d)[i])


@functools.lru_cache(maxsize=None)
def make(name, dtype, k):
    """The named state (cases a-g of tests/test_gpu_zero_class.py)."""
    rng = np.random.default_rng(100 + k)
    if name == "f_single_runs":
        g, label = spoiled_forest()
        F0 = np.zeros((g.num_nodes, k), np.float32)
        F0[np.flatnonzero(label == -3)[0]] = _row(rng, k, 3)
        return _case(name, g, label, dtype, k, F0)
    g, label = forest()
    n = g.num_nodes
    indptr, indices = np.asarray(g.indptr), np.asarray(g.indices)
    nbrs = lambda u: indices[indptr[u]: indptr[u + 1]]  # noqa: E731
    F0 = np.zeros((n, k), np.float32)
    if name == "a_all_zero":
        pass
    elif name == "b_far_row":
        F0[nbrs(centre(label, 5))[0]] = _row(rng, k, 4)
    elif name == "c_mixed":
        # first star of every degree: one leaf non-zero (the centre and
        # that leaf leave the class, the other leaves stay: zero nodes
        # next to a zero centre).  Second star of degrees 3, 8 and 16: the
        # centre non-zero, so its zero leaves have bound > 0.
        for d in range(1, kf.KFP_DEG + 1):
            F0[nbrs(centre(label, d, 0))[d // 2]] = _row(rng, k, 1 + d % 3)
        for d in (3, 8, 16):
            F0[centre(label, d, 1)] = _row(rng, k, 2)
    elif name == "d_one_zero":
        for u in range(n):
            F0[u] = _row(rng, k, 2)
        F0[centre(label, 0, 1)] = 0.0
    elif name == "e_none":
        for u in range(n):
            F0[u] = _row(rng, k, 2)
    elif name == "g_odd_count":
        # a zero class of more than one kz_fill block whose size is neither
        # a multiple of the block nor of 4
        F0[centre(label, 0, 0)] = _row(rng, k, 2)
        F0[centre(label, 2, 0)] = _row(rng, k, 2)
    else:
        raise ValueError(name)
    return _case(name, g, label, dtype, k, F0)


NAMES = ("a_all_zero", "b_far_row", "c_mixed", "d_one_zero", "e_none",
         "f_single_runs", "g_odd_count")
KZ_BLOCK = 256  # threads of a kz_fill block


def expected(case, cap=CAP, wcap=WCAP, qcap=QCAP, zero=True):
    indptr = np.asarray(case.graph.indptr)
    deg = np.diff(indptr)
    return split_zero(kf.launch_order(indptr), kf.case_bounds(case), deg, cap,
                      wcap, qcap, zero)


# ------------------------------------------------------------- row shards
@functools.lru_cache(maxsize=None)
def shard_graph():
    """300 nodes for three row shards of about 100.  Node 0 (rank 0) joins
    nodes 200..204 only, node 180 (rank 1) joins 205..207 only: their every
    neighbour is a halo row.  Inside each rank a few local stars, and
    isolated nodes."""
    n = 300
    src, dst = [], []

    def star(c, leaves):
        leaves = np.asarray(leaves)
        src.extend([np.full(len(leaves), c), leaves])
        dst.extend([leaves, np.full(len(leaves), c)])

    star(0, range(200, 205))
    star(180, range(205, 208))
    for base in (0, 100, 200):
        star(base + 10, range(base + 11, base + 27))  # degree 16
        star(base + 30, range(base + 31, base + 34))  # degree 3
        star(base + 40, range(base + 41, base + 43))  # degree 2
        star(base + 50, range(base + 51, base + 68))  # degree 17: KFW
    g = cf._csr_graph(n, np.concatenate(src), np.concatenate(dst))
    return g, np.full(n, -1, np.int64)


@functools.lru_cache(maxsize=None)
def shard_case(dtype, k=64):
    """Mostly zero rows; rank 1's degree-3 star has a non-zero leaf and
    rank 2's node 250 a non-zero row, so sumF and GG are non-zero and every
    rank has packed nodes with bound > 0 or 0.  Nodes 0 and 180 and their
    halo neighbours stay zero."""
    g, label = shard_graph()
    rng = np.random.default_rng(77)
    F0 = np.zeros((g.num_nodes, k), np.float32)
    for u in (31, 131, 142, 250, 231, 12):
        F0[u] = _row(rng, k, 3)
    return _case("shard", g, label, dtype, k, F0)


def halo_only_zero(case, rank, world_size=3):
    """Local ids of rank's zero-class nodes with edges whose every
    neighbour is a halo row."""
    from bigclam.core.shard import make_shard

    sh = make_shard(case.graph, rank, world_size)
    b = kf.case_bounds(case)[sh.start: sh.stop]
    ip, ix = np.asarray(sh.indptr), np.asarray(sh.indices)
    return [u for u in range(sh.n_local)
            if b[u] == 0 and 0 < ip[u + 1] - ip[u] <= kf.KFP_DEG
            and (ix[ip[u]: ip[u + 1]] >= sh.n_local).all()]
