"""CPU-side fixtures of the packed wave kernel's tests (KFP): the numpy
reference of the packed / single split of the wave class, and the small
ladder states with hand-set rows that tests/test_gpu_kfp_pack.py sweeps.
Nothing here touches a GPU; tests/test_kfp_split_cpu.py checks the helper
and the fixture counts."""
import numpy as np
import torch

import contract_fixtures as cf
from bigclam.core.state import ShardState

KFP_DEG = 16  # most edges of a packed node (one lane per edge)


def launch_order(indptr):
    deg = np.diff(indptr)
    return np.argsort(-deg, kind="stable").astype(np.int32)


def bounds_of(F, graph):
    """Routing bound s_u + sum of the neighbours' s_v per node, from the
    stored F, through ``ShardState.sparse_bounds``."""
    F = np.asarray(F)
    sc = torch.from_numpy((F != 0).sum(axis=1).astype(np.int32))
    b, _ = ShardState.sparse_bounds(
        sc, torch.from_numpy(np.asarray(graph.indptr)),
        torch.from_numpy(np.asarray(graph.indices, dtype=np.int64)),
        graph.num_nodes)
    return b.numpy()


def case_bounds(case):
    return bounds_of(case.stored_F().float().numpy(), case.graph)


def eligible(bound, deg, wcap, qcap):
    """Packable: wave class, bound <= qcap, degree <= KFP_DEG."""
    q = min(qcap, wcap)
    return (bound <= q) & (deg <= KFP_DEG) & (q > 0)


def split_wave_class(order, bound, deg, cap, wcap, qcap):
    """Stable two-way partition of the wave class of a launch order.

    Returns (n_block, wsplit, n_pack): ``wsplit[:n_pack]`` the pack
    positions (n_block + rank within the wave class) of the packable
    nodes, ``wsplit[n_pack:]`` those of the others, both in launch order.
    """
    order = np.asarray(order, dtype=np.int64)
    b_o, d_o = bound[order], deg[order]
    wave = (b_o <= wcap) if wcap > 0 else np.zeros(len(order), bool)
    n_block = int(((b_o > wcap) & (b_o <= cap)).sum()) if wcap > 0 else int(
        (b_o <= cap).sum())
    el = eligible(b_o[wave], d_o[wave], wcap, qcap)
    posn = n_block + np.arange(int(wave.sum()))
    wsplit = np.concatenate([posn[el], posn[~el]]).astype(np.int32)
    return n_block, wsplit, int(el.sum())


def edge_case(dtype, k, zero_rows=(), full_row=None):
    """The small ladder in the sparse regime with the hand-set rows of the
    wave kernel's edge-shape test: a degree-1 centre whose own row and only
    neighbour are zero (ns == 0 with one edge), an isolated all-zero node,
    and a centre holding only columns 0 and k-1.  ``zero_rows``: further
    rows set to zero.  ``full_row = (node, cols)``: that row gets exactly
    the listed columns."""
    base = cf.make_case("small", "sparse", dtype, k)
    g, label = base.graph, base.label
    indptr, indices = np.asarray(g.indptr), np.asarray(g.indices)
    F0 = base.F0.copy()
    c1 = int(np.flatnonzero(label == 1)[0])
    leaf = int(indices[indptr[c1]])
    iso = int(np.flatnonzero(label == -2)[0])
    c2 = int(np.flatnonzero(label == 2)[0])
    F0[[c1, iso, leaf, c2]] = 0.0
    F0[c2, 0] = 0.75
    F0[c2, k - 1] = 0.5
    for r in zero_rows:
        F0[int(r)] = 0.0
    if full_row is not None:
        node, cols = full_row
        F0[int(node)] = 0.0
        F0[int(node), np.asarray(cols)] = 0.5
    case = cf.Case(base.kind, base.regime, dtype, k, g, label, base.cfg, F0)
    return case, dict(c1=c1, leaf=leaf, iso=iso, c2=c2)


def n_pack_of(case, wcap, qcap, cap=1024):
    g = case.graph
    indptr = np.asarray(g.indptr)
    deg = np.diff(indptr)
    return split_wave_class(launch_order(indptr), case_bounds(case), deg, cap,
                            wcap, qcap)[2]


def tail_rows(dtype, k, wcap, qcap):
    """For each residue r in 0..3, a tuple of rows to zero so that the
    edge case's n_pack % 4 == r.  Zeroing a row only lowers bounds, so
    n_pack climbs in small steps as more rows go; the search zeroes the
    rows in id order and keeps the first prefix per residue."""
    case, hand = edge_case(dtype, k)
    rows_all = [int(u) for u in range(case.graph.num_nodes)
                if u not in hand.values()]
    found = {}
    for n in range(len(rows_all) + 1):
        rows = tuple(rows_all[:n])
        c, _ = edge_case(dtype, k, zero_rows=rows)
        found.setdefault(n_pack_of(c, wcap, qcap) % 4, rows)
        if len(found) == 4:
            break
    return found


def quad_case(dtype, k=33, drop=0):
    """A hand-built state of the small ladder whose packed set at
    qcap = 20 is ONE quad: the degree-16 centre next to degree-0 nodes.

    The degree-16 centre keeps columns 16..19 and each of its 16 leaves one
    distinct column 0..15, so its bound is 20 == qcap with all staged
    columns distinct (ns == qcap).  Every other node with an edge has a
    bound above 20 (20 own columns, or a neighbour with 20), every node of
    degree 0 (the degree-0 centre, the two isolated nodes) a bound of 2.
    ``drop`` of the three degree-0 nodes get 21 columns instead, so n_pack
    is 4 - drop."""
    base = cf.make_case("small", "sparse", dtype, k)
    g, label = base.graph, base.label
    indptr, indices = np.asarray(g.indptr), np.asarray(g.indices)
    n = g.num_nodes
    F0 = np.zeros((n, k), np.float32)
    rng = np.random.default_rng(7)
    F0[:, :20] = rng.uniform(0.25, 1.0, size=(n, 20)).astype(np.float32)
    c16 = int(np.flatnonzero(label == 16)[0])
    nb = indices[indptr[c16]: indptr[c16 + 1]]
    assert len(nb) == 16
    F0[c16] = 0.0
    F0[c16, 16:20] = (0.5, 0.75, 1.0, 1.25)
    for j, v in enumerate(nb):
        F0[v] = 0.0
        F0[v, j] = 0.5 + 0.0625 * j
    zero_deg = [int(u) for u in np.flatnonzero(np.diff(indptr) == 0)]
    assert len(zero_deg) == 3
    for i, u in enumerate(zero_deg):
        F0[u] = 0.0
        F0[u, : (21 if i < drop else 2)] = 0.5
    case = cf.Case(base.kind, base.regime, dtype, k, g, label, base.cfg, F0)
    return case, dict(c16=c16, zero_deg=zero_deg)
