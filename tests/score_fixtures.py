"""Shared inputs of the structural-score tests (tests/test_scores.py on the
CPU, tests/test_gpu_scores.py on the device): graphs with a fixed node
count (isolated nodes allowed), random covers, the edge fixture and a plain
Python set-based oracle of the K10 contract."""
import numpy as np

from bigclam.io import Cover
from bigclam.io.edgelist import Graph

EDGE_N = 700
EDGE_TILES = (16, 64, 65, None)


def graph_from_edges(n, edges):
    """Symmetric CSR over exactly ``n`` nodes (rows ascending, duplicates
    and self-loops removed) — what ``build_graph`` produces, except that
    nodes without an edge keep their id."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    both = np.concatenate([e, e[:, ::-1]])
    key = np.unique(both[:, 0] * n + both[:, 1])
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=indptr[1:])
    return Graph(indptr=indptr, indices=(key % n).astype(np.int32),
                 raw_ids=np.arange(n, dtype=np.int64))


def random_graph(n, num_edges, seed):
    rng = np.random.default_rng(seed)
    return graph_from_edges(n, rng.integers(0, n, size=(num_edges, 2)))


def random_cover(n, num_comms, max_mem, seed):
    """Every node joins 0..max_mem distinct communities."""
    rng = np.random.default_rng(seed)
    comms, nodes = [], []
    for u in range(n):
        k = int(rng.integers(0, max_mem + 1))
        comms.extend(rng.choice(num_comms, size=k, replace=False).tolist())
        nodes.extend([u] * k)
    return Cover.from_pairs(comms, nodes, n, num_comms=num_comms)


def dmed_of(graph):
    """floor(median degree), the slow obvious way."""
    return int(np.floor(np.median(np.diff(graph.indptr))))


def set_oracle(graph, cover, dmed):
    """The five outputs of the contract from Python sets."""
    int_deg = np.zeros(cover.num_pairs, dtype=np.int32)
    g = cover.num_comms
    vol = np.zeros(g, dtype=np.int64)
    m2 = np.zeros(g, dtype=np.int64)
    n_flake = np.zeros(g, dtype=np.int32)
    n_fomd = np.zeros(g, dtype=np.int32)
    for x in range(g):
        mem = cover.members(x)
        s = set(int(u) for u in mem)
        for j, u in enumerate(mem):
            nb = graph.neighbors(int(u))
            d = sum(1 for v in nb if int(v) in s)
            int_deg[cover.grp_ptr[x] + j] = d
            vol[x] += len(nb)
            m2[x] += d
            n_flake[x] += int(2 * d < len(nb))
            n_fomd[x] += int(d > dmed)
    return int_deg, vol, m2, n_flake, n_fomd


# community indices of the edge fixture
C_EMPTY, C_ONE, C_16, C_17, C_64, C_65, C_130, C_ALL = range(8)
C_TWIN_A, C_TWIN_B, C_INDEP, C_CLIQUE, C_EMPTY2, C_LAST = range(8, 14)
HUB = 0
DEGREE_NODES = {601: 1, 602: 15, 603: 16, 604: 17, 605: 64, 606: 65}
ISOLATED = range(690, 697)


def edge_fixture():
    """700 nodes, 14 communities; see the assertions of
    ``test_edge_fixture_is_what_it_claims`` for what it holds."""
    n = EDGE_N
    rng = np.random.default_rng(5)
    edges = [(HUB, v) for v in range(1, 601)]  # the hub: degree 600
    # members of degree 1, 15, 16 and 17 (the 16-lane group edge), 64, 65
    for u, d in DEGREE_NODES.items():
        edges += [(u, v) for v in range(1, d + 1)]
    # sparse background among 1..600
    edges += rng.integers(1, 601, size=(1500, 2)).tolist()
    # clique 610..619; only its overlap node 610 has an edge outside
    clique = list(range(610, 620))
    edges += [(a, b) for a in clique for b in clique if a < b]
    edges.append((610, 620))
    # mutually non-adjacent members, each with one edge outside the set
    indep = list(range(621, 641))
    edges += [(u, 660 + u % 5) for u in indep]
    # the last nodes
    edges += [(699, 698), (699, 697), (698, 697), (699, 600)]
    graph = graph_from_edges(n, edges)

    low = np.arange(1, 601)
    twin = [HUB] + rng.choice(low, size=40, replace=False).tolist()
    members = [None] * 14
    members[C_EMPTY] = []
    members[C_ONE] = [5]
    members[C_16] = list(range(1, 17))
    members[C_17] = list(range(20, 37))
    members[C_64] = rng.choice(low, size=64, replace=False).tolist()
    members[C_65] = [HUB] + list(DEGREE_NODES) + list(range(1, 59))
    members[C_130] = ([HUB] + list(range(1, 101)) + list(DEGREE_NODES)
                      + rng.choice(np.arange(300, 601), size=23,
                                   replace=False).tolist())
    members[C_ALL] = list(range(n))
    members[C_TWIN_A] = twin
    members[C_TWIN_B] = list(twin)
    members[C_INDEP] = indep
    members[C_CLIQUE] = clique
    members[C_EMPTY2] = []
    members[C_LAST] = [600] + list(range(695, 700))
    cover = Cover.from_members(
        [np.asarray(m, dtype=np.int64) for m in members], n
    )
    return graph, cover
