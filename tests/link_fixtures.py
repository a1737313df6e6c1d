"""Shared inputs of the link-recommendation tests (tests/test_recommend.py
on the CPU, tests/test_gpu_recommend.py on the device): a hand-built edge
fixture whose F values are small powers of two (many exact ties), random
models, and an independent dense oracle of the K11 contract."""
import numpy as np
import torch

from score_fixtures import graph_from_edges, random_graph

EDGE_N = 300
EDGE_K = 24
EDGE_TOP = 10  # the n the fixture's cases are built around

# query nodes of the edge fixture, by case (see edge_fixture)
Q_BIG = 0  # (a) in the 200-member column; (h) neighbours 1, 2, 3 in it too
BIG_SIZE = 200
NB_IN_COL = (1, 2, 3)
Q_EMPTY = 299  # (b) empty F row
Q_ALLNB = 210  # (c) every candidate is a neighbour
Q_NM1, Q_N, Q_NP1 = 220, 230, 241  # (d) n-1, n, n+1 candidates
Q_SELFCOL = 260  # (e) sole member of column 5
Q_ORDER, C_ORDER = 270, 271  # (f) products 2^18, 2^-6, 2^-6
Q_TIE = 280  # (g) 4 candidates ahead of 15 tied ones
TIE_GROUP = tuple(range(100, 115))
TIE_SCORE = 2.0 ** -4

EDGE_QUERIES = np.array(
    [Q_TIE, Q_BIG, Q_EMPTY, Q_ALLNB, Q_NM1, Q_N, Q_NP1, Q_SELFCOL, Q_ORDER,
     Q_BIG, C_ORDER, 199, 150, 100, 5, 284, 261, 213, 229],
    dtype=np.int32,
)  # 19 of them: unsorted, Q_BIG twice, no multiple of 4 or 64


def edge_fixture():
    """``(F float32 [300, 24], graph)``; what it holds is asserted by
    test_recommend.py::test_edge_fixture_is_what_it_claims."""
    F = np.zeros((EDGE_N, EDGE_K), dtype=np.float32)
    edges = []
    # (a) column 0: 200 members, two values -> two big tie groups
    F[0:150, 0] = 2.0 ** -3
    F[150:BIG_SIZE, 0] = 2.0 ** -2
    # (h) members of Q_BIG's column that are its neighbours; one neighbour
    # outside the column
    edges += [(Q_BIG, v) for v in NB_IN_COL] + [(Q_BIG, 250)]
    # (c) column 1
    F[210:214, 1] = 1.0
    edges += [(Q_ALLNB, v) for v in (211, 212, 213)]
    # (d) columns 2, 3, 4 with 10, 11 and 12 members, mixed values
    for col, lo, size in ((2, Q_NM1, 10), (3, Q_N, 11), (4, Q_NP1, 12)):
        ids = np.arange(lo, lo + size)
        F[ids, col] = 2.0 ** ((ids % 4) - 2).astype(np.float32)
    # (e) column 5: Q_SELFCOL alone; its candidates come from column 6
    F[Q_SELFCOL, 5] = 4.0
    F[[Q_SELFCOL, 261, 262], 6] = [0.5, 2.0, 0.25]
    # (f) columns 7, 8, 9
    F[[Q_ORDER, C_ORDER], 7] = 2.0 ** 9
    F[[Q_ORDER, C_ORDER, 272], 8] = 2.0 ** -3
    F[[Q_ORDER, C_ORDER], 9] = 2.0 ** -3
    # (g) column 10: four distinct scores ahead; column 11: the tie group
    F[Q_TIE, 10] = 1.0
    F[[281, 282, 283, 284], 10] = [8.0, 4.0, 2.0, 1.0]
    F[Q_TIE, 11] = 2.0 ** -2
    F[list(TIE_GROUP), 11] = 2.0 ** -2
    # background edges among 1..199 (exclusions inside the big column)
    rng = np.random.default_rng(9)
    edges += rng.integers(1, BIG_SIZE, size=(400, 2)).tolist()
    return F, graph_from_edges(EDGE_N, edges)


def random_model(N=2000, K=64, max_row_nnz=8, seed=0, bf16=False):
    """F float32 [N, K]: every row has 0..max_row_nnz nonzeros, uniform in
    [2^-6, 8); ``bf16`` rounds the values to bfloat16 (exact in fp32)."""
    rng = np.random.default_rng(seed)
    F = np.zeros((N, K), dtype=np.float32)
    for u in range(N):
        m = int(rng.integers(0, max_row_nnz + 1))
        cols = rng.choice(K, size=m, replace=False)
        F[u, cols] = rng.uniform(2.0 ** -6, 8.0, size=m).astype(np.float32)
    if bf16:
        F = torch.from_numpy(F).to(torch.bfloat16).float().numpy()
    return F


def random_inputs(seed, bf16=False, num_queries=150):
    """``(F, graph, queries)``: a random model on a random 8000-edge graph
    and an unsorted query list with repeats."""
    F = random_model(seed=seed, bf16=bf16)
    graph = random_graph(F.shape[0], 8000, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    q = rng.integers(0, F.shape[0], size=num_queries).astype(np.int32)
    q[-1] = q[0]
    return F, graph, q


def smallest_product(F):
    """The smallest product of two nonzeros of one column."""
    lo = np.where(F > 0, F, np.inf).min(axis=0)
    lo = lo[np.isfinite(lo)]
    return float((lo.astype(np.float64) ** 2).min())


def dense_oracle(F, graph, q, n):
    """The contract from dense F, independent of the sparse form: a float32
    column-by-column loop over all K columns and all N nodes."""
    F = np.asarray(F, dtype=np.float32)
    N, K = F.shape
    top_id = np.full((len(q), n), -1, dtype=np.int32)
    top_score = np.zeros((len(q), n), dtype=np.float32)
    n_cand = np.zeros(len(q), dtype=np.int32)
    for i, u in enumerate(np.asarray(q).tolist()):
        acc = np.zeros(N, dtype=np.float32)
        for c in range(K):
            acc = acc + F[u, c] * F[:, c]
        assert acc.dtype == np.float32
        acc[u] = 0.0
        acc[graph.neighbors(u)] = 0.0
        ids = np.flatnonzero(acc > 0)
        n_cand[i] = len(ids)
        order = np.lexsort((ids, -acc[ids]))[:n]
        top_id[i, :len(order)] = ids[order]
        top_score[i, :len(order)] = acc[ids[order]]
    return top_id, top_score, n_cand
