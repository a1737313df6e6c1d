"""Top-n link recommendation on the CPU — the CPU path and the exact oracle
of the K11 kernel (kernels/link_kernels.hip), same contract:

For a query node u the candidates are the nodes v != u that are not CSR
neighbours of u and share at least one nonzero column of F with u.  The
score is accumulated in fp32 in ASCENDING column order of row u, product
and sum rounded separately (``acc = acc + F_uc * F_vc`` on float32 values:
the IEEE operations the kernel's ``__fmul_rn`` / ``__fadd_rn`` perform), so
device and CPU results are bitwise equal.  Of the candidates with score > 0
the n largest are returned, ties broken by the lowest node id.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def candidate_bound(model: dict, q: np.ndarray) -> np.ndarray:
    """``T_u`` = sum of the member counts of u's columns, int64 [Q]: the
    number of (candidate, column) terms of the query, an upper bound on its
    distinct candidates."""
    row_ptr = model["row_ptr"]
    sizes = np.diff(model["col_ptr"])
    per_nz = sizes[model["row_col"].astype(np.int64)]
    cum = np.zeros(len(per_nz) + 1, dtype=np.int64)
    np.cumsum(per_nz, out=cum[1:])
    qi = np.asarray(q, dtype=np.int64)
    return cum[row_ptr[qi + 1]] - cum[row_ptr[qi]]


def topn_links_cpu(model, indptr: np.ndarray, indices: np.ndarray,
                   q: np.ndarray, n: int
                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(top_id int32 [Q, n], top_score float32 [Q, n], n_cand int32 [Q])``
    for the queries ``q`` (any order, repeats allowed).  ``model`` is a
    ``SparseModel`` or the dict of its host arrays; rows of fewer than n
    candidates are padded with (-1, 0).  ``n_cand`` counts the distinct
    candidates with score > 0; when it is >= n the row is the exact global
    top-n over all N nodes."""
    m = model.numpy() if hasattr(model, "numpy") else model
    row_ptr, row_col, row_val = m["row_ptr"], m["row_col"], m["row_val"]
    col_ptr, col_row, col_val = m["col_ptr"], m["col_row"], m["col_val"]
    assert row_val.dtype == np.float32 and col_val.dtype == np.float32
    q = np.asarray(q)
    top_id = np.full((len(q), n), -1, dtype=np.int32)
    top_score = np.zeros((len(q), n), dtype=np.float32)
    n_cand = np.zeros(len(q), dtype=np.int32)
    for i, u in enumerate(q.tolist()):
        r0, r1 = int(row_ptr[u]), int(row_ptr[u + 1])
        if r1 == r0:
            continue
        # the (v, p) terms, listed in ascending column order of row u
        vs, ps = [], []
        for j in range(r0, r1):
            c = int(row_col[j])
            m0, m1 = int(col_ptr[c]), int(col_ptr[c + 1])
            vs.append(col_row[m0:m1])
            ps.append(row_val[j] * col_val[m0:m1])  # float32 * float32
        v = np.concatenate(vs)
        ids, inv = np.unique(v, return_inverse=True)
        acc = np.zeros(len(ids), dtype=np.float32)
        # ufunc.at applies repeated indices one by one, in the order listed
        np.add.at(acc, inv, np.concatenate(ps))
        nb = indices[indptr[u]:indptr[u + 1]]
        keep = (acc > 0) & (ids != u) & ~np.isin(ids, nb)
        ids, acc = ids[keep], acc[keep]
        n_cand[i] = len(ids)
        order = np.lexsort((ids, -acc))[:n]  # score desc, then id asc
        top_id[i, :len(order)] = ids[order]
        top_score[i, :len(order)] = acc[order]
    return top_id, top_score, n_cand
