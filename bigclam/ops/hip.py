"""GPU op wrappers around the in-tree HIP extension ``bigclam._C``.

The extension is built by ``setup.py build_ext --inplace`` (or
``__graft_entry__.build()``) with ``hipcc --offload-arch=gfx950`` and ships
in-tree so the gpurun snapshot carries it.  On a GPU box a missing extension
is a hard error — there is deliberately no silent eager fallback here
(see core/state.py).
"""
from __future__ import annotations

from typing import Tuple

import torch

from ..config import BigClamConfig

_C = None


def ensure_loaded():
    global _C
    if _C is None:
        try:
            from .. import _C as ext
        except ImportError as e:  # pragma: no cover
            raise RuntimeError(
                "bigclam._C HIP extension not built. Run "
                "`python setup.py build_ext --inplace` (gfx950) first. "
                f"Original error: {e}"
            ) from e
        _C = ext
    return _C


_xbuf_cache = {}


def _xbuf(nnz: int, device) -> torch.Tensor:
    """Per-edge dot buffer for the chunked K1 (reused across sweeps)."""
    key = str(device)
    t = _xbuf_cache.get(key)
    if t is None or t.shape[0] < nnz:
        t = torch.empty(nnz, device=device, dtype=torch.float32)
        _xbuf_cache[key] = t
    return t


def _use_chunked_k1(F: torch.Tensor) -> bool:
    """Chunked KD+KW replaces the one-pass K1 where gacc[K] LDS residency
    would cap occupancy at 1 block/CU (measured 235-247 ms/sweep at
    K=25000, profiles/r01_kernel_opt_log.md).  BIGCLAM_K1_CHUNKED=1/0
    forces it on/off (tests + dispatch measurements)."""
    import os

    env = os.environ.get("BIGCLAM_K1_CHUNKED")
    if env is not None:
        return env != "0"
    cap = 16384 if F.dtype == torch.bfloat16 else 8192
    return F.shape[1] > cap


def edge_grad_llh(
    F: torch.Tensor,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    sumF: torch.Tensor,
    order: torch.Tensor,
    cfg: BigClamConfig,
    out: Tuple[torch.Tensor, torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """K1 over the nodes listed in ``order`` (grid = len(order)); rows of
    grad/llh not listed stay untouched, so interior/boundary subsets can be
    launched separately into the same ``out`` buffers (halo overlap)."""
    ext = ensure_loaded()
    n_local = len(indptr) - 1
    if out is None:
        grad = torch.empty(
            n_local, F.shape[1], device=F.device, dtype=torch.float32
        )
        llh = torch.empty(n_local, device=F.device, dtype=torch.float64)
    else:
        grad, llh = out
    if _use_chunked_k1(F):
        ext.edge_grad_llh_chunked(
            F, indptr, indices, sumF, order, grad, llh,
            _xbuf(indices.shape[0], F.device), cfg.min_p, cfg.max_p,
        )
    else:
        ext.edge_grad_llh(
            F, indptr, indices, sumF, order, grad, llh, cfg.min_p, cfg.max_p
        )
    return grad, llh


_ladder_cache = {}


def _ladder(cfg: BigClamConfig, device) -> torch.Tensor:
    key = (tuple(cfg.ladder()), str(device))
    t = _ladder_cache.get(key)
    if t is None:  # cached: a fresh HtoD copy per sweep costs a sync
        t = torch.tensor(cfg.ladder(), device=device, dtype=torch.float32)
        _ladder_cache[key] = t
    return t


def fused_grad_ls(
    F: torch.Tensor,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    sumF: torch.Tensor,
    order: torch.Tensor,
    cfg: BigClamConfig,
    out=None,
    n_mfma: int = 0,
):
    """KF: fused K1 gradient+LLH and K2 line search in one per-node pass.

    Returns (grad [n,K], llh [n] f64, best_step [n]).  ``order`` may be a
    node subset (halo overlap) writing into shared ``out`` buffers.
    ``n_mfma``: the first n_mfma entries of ``order`` (the high-degree
    prefix of the degree-descending launch order) run the MFMA phase-B
    kernel; the rest the direct one."""
    ext = ensure_loaded()
    n_local = len(indptr) - 1
    if out is None:
        grad = torch.empty(
            n_local, F.shape[1], device=F.device, dtype=torch.float32
        )
        llh = torch.empty(n_local, device=F.device, dtype=torch.float64)
        best = torch.empty(n_local, device=F.device, dtype=torch.float32)
    else:
        grad, llh, best = out
    ext.fused_grad_ls(
        F, indptr, indices, sumF, order, grad, llh,
        _ladder(cfg, F.device), best,
        cfg.alpha, cfg.min_p, cfg.max_p, cfg.min_f, cfg.max_f,
        int(n_mfma),
    )
    return grad, llh, best


def linesearch(
    F: torch.Tensor,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    sumF: torch.Tensor,
    grad: torch.Tensor,
    llh: torch.Tensor,
    order: torch.Tensor,
    cfg: BigClamConfig,
    out: torch.Tensor = None,
) -> torch.Tensor:
    """K2 over the nodes listed in ``order`` (subset-capable like K1);
    with ``out`` the results land in the caller's buffer at the listed
    positions."""
    ext = ensure_loaded()
    n_local = len(indptr) - 1
    best = out if out is not None else torch.empty(
        n_local, device=F.device, dtype=torch.float32
    )
    ladder = _ladder(cfg, F.device)
    ext.linesearch(
        F,
        indptr,
        indices,
        sumF,
        grad,
        llh,
        order,
        ladder,
        best,
        cfg.alpha,
        cfg.min_p,
        cfg.max_p,
        cfg.min_f,
        cfg.max_f,
    )
    return best


def apply_step(
    F_local: torch.Tensor,
    grad: torch.Tensor,
    steps: torch.Tensor,
    cfg: BigClamConfig,
    rows: torch.Tensor = None,
    dirty: torch.Tensor = None,
) -> None:
    """K3: in-place projected commit on the owned rows.  ``rows`` (int32)
    switches to list mode: only the listed rows are committed, one block
    each, and ``dirty[u] = steps[u] > 0`` is recorded for them."""
    ext = ensure_loaded()
    ext.apply_step(F_local, grad, steps, cfg.min_f, cfg.max_f, rows, dirty)


def apply_step_colsum(
    F_local: torch.Tensor,
    grad: torch.Tensor,
    steps: torch.Tensor,
    partials: torch.Tensor,
    cfg: BigClamConfig,
) -> torch.Tensor:
    """K3+colsum fused (bf16 storage): commits F in place and returns the
    exact fp32 column sums of the updated shard (one pass over F instead
    of commit + fp32 materialize + torch reduce)."""
    ext = ensure_loaded()
    ext.apply_step_colsum(
        F_local, grad, steps, partials, cfg.min_f, cfg.max_f
    )
    return partials.sum(dim=0)


def seed_init_device(state, graph, seeds, include_seed: bool) -> None:
    """K6: device-side seed-init scatter — F[v, c] = 1 for v in
    N(seed_c) (codes/bigclamv3-7.scala:60-87).  The seeds' compact
    adjacency (k rows) uploads in a few hundred KB; works at any world
    size (off-shard rows are skipped in-kernel).  The caller handles
    pad columns (only exist when #seeds < k) and the sumF refresh."""
    import numpy as np

    ext = ensure_loaded()
    seeds = np.asarray(seeds, dtype=np.int64)
    deg = (graph.indptr[seeds + 1] - graph.indptr[seeds]).astype(np.int64)
    sindptr = np.concatenate([[0], np.cumsum(deg)])
    offs = np.arange(int(deg.sum()), dtype=np.int64) - np.repeat(
        np.cumsum(deg) - deg, deg
    )
    snbrs = graph.indices[
        np.repeat(graph.indptr[seeds], deg) + offs
    ].astype(np.int64)
    dev = state.device
    state.F.zero_()
    ext.seed_init(
        state.F_local,
        torch.from_numpy(sindptr).to(dev),
        torch.from_numpy(snbrs).to(dev),
        torch.from_numpy(seeds).to(dev),
        state.shard.start,
        state.shard.stop,
        include_seed,
    )


def conductance_full_graph(graph, device) -> "torch.Tensor":
    """K5: ego-net conductance of every node of the FULL graph on GPU.

    Used by the seed-init ranking; the ranking itself is a
    trivial host-side pass over the returned [N] fp64 vector.
    """
    import numpy as np

    ext = ensure_loaded()
    indptr = torch.from_numpy(graph.indptr.astype(np.int64)).to(device)
    indices = torch.from_numpy(graph.indices.astype(np.int32)).to(device)
    cond = torch.empty(graph.num_nodes, device=device, dtype=torch.float64)
    total_degree = float(len(graph.indices))
    ext.conductance(indptr, indices, cond, total_degree)
    return cond


def sparse_sweep_part(
    F: torch.Tensor,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    sumF: torch.Tensor,
    order_sparse: torch.Tensor,
    soffset: torch.Tensor,
    sidx: torch.Tensor,
    sval: torch.Tensor,
    scount: torch.Tensor,
    epre: torch.Tensor,
    bound: torch.Tensor,
    goffset: torch.Tensor,
    cap: int,
    llh_out: torch.Tensor,
    best_out: torch.Tensor,
    cfg: BigClamConfig,
    state_pools=None,
    n_block: int = None,
    wcap: int = 0,
    GG: torch.Tensor = None,
    qcap: int = 0,
    wsplit: torch.Tensor = None,
    n_pack: int = 0,
    skip: bool = True,
    n_zero: int = 0,
    n_rep: int = 0,
    zscr: torch.Tensor = None,
):
    """KFS/KFW for the routed (sparse) nodes: the compact gradient pools,
    llh per node, and the Armijo best step.  ``order_sparse[:n_block]``
    (bound in (wcap, cap]) runs one block per node, the rest (bound <=
    wcap) one wave per node; ``n_block=None`` sends every node to the
    block kernel.  Pools, goffset and gcount are indexed by position in
    ``order_sparse`` for both.  Writes llh_out/best_out at the routed
    node positions; returns the commit pack for K3S.  ``epre`` (int32
    [nnz], node-local exclusive support prefix) and ``bound`` (int32
    [n_local]) come from the routing pass, as does ``GG`` = Σ sumF²
    (computed here when not given).  With ``qcap > 0`` and the routing's
    ``wsplit``, the wave class runs as two launches: the pack positions
    ``wsplit[:n_pack]`` four nodes per wave (KFP), the rest one wave per
    node; the outputs are bitwise the same either way.  ``skip`` selects
    the KFW/KFP builds that pass over empty edges and empty active sets
    (``ShardState.sparse_skip``); again bitwise the same outputs.  With
    ``n_zero > 0`` the packed part of ``wsplit`` holds ``n_pack + n_zero``
    nodes, which ``zscr`` lists again as [bound > 0 | bound 0]; the latter,
    the zero class, is not run node by node: KFP runs its ``n_rep``
    representatives and ``kz_fill`` copies their llh and step to the rest,
    bitwise the same once more."""
    ext = ensure_loaded()
    dev = F.device
    n_s = int(order_sparse.numel())
    if n_block is None:
        n_block = n_s
    # per-STATE grad pools (via state_pools): the commit consumes them at
    # the START of the next sweep (the pipelined carry), so a shared
    # module pool could be clobbered by another coexisting state
    gidx, gval = state_pools
    gcount = torch.empty(n_s, device=dev, dtype=torch.int32)
    if GG is None:
        GG = (sumF * sumF).sum().reshape(1)  # device scalar: no host sync
    ext.sparse_fused(
        F, indptr, indices, sumF, order_sparse, soffset, sidx, sval, scount,
        epre, bound, goffset, gidx, gval, gcount, llh_out, GG, _ladder(cfg, dev),
        best_out, cap, cfg.alpha, cfg.min_p, cfg.max_p, cfg.min_f, cfg.max_f,
        int(n_block), int(wcap), int(qcap), wsplit, int(n_pack), bool(skip),
        int(n_zero), int(n_rep), zscr,
    )
    return {
        "order": order_sparse,
        "goffset": goffset,
        "gidx": gidx,
        "gval": gval,
        "gcount": gcount,
    }


def sparse_commit(F_local: torch.Tensor, pack: dict, best: torch.Tensor,
                  state, cfg: BigClamConfig):
    """K3S/K3W: projected commit confined to each routed node's active set,
    rewriting the committed rows' persistent support lists in place (the
    next sweep's KAF then skips them).  The block class
    ``order[:n_block]`` commits one block per node, the wave class one
    wave per node; both clear the routed rows' dirty flags."""
    ensure_loaded().sparse_commit(
        F_local, pack["order"], pack["goffset"], pack["gidx"], pack["gval"],
        pack["gcount"], best, state._sp_soffset, state._sp_sidx,
        state._sp_sval, state._sp_scount, state._sp_cap,
        cfg.min_f, cfg.max_f,
        int(pack.get("n_block", -1)), int(pack.get("wcap", 0)),
        state._dirty,
    )


def extract_membership(
    F_local: torch.Tensor, k_true: int, delta: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """K7: per-row community memberships of the local F shard on device.

    Returns ``(counts int32 [n], comms int32 [total])`` — row u's
    memberships are ``comms[offsets[u] : offsets[u] + counts[u]]`` in
    ascending community order (offsets = exclusive prefix sum of counts).
    Replaces the reference's driver-side threshold pass
    (codes/Bigclamv2.scala:226-229) without materializing N×K anywhere.
    """
    ext = ensure_loaded()
    n = F_local.shape[0]
    counts = torch.empty(n, device=F_local.device, dtype=torch.int32)
    ext.extract_count(F_local, k_true, delta, counts)
    offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts.to(torch.int64)
    total = int(counts.sum().item())
    comms = torch.empty(total, device=F_local.device, dtype=torch.int32)
    ext.extract_fill(F_local, k_true, delta, offsets, comms)
    return counts, comms


def full_llh(
    F: torch.Tensor,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    sumF: torch.Tensor,
    order: torch.Tensor,
    cfg: BigClamConfig,
) -> torch.Tensor:
    ext = ensure_loaded()
    n_local = len(indptr) - 1
    llh = torch.empty(n_local, device=F.device, dtype=torch.float64)
    ext.llh_only(F, indptr, indices, sumF, order, llh, cfg.min_p, cfg.max_p)
    return llh.sum()


def cover_max_tile() -> int:
    """Compiled maximum of K8's LDS tile (counters per block)."""
    return int(ensure_loaded().COVER_MAX_TILE)


def cover_best_match(
    grp_ptr: torch.Tensor,
    grp_nodes: torch.Tensor,
    node_ptr: torch.Tensor,
    node_comm: torch.Tensor,
    size_y: torch.Tensor,
    tile: int = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """K8: for every community of cover X (group-major ``grp_ptr``/
    ``grp_nodes``) the best-matching community of cover Y (node-major
    ``node_ptr``/``node_comm`` ascending per node, sizes ``size_y``) under
    the exact F1/Jaccard argmax (ops/cover_cpu.py is the same contract on
    CPU).  Returns ``(best_idx int32 [G], best_inter int32 [G])`` on
    device; ``tile`` defaults to the compiled maximum (16384 counters)."""
    ext = ensure_loaded()
    if tile is None:
        tile = int(ext.COVER_MAX_TILE)
    g = max(int(grp_ptr.shape[0]) - 1, 0)
    dev = grp_ptr.device
    best_idx = torch.empty(g, device=dev, dtype=torch.int32)
    best_inter = torch.empty(g, device=dev, dtype=torch.int32)
    ext.cover_best_match(
        grp_ptr, grp_nodes, node_ptr, node_comm, size_y, int(tile),
        best_idx, best_inter,
    )
    return best_idx, best_inter


def score_max_tile() -> int:
    """Compiled maximum of K10's LDS tile (member ids per block)."""
    return int(ensure_loaded().SCORE_MAX_TILE)


def community_scores(
    grp_ptr: torch.Tensor,
    grp_nodes: torch.Tensor,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    dmed: int,
    tile: int = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
           torch.Tensor]:
    """K10: the integer edge counts of every community of a cover
    (group-major ``grp_ptr``/``grp_nodes``, members ascending) on a
    symmetric CSR graph (``indptr`` int64 [N+1], ``indices`` int32 [nnz]);
    ``dmed`` is floor(median degree).  Returns ``(int_deg int32 [M], vol
    int64 [G], m2 int64 [G], n_flake int32 [G], n_fomd int32 [G])`` on
    device (ops/cover_cpu.py ``community_scores_cpu`` is the same contract
    on CPU).  ``tile`` (member ids staged in LDS per pass) defaults to the
    largest community size, capped at the compiled maximum."""
    ext = ensure_loaded()
    g = max(int(grp_ptr.shape[0]) - 1, 0)
    if tile is None:
        largest = (
            int((grp_ptr[1:] - grp_ptr[:-1]).max())
            if g > 0 and grp_ptr.is_cuda and grp_ptr.dtype == torch.int64
            else 1
        )
        tile = min(int(ext.SCORE_MAX_TILE), max(1, largest))
    dev = grp_ptr.device
    int_deg = torch.zeros(grp_nodes.shape[0], device=dev, dtype=torch.int32)
    vol = torch.empty(g, device=dev, dtype=torch.int64)
    m2 = torch.empty(g, device=dev, dtype=torch.int64)
    n_flake = torch.empty(g, device=dev, dtype=torch.int32)
    n_fomd = torch.empty(g, device=dev, dtype=torch.int32)
    ext.community_scores(
        grp_ptr, grp_nodes, indptr, indices, int(dmed), int(tile),
        int_deg, vol, m2, n_flake, n_fomd,
    )
    return int_deg, vol, m2, n_flake, n_fomd


def pair_dot(
    F_own: torch.Tensor,
    F_extra: torch.Tensor,
    pu: torch.Tensor,
    pv: torch.Tensor,
) -> torch.Tensor:
    """K9: ``x[i] = F[pu[i]] · F[pv[i]]`` (fp32) over the row space
    ``[F_own ; F_extra]`` — an index below ``F_own.shape[0]`` reads
    ``F_own``, any other reads ``F_extra[idx - n_own]``; the two buffers
    stay separate.  ``pu``/``pv`` are int32 on the device of F.  Bitwise
    reproducible and independent of the other pairs in the call
    (ops/reference.py ``pair_dot`` is the same contract in torch)."""
    ext = ensure_loaded()
    x = torch.empty(pu.shape[0], device=F_own.device, dtype=torch.float32)
    ext.pair_dot(F_own, F_extra, pu, pv, x)
    return x


def link_max_n() -> int:
    """Compiled maximum of K11's ``n`` (recommendations per query)."""
    return int(ensure_loaded().LINK_MAX_N)


def _check_link_input(t, name: str, dtype) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be on GPU")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} has wrong dtype ({t.dtype}, not {dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if t.dim() != 1:
        raise RuntimeError(f"{name} must be 1-D")


def _pow2_at_least(x: torch.Tensor) -> torch.Tensor:
    """Smallest power of two >= x, elementwise (int64, x >= 1)."""
    x = x - 1
    for s in (1, 2, 4, 8, 16, 32):
        x = x | (x >> s)
    return x + 1


def topn_links(
    model,
    indptr: torch.Tensor,
    indices: torch.Tensor,
    q: torch.Tensor,
    n: int,
    lds_slots: int = None,
    scratch_bytes: int = 1 << 30,
    block: int = 256,
):
    """K11: for every query node ``q[i]`` (int32, any order, repeats
    allowed) the ``n`` nodes with the largest ``F_u . F_v`` among the nodes
    that are not u, not a CSR neighbour of u and share a nonzero column with
    u.  ``model`` is a ``core.sparse_model.SparseModel`` on the device;
    ``indptr`` int64 [N+1] / ``indices`` int32 are the graph's symmetric
    CSR.  Returns ``(top_id int32 [Q, n] padded with -1, top_score float32
    [Q, n] padded with 0, n_cand int32 [Q], info)`` on device;
    ops/links_cpu.py ``topn_links_cpu`` is the same contract on CPU and
    agrees bitwise.

    Every query accumulates in its own (id, score) table of
    ``pow2 >= 2 * min(T_u, N)`` slots (at least 64), T_u = the summed
    member counts of u's columns, so a table never fills.  Tables of up to
    ``lds_slots`` slots (default and maximum: 8192 = 64 KB) live in LDS;
    the other queries run the same code on slices of a global scratch, in
    batches of at most ``scratch_bytes``.  ``info`` reports the split:
    ``n_lds``, ``n_global``, ``global_batches``, ``work`` (sum of T_u) and
    ``max_slots``."""
    ext = ensure_loaded()
    n = int(n)
    if not 1 <= n <= int(ext.LINK_MAX_N):
        raise RuntimeError(
            f"n must be in [1, {int(ext.LINK_MAX_N)}], got {n}"
        )
    max_lds = int(ext.LINK_MAX_LDS_SLOTS)
    min_slots = int(ext.LINK_MIN_SLOTS)
    lds_slots = max_lds if lds_slots is None else int(lds_slots)
    if not 0 <= lds_slots <= max_lds:
        raise RuntimeError(
            f"lds_slots must be in [0, {max_lds}], got {lds_slots}"
        )
    for name, dt in (("row_ptr", torch.int64), ("row_col", torch.int32),
                     ("row_val", torch.float32), ("col_ptr", torch.int64),
                     ("col_row", torch.int32), ("col_val", torch.float32)):
        _check_link_input(getattr(model, name), name, dt)
    _check_link_input(indptr, "indptr", torch.int64)
    _check_link_input(indices, "indices", torch.int32)
    _check_link_input(q, "q", torch.int32)
    dev = q.device
    n_nodes, k, nnz = model.n, model.k, int(model.row_col.shape[0])
    if (model.row_ptr.shape[0] != n_nodes + 1
            or indptr.shape[0] != n_nodes + 1
            or model.col_ptr.shape[0] != k + 1
            or any(getattr(model, f).shape[0] != nnz
                   for f in ("row_val", "col_row", "col_val"))):
        raise RuntimeError(
            "pointer/value array lengths do not match N, K and nnz"
        )
    n_q = int(q.shape[0])
    top_id = torch.full((n_q, n), -1, device=dev, dtype=torch.int32)
    top_score = torch.zeros((n_q, n), device=dev, dtype=torch.float32)
    n_cand = torch.zeros(n_q, device=dev, dtype=torch.int32)
    info = {"n_lds": 0, "n_global": 0, "global_batches": 0, "work": 0,
            "max_slots": 0}
    if n_q == 0:
        return top_id, top_score, n_cand, info
    if int(q.min()) < 0 or int(q.max()) >= n_nodes:
        raise RuntimeError(f"q out of range [0, {n_nodes})")
    if nnz and (int(model.row_col.min()) < 0 or int(model.row_col.max()) >= k
                or int(model.row_ptr[-1]) != nnz
                or int(model.col_ptr[-1]) != nnz):
        raise RuntimeError("malformed sparse model")

    # exact candidate bound T_u per query (cold path)
    sizes = model.col_ptr[1:] - model.col_ptr[:-1]
    cum = torch.zeros(nnz + 1, device=dev, dtype=torch.int64)
    torch.cumsum(sizes[model.row_col.long()], 0, out=cum[1:])
    ql = q.long()
    bound = cum[model.row_ptr[ql + 1]] - cum[model.row_ptr[ql]]
    slots = _pow2_at_least(
        (2 * bound.clamp(max=n_nodes)).clamp(min=min_slots)
    )
    info["work"] = int(bound.sum())
    info["max_slots"] = int(slots.max())
    if info["max_slots"] > 1 << 30:
        raise RuntimeError("a candidate table needs more than 2^30 slots")

    arrays = (model.row_ptr, model.row_col, model.row_val, model.col_ptr,
              model.col_row, model.col_val, indptr, indices, q)
    no_off = torch.empty(0, device=dev, dtype=torch.int64)
    no_keys = torch.empty(0, device=dev, dtype=torch.int32)
    no_vals = torch.empty(0, device=dev, dtype=torch.float32)

    # LDS tables: small ones apart, so one heavy query does not size the
    # dynamic LDS (and the occupancy) of every block
    in_lds = slots <= lds_slots
    for part in (in_lds & (slots <= 1024), in_lds & (slots > 1024)):
        sel = torch.nonzero(part).flatten().to(torch.int32)
        if sel.numel() == 0:
            continue
        tab = slots[part].to(torch.int32)
        ext.topn_links(*arrays, sel, tab, no_off, no_keys, no_vals, n,
                       int(tab.max()), int(block), top_id, top_score, n_cand)
        info["n_lds"] += int(sel.numel())

    # global tables, batched under the scratch budget
    sel_g = torch.nonzero(~in_lds).flatten()
    if sel_g.numel():
        budget = int(scratch_bytes) // 8  # slots: int32 id + fp32 score
        tab_g = slots[sel_g]
        if int(tab_g.max()) > budget:
            raise RuntimeError(
                f"a candidate table of {int(tab_g.max())} slots does not fit "
                f"scratch_bytes = {int(scratch_bytes)}"
            )
        ends = torch.cumsum(tab_g, 0).cpu().numpy()
        cuts, start, base = [], 0, 0
        while start < len(ends):  # greedy: as many tables as fit
            stop = int(ends.searchsorted(base + budget, side="right"))
            cuts.append((start, stop))
            start, base = stop, int(ends[stop - 1])
        largest = max(int(ends[b - 1]) - (int(ends[a - 1]) if a else 0)
                      for a, b in cuts)
        keys = torch.empty(largest, device=dev, dtype=torch.int32)
        vals = torch.empty(largest, device=dev, dtype=torch.float32)
        for a, b in cuts:
            tab = tab_g[a:b]
            off = torch.cumsum(tab, 0) - tab
            ext.topn_links(*arrays, sel_g[a:b].to(torch.int32),
                           tab.to(torch.int32), off.contiguous(), keys, vals,
                           n, 0, int(block), top_id, top_score, n_cand)
        info["n_global"] = int(sel_g.numel())
        info["global_batches"] = len(cuts)
    return top_id, top_score, n_cand, info
