"""Loop-based fp64 NumPy oracle for BigCLAM — the correctness anchor.

Implements exactly the reference math (SURVEY.md §2.6-§2.10, §2.14;
reference: codes/bigclamv3-7.scala:89-204, codes/Bigclamv2.scala:223-230):
per-node gradient with the 1/(1-exp(-x)) weighting and MIN_P/MAX_P clamps,
per-node local LLH with the sumF trick, the 16-candidate Armijo ladder
evaluated Jacobi-style against a stale F snapshot, the projected commit,
and delta-threshold community extraction.

Deliberately slow and simple (python loops over nodes); used only in tests
on tiny graphs.
"""
from __future__ import annotations

import numpy as np

MIN_P = 1e-4
MAX_P = 0.9999
MIN_F = 0.0
MAX_F = 1000.0
ALPHA = 0.05
BETA = 0.1
LS_STEPS = 15


def clamp_p(x):
    return np.clip(np.exp(-x), MIN_P, MAX_P)


def project(row):
    return np.clip(row, MIN_F, MAX_F)


def node_llh(F, sumF, indptr, indices, u, Fu=None, sumF_u=None):
    """Local log-likelihood of node u (reference codes/bigclamv3-7.scala:137-150).

    llh_u = sum_{v in N(u)} [log(1 - clamp(exp(-Fu.Fv))) + Fu.Fv]
            - Fu.sumF' + Fu.Fu
    where Fu/sumF' may be overridden (line-search trial evaluation).
    """
    fu = F[u] if Fu is None else Fu
    sf = sumF if sumF_u is None else sumF_u
    acc = 0.0
    for v in indices[indptr[u] : indptr[u + 1]]:
        x = float(fu @ F[v])
        p = float(np.clip(np.exp(-x), MIN_P, MAX_P))
        acc += np.log(1.0 - p) + x
    return acc - float(fu @ sf) + float(fu @ fu)


def node_grad_llh(F, sumF, indptr, indices, u):
    """Gradient and local LLH of node u (codes/bigclamv3-7.scala:138-150)."""
    fu = F[u]
    K = F.shape[1]
    grad_acc = np.zeros(K, dtype=np.float64)
    llh_acc = 0.0
    for v in indices[indptr[u] : indptr[u + 1]]:
        fv = F[v]
        x = float(fu @ fv)
        p = float(np.clip(np.exp(-x), MIN_P, MAX_P))
        llh_acc += np.log(1.0 - p) + x
        grad_acc += fv / (1.0 - p)
    grad = grad_acc - sumF + fu
    llh = llh_acc - float(fu @ sumF) + float(fu @ fu)
    return grad, llh


def full_llh(F, sumF, indptr, indices):
    """Total objective: sum of node_llh over all nodes (edges counted twice)."""
    return sum(
        node_llh(F, sumF, indptr, indices, u) for u in range(len(indptr) - 1)
    )


def line_search(F, sumF, indptr, indices, u, grad, llh):
    """Best accepted Armijo step for node u (codes/bigclamv3-7.scala:153-163).

    All candidates evaluated against the same stale F; accept iff
    llh(F_u') >= llh + alpha * s * (grad . grad); keep the max accepted s.
    Returns 0.0 if no candidate is accepted.
    """
    gg = float(grad @ grad)
    best = 0.0
    for i in range(LS_STEPS + 1):
        s = BETA ** i
        fu_new = project(F[u] + s * grad)
        sf_new = sumF - F[u] + fu_new
        trial = node_llh(F, sumF, indptr, indices, u, Fu=fu_new, sumF_u=sf_new)
        if trial >= llh + ALPHA * s * gg:
            best = max(best, s)
            break  # ladder is descending; the first accept is the max
    return best


def sweep(F, sumF, indptr, indices):
    """One synchronous gradient/line-search sweep over all nodes.

    Jacobi semantics: every node's gradient and trial evaluations read the
    same stale snapshot; updates land simultaneously afterwards
    (SURVEY.md §2.8).  Returns (F_new, sumF_new, llh_after, steps[N]).
    """
    n = len(indptr) - 1
    F_new = F.copy()
    steps = np.zeros(n)
    for u in range(n):
        grad, llh = node_grad_llh(F, sumF, indptr, indices, u)
        s = line_search(F, sumF, indptr, indices, u, grad, llh)
        steps[u] = s
        if s > 0.0:
            F_new[u] = project(F[u] + s * grad)
    sumF_new = sumF + (F_new - F).sum(axis=0)
    llh_after = full_llh(F_new, sumF_new, indptr, indices)
    return F_new, sumF_new, llh_after, steps


def fit(F, indptr, indices, tol=1e-4, max_sweeps=50):
    """Convergence loop (MBSGD, codes/bigclamv3-7.scala:206-225)."""
    sumF = F.sum(axis=0)
    llh_old = 0.0
    history = []
    for _ in range(max_sweeps):
        F, sumF, llh, _ = sweep(F, sumF, indptr, indices)
        history.append(llh)
        if llh_old != 0.0 and abs(1.0 - llh / llh_old) < tol:
            break
        llh_old = llh
    return F, sumF, history


def extract_communities(F, num_edges, argmax_fallback=True):
    """Delta-threshold community assignment (codes/Bigclamv2.scala:223-230).

    eps = background edge density; delta = sqrt(-log(1-eps)); node u belongs
    to community c iff F[u,c] >= delta; if no community qualifies, u joins
    the argmax columns (ties included, matching the reference).  Deviation
    (documented): all-zero rows are assigned to NO community (the reference
    would assign them to every community — a latent quirk).
    """
    n = F.shape[0]
    eps = 2.0 * num_edges / (n * (n - 1))
    delta = np.sqrt(-np.log(1.0 - eps))
    members = []
    for u in range(n):
        row = F[u]
        fmax = row.max()
        if fmax >= delta:
            members.append(np.nonzero(row >= delta)[0])
        elif argmax_fallback and fmax > 0:
            members.append(np.nonzero(row == fmax)[0])
        else:
            members.append(np.array([], dtype=np.int64))
    return members, delta


def conductance(indptr, indices, u, total_degree):
    """Ego-net conductance of node u (codes/bigclamv3-7.scala:43-49).

    y = {u} ∪ N(u); z = multiset of neighbors of members of y;
    cut = |{z outside y}|; volS = |z| - cut; volT = Σdeg - volS - 2·cut;
    cond = cut/min(volS, volT) with the reference's 0/1 guards.
    """
    nbrs = indices[indptr[u] : indptr[u + 1]]
    y = set([u]) | set(int(v) for v in nbrs)
    cut = 0
    z_size = 0
    for m in y:
        for w in indices[indptr[m] : indptr[m + 1]]:
            z_size += 1
            if int(w) not in y:
                cut += 1
    vol_s = z_size - cut
    vol_t = total_degree - vol_s - 2 * cut
    if vol_s == 0:
        return 0.0
    if vol_t == 0:
        return 1.0
    return cut / min(vol_s, vol_t)


def armijo_margin_f64(graph, F, grad_u, u, s, cfg):
    """fp64 Armijo acceptance margin of step ``s`` for node ``u``:
    llh_u(clamp(F_u + s·grad_u)) − llh_u(F_u) − α·s·‖grad_u‖².
    A margin within fp32 noise of zero means accept/reject is a tie and
    fp32 implementations may legitimately disagree on the pick."""
    Fd = np.asarray(F, dtype=np.float64)
    sumF = Fd.sum(0)
    gu = np.asarray(grad_u, dtype=np.float64)
    nbrs = graph.indices[graph.indptr[u] : graph.indptr[u + 1]]

    def llh_u(fu):
        x = Fd[nbrs] @ fu
        p = np.clip(np.exp(-x), cfg.min_p, cfg.max_p)
        sf = sumF - Fd[u] + fu
        return float(np.sum(np.log(1 - p) + x) - fu @ sf + fu @ fu)

    fu2 = np.clip(Fd[u] + s * gu, cfg.min_f, cfg.max_f)
    return llh_u(fu2) - llh_u(Fd[u]) - cfg.alpha * s * (gu @ gu)


# ---------------------------------------------------------------------------
# Vectorised fp64 contract oracle (docs/kernels.md, "Numerics contract").
#
# Same math as the loop oracle above, organised as per-node matrix products
# ((deg x K) @ (K x n_ladder)) so that N ~ 650 nodes at K up to 16392 is
# cheap.  It works in a shard's LOCAL index space (rows [0, n_local) owned,
# halo rows after them), takes the STORED F values upcast exactly
# (bf16 -> fp64 is exact) and the fp32 sumF the kernel is given, and returns
# the fp64 result together with the condition scales the error bounds hang
# on.
#
# Tolerances are C * EPS32 * scale.  The constants were MEASURED on the CPU
# against the fp32 torch reference (bigclam/ops/reference.py, plus the fp32
# trial evaluation tests/contract_fixtures.ref_trials) over every fixture in
# tests/contract_fixtures.all_cases(), never against the HIP kernels:
# C = 8 x (largest normalised error of the reference), rounded up to a power
# of two.  The 8x covers the kernels' different reduction order (strided
# partials + wave butterfly + LDS round) and __expf/log1pf being a few ulp
# instead of one.  tests/test_oracle.py::test_reference_meets_contract
# re-measures the maxima and asserts they stay under C/8.
#
#   measured maxima of |ref - fp64| / (eps32 * scale) over all 52 fixtures
#   (largest over the two hosts measured; torch's CPU sum order and
#   exp/log1p differ with the vector width, which moves the margin figure:
#   106.5 on one x86 host, 127.0 on another):
#     grad    45.1  (small ladder, dense, bf16 K=9)     -> 8x =  361 -> 512
#     llh      9.87 (small ladder, dense, bf16 K=9)     -> 8x =   79 -> 128
#     margin 127.0  (small ladder, dense, bf16 K=8185)  -> 8x = 1016 -> 1024
# The maxima are well above 1 because the scales model the error of x but
# not the half-ulp rounding of p = exp(-x) itself, which 1/(1-p) and
# log(1-p) amplify by p/(1-p) ~ 1/x on edges with small x (leaf rows with
# scale 0.01; candidate rows clamped to nearly zero).
EPS32 = 2.0 ** -23
MEASURED_MAX = {"grad": 45.1, "llh": 9.87, "margin": 127.05}
C_GRAD = 512.0
C_LLH = 128.0
C_MARGIN = 1024.0
# bf16 MFMA phase B rounds the clamped candidate rows to bf16 (relative
# error 2^-9 per element, RNE): derived, not measured.
BF16_CAND_EPS = 2.0 ** -9
# share of nodes whose pick may differ from the exact pick (the caps the
# project already used: 2% fp32 paths, 5% bf16 paths; < 100 nodes: 2 nodes)
PICK_CAP = {"fp32": 0.02, "bf16": 0.05}


def _f32(v):
    """A config scalar as the kernels receive it: rounded to fp32.  (With
    max_p = 0.9999 the rounding moves log(1 - p) by 3e-4 relative.)"""
    return float(np.float32(v))


def _cfg_ladder32(cfg):
    """The ladder as the kernels see it: fp32 values, upcast."""
    return np.asarray(cfg.ladder(), dtype=np.float32).astype(np.float64)


def vec_grad_llh(F, sumF, indptr, indices, cfg, n_local=None):
    """fp64 gradient/LLH of every owned node plus condition scales.

    Returns dict(grad [n,K], llh [n], A [n,K], L [n], n_min_p, n_max_p):
      X_e  = sum_k |fu_k||fv_k|
      dw_e = p_e/(1-p_e)^2 where the p-clamp is inactive, else 0
      A[u,k] = sum_e (w_e + dw_e X_e)|fv_k| + |sumF_k| + |fu_k|
      L[u]   = sum_e (|log(1-p_e)| + (1 + p_e/(1-p_e)) X_e)
               + sum_k |fu_k|(|sumF_k| + |fu_k|)
    n_min_p / n_max_p count the edges on which either p-clamp is active.
    """
    F = np.asarray(F, dtype=np.float64)
    sumF = np.asarray(sumF, dtype=np.float64)
    n = len(indptr) - 1 if n_local is None else n_local
    K = F.shape[1]
    grad = np.empty((n, K))
    A = np.empty((n, K))
    llh = np.empty(n)
    L = np.empty(n)
    n_min_p = n_max_p = 0
    aS = np.abs(sumF)
    for u in range(n):
        fu = F[u]
        Fv = F[indices[indptr[u] : indptr[u + 1]]]
        x = Fv @ fu
        X = np.abs(Fv) @ np.abs(fu)
        praw = np.exp(-x)
        p = np.clip(praw, _f32(cfg.min_p), _f32(cfg.max_p))
        free = (praw > _f32(cfg.min_p)) & (praw < _f32(cfg.max_p))
        n_min_p += int((praw <= _f32(cfg.min_p)).sum())
        n_max_p += int((praw >= _f32(cfg.max_p)).sum())
        w = 1.0 / (1.0 - p)
        dw = np.where(free, p / (1.0 - p) ** 2, 0.0)
        grad[u] = w @ Fv - sumF + fu
        A[u] = (w + dw * X) @ np.abs(Fv) + aS + np.abs(fu)
        llh[u] = np.sum(np.log1p(-p) + x) - fu @ sumF + fu @ fu
        L[u] = np.sum(np.abs(np.log1p(-p)) + (1.0 + p / (1.0 - p)) * X) + np.abs(
            fu
        ) @ (aS + np.abs(fu))
    return dict(grad=grad, llh=llh, A=A, L=L, n_min_p=n_min_p, n_max_p=n_max_p)


def vec_margins(F, sumF, indptr, indices, cfg, grad, llh, n_local=None):
    """Armijo margins of every ladder rung for every owned node, given a
    gradient row and base LLH per node (the tests pass the implementation's
    OWN grad/llh upcast, so phase B is judged separately from phase A).

    Returns dict(m [n,J], M [n,J], B [n,J], trial [n,J], pick [n],
    n_max_f): m = trial64_j - llh_u - alpha s_j |g|^2; M its scale (built
    like L on the candidate row, node term bounded by
    sum|fc_k|(|sumF_k| + |fu_k|), plus alpha s_j |g|^2); B the bf16
    candidate-rounding scale sum_e (1 + p/(1-p)) X'_e; pick the exact pick
    (first j with m >= 0, else -1); n_max_f the number of candidate
    entries on the upper F clamp.
    """
    F = np.asarray(F, dtype=np.float64)
    sumF = np.asarray(sumF, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)
    llh = np.asarray(llh, dtype=np.float64)
    n = len(indptr) - 1 if n_local is None else n_local
    s = _cfg_ladder32(cfg)
    J = len(s)
    m = np.empty((n, J))
    M = np.empty((n, J))
    B = np.empty((n, J))
    trial = np.empty((n, J))
    n_max_f = 0
    aS = np.abs(sumF)
    for u in range(n):
        fu = F[u]
        g = grad[u]
        Fv = F[indices[indptr[u] : indptr[u + 1]]]
        raw = fu[:, None] + g[:, None] * s[None, :]
        n_max_f += int((raw >= _f32(cfg.max_f)).sum())
        C = np.clip(raw, _f32(cfg.min_f), _f32(cfg.max_f))  # [K, J]
        x = Fv @ C  # [deg, J]
        X = np.abs(Fv) @ np.abs(C)
        p = np.clip(np.exp(-x), _f32(cfg.min_p), _f32(cfg.max_p))
        amp = (1.0 + p / (1.0 - p)) * X
        gg = float(g @ g)
        arm = cfg.alpha * s * gg
        trial[u] = np.sum(np.log1p(-p) + x, axis=0) - (sumF - fu) @ C
        m[u] = trial[u] - llh[u] - arm
        B[u] = amp.sum(axis=0)
        M[u] = (
            np.sum(np.abs(np.log1p(-p)), axis=0)
            + B[u]
            + (aS + np.abs(fu)) @ np.abs(C)
            + np.abs(arm)
        )
    ok = m >= 0
    pick = np.where(ok.any(axis=1), ok.argmax(axis=1), -1)
    return dict(m=m, M=M, B=B, trial=trial, pick=pick, n_max_f=n_max_f)


def vec_commit(F_local, grad, steps, cfg):
    """fp64 projected commit: clamp(fu + s g) where s > 0, else unchanged."""
    F = np.asarray(F_local, dtype=np.float64)
    g = np.asarray(grad, dtype=np.float64)
    s = np.asarray(steps, dtype=np.float64)[:, None]
    return np.where(s > 0, np.clip(F + s * g, _f32(cfg.min_f), _f32(cfg.max_f)), F)


def steps_to_rungs(best, cfg):
    """Map an implementation's best-step values to ladder rung indices
    (-1 = no step).  A value that is neither 0 nor an fp32 ladder entry is
    a contract violation in itself."""
    lad = np.asarray(cfg.ladder(), dtype=np.float32)
    best = np.asarray(best, dtype=np.float32)
    rung = np.full(best.shape, -2, dtype=np.int64)
    rung[best == 0] = -1
    for j in range(len(lad) - 1, -1, -1):  # descending ladder: all distinct
        rung[best == lad[j]] = j
    assert (rung > -2).all(), "best step is not a ladder value: %r" % (
        best[rung == -2][:5],
    )
    return rung


def grad_violations(grad, o, c_grad=None):
    """Entries of an implementation's grad outside C*eps32*A of grad64."""
    c = C_GRAD if c_grad is None else c_grad
    err = np.abs(np.asarray(grad, dtype=np.float64) - o["grad"])
    return np.argwhere(err > c * EPS32 * o["A"])


def llh_violations(llh, o, c_llh=None):
    c = C_LLH if c_llh is None else c_llh
    err = np.abs(np.asarray(llh, dtype=np.float64) - o["llh"])
    return np.flatnonzero(err > c * EPS32 * o["L"])


def pick_violations(rung, mo, bf16_candidates=False, c_margin=None):
    """Nodes whose pick breaks the acceptance rule (EVERY node is judged):
    no earlier rung clearly acceptable (m <= T for all j < j*), the chosen
    rung not clearly rejected (m[j*] >= -T); for "no step" every rung has
    m <= T.  T = C_MARGIN eps32 M (+ 2^-9 B where the implementation rounds
    candidate rows to bf16).  Returns (bad node ids, nodes differing from
    the exact pick)."""
    c = C_MARGIN if c_margin is None else c_margin
    T = c * EPS32 * mo["M"]
    if bf16_candidates:
        T = T + BF16_CAND_EPS * mo["B"]
    m = mo["m"]
    n, J = m.shape
    jj = np.arange(J)[None, :]
    stop = np.where(rung < 0, J, rung)[:, None]
    earlier_clear = ((m > T) & (jj < stop)).any(axis=1)
    rows = np.flatnonzero(rung >= 0)
    rejected = np.zeros(n, dtype=bool)
    rejected[rows] = m[rows, rung[rows]] < -T[rows, rung[rows]]
    bad = np.flatnonzero(earlier_clear | rejected)
    differ = np.flatnonzero(rung != mo["pick"])
    return bad, differ


def pick_cap_ok(n_differ, n_nodes, dtype):
    if n_nodes < 100:
        return n_differ <= 2
    return n_differ <= PICK_CAP[dtype] * n_nodes


# ---------------------------------------------------------------------------
# Exact oracles of the kernels that bracket the sweep (docs/kernels.md,
# "K5 / K6 / K7 contract").  K5 produces one IEEE division of exact
# integers, K6 exact 0/1 values, K7 integers: every comparison against
# these is exact equality, no tolerance anywhere.  Plain loops, slow on
# purpose.
def memberships(F64, k_true, delta):
    """K7 oracle.  ``F64``: the STORED values upcast exactly, [n, >=k_true].
    The threshold is ``delta`` rounded to fp32 — what the kernel compares
    against (``(float)delta``) and what a torch fp32 comparison with a
    Python float does.  Row rule: members are the columns < k_true with
    f >= t; if there are none and the row max over [:k_true] is > 0,
    members are the columns equal to that max; otherwise none.
    Returns (counts int64 [n], comms int32 [total]), row-major ascending."""
    F64 = np.asarray(F64, dtype=np.float64)
    t = float(np.float32(delta))
    counts = np.zeros(F64.shape[0], dtype=np.int64)
    comms = []
    for u in range(F64.shape[0]):
        row = F64[u, :k_true].tolist()
        mem =[c for c in range(k_true) if row[c] >= t]
        if not mem:
            fmax = max(row) if k_true else 0.0
            if fmax > 0:
                mem = [c for c in range(k_true) if row[c] == fmax]
        counts[u] = len(mem)
        comms += mem
    return counts, np.asarray(comms, dtype=np.int32)


def conductance_int(indptr, indices, u):
    """K5 oracle: ``(deg, z_size, cut, cond)`` of node u from the
    brute-force 2-hop walk over the closed ego-net y = {u} ∪ N(u); the
    three counts are Python ints, cond follows from them by the documented
    guards (vol_S == 0 -> 0, vol_T == 0 -> 1).  All integers are far below
    2^53 and the kernel performs one double division of the same integers,
    so a device cond must be BITWISE equal.  No max(.., 1) guard: vol_T =
    sum of outside degrees - cut >= 0, and two non-zero volumes are >= 1,
    so it cannot fire."""
    total_degree = int(len(indices))
    nbrs = indices[indptr[u] : indptr[u + 1]]
    deg = int(len(nbrs))
    inside = np.zeros(len(indptr) - 1, dtype=bool)
    inside[u] = True
    inside[nbrs] = True
    z_size = 0
    cut = 0
    for m in np.flatnonzero(inside):
        row = indices[indptr[m] : indptr[m + 1]]
        z_size += int(len(row))
        cut += int(np.count_nonzero(~inside[row]))
    vol_s = z_size - cut
    vol_t = total_degree - vol_s - 2 * cut
    if vol_s == 0:
        cond = 0.0
    elif vol_t == 0:
        cond = 1.0
    else:
        cond = float(np.float64(cut) / np.float64(min(vol_s, vol_t)))
    return deg, z_size, cut, cond


def seed_scatter(indptr, indices, seeds, start, stop, kp, include_seed, fill):
    """K6 oracle: an [stop-start, kp] fp64 array pre-filled with ``fill``;
    column c gets 1.0 in the rows of N(seeds[c]) (and of seeds[c] itself
    with ``include_seed``) that lie in [start, stop)."""
    out = np.full((stop - start, kp), float(fill), dtype=np.float64)
    for c, s in enumerate(seeds):
        s = int(s)
        for v in indices[indptr[s] : indptr[s + 1]]:
            v = int(v)
            if start <= v < stop:
                out[v - start, c] = 1.0
        if include_seed and start <= s < stop:
            out[s - start, c] = 1.0
    return out
