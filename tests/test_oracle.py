"""Validate the fp64 NumPy oracle itself (the correctness anchor)."""
import numpy as np
import pytest

import oracle


def _rand_F(n, k, seed=0, scale=0.5):
    rng = np.random.default_rng(seed)
    return rng.random((n, k)) * scale


def test_gradient_matches_finite_differences(tiny_graph):
    g = tiny_graph
    k = 4
    F = _rand_F(g.num_nodes, k, seed=1)
    sumF = F.sum(axis=0)
    u = 2
    grad, llh = oracle.node_grad_llh(F, sumF, g.indptr, g.indices, u)
    # central differences on the GLOBAL objective wrt F[u] — restricted to
    # the terms involving u.  Use the analytic identity: d llh_total / dF_u
    # = 2 * (d llh_u / dF_u) contribution shape... simpler: finite-diff the
    # full objective; the true gradient of the full objective wrt F_u equals
    # 2*grad_u under the edge-doubling convention minus correction — instead
    # finite-diff llh_u directly with sumF updated consistently.
    eps = 1e-6
    num = np.zeros(k)
    for j in range(k):
        Fp = F.copy()
        Fp[u, j] += eps
        sp = sumF.copy()
        sp[j] += eps
        lp = oracle.node_llh(Fp, sp, g.indptr, g.indices, u)
        Fm = F.copy()
        Fm[u, j] -= eps
        sm = sumF.copy()
        sm[j] -= eps
        lm = oracle.node_llh(Fm, sm, g.indptr, g.indices, u)
        num[j] = (lp - lm) / (2 * eps)
    # note: llh_u's own-row terms: -Fu.sumF + Fu.Fu with sumF containing Fu;
    # d/dFu of that = -sumF - Fu + 2Fu = -sumF + Fu  (matches grad finalize)
    np.testing.assert_allclose(grad, num, rtol=1e-4, atol=1e-5)


def test_full_llh_decomposition(tiny_graph):
    g = tiny_graph
    F = _rand_F(g.num_nodes, 3, seed=2)
    sumF = F.sum(axis=0)
    total = oracle.full_llh(F, sumF, g.indptr, g.indices)
    per_node = [
        oracle.node_llh(F, sumF, g.indptr, g.indices, u)
        for u in range(g.num_nodes)
    ]
    assert np.isclose(total, sum(per_node))


def test_sweep_increases_llh_and_preserves_invariants(small_graph):
    g = small_graph
    k = 3
    F = _rand_F(g.num_nodes, k, seed=3, scale=0.3)
    sumF = F.sum(axis=0)
    llh0 = oracle.full_llh(F, sumF, g.indptr, g.indices)
    F1, sumF1, llh1, steps = oracle.sweep(F, sumF, g.indptr, g.indices)
    # F stays in box
    assert (F1 >= oracle.MIN_F).all() and (F1 <= oracle.MAX_F).all()
    # sumF incremental == fresh column sums
    np.testing.assert_allclose(sumF1, F1.sum(axis=0), rtol=1e-9, atol=1e-9)
    # LLH non-decreasing across the Armijo sweep
    assert llh1 >= llh0 - 1e-9
    # at least some node moved
    assert (steps > 0).any()


def test_fit_converges_monotone(small_graph):
    g = small_graph
    F = _rand_F(g.num_nodes, 3, seed=4, scale=0.3)
    F, sumF, hist = oracle.fit(F, g.indptr, g.indices, max_sweeps=30)
    assert len(hist) >= 2
    assert all(b >= a - 1e-9 for a, b in zip(hist, hist[1:]))


def test_armijo_first_accept_is_max_accepted(tiny_graph):
    g = tiny_graph
    F = _rand_F(g.num_nodes, 3, seed=5)
    sumF = F.sum(axis=0)
    for u in range(g.num_nodes):
        grad, llh = oracle.node_grad_llh(F, sumF, g.indptr, g.indices, u)
        s = oracle.line_search(F, sumF, g.indptr, g.indices, u, grad, llh)
        if s == 0.0:
            continue
        gg = float(grad @ grad)
        # every larger candidate must have been rejected
        for i in range(oracle.LS_STEPS + 1):
            sv = oracle.BETA ** i
            if sv <= s:
                break
            fu_new = oracle.project(F[u] + sv * grad)
            sf_new = sumF - F[u] + fu_new
            t = oracle.node_llh(F, sumF, g.indptr, g.indices, u, fu_new, sf_new)
            assert t < llh + oracle.ALPHA * sv * gg


def test_extract_threshold(tiny_graph):
    g = tiny_graph
    F = np.zeros((g.num_nodes, 3))
    F[0, 0] = 5.0
    F[1, 1] = 0.01  # below delta -> argmax fallback
    members, delta = oracle.extract_communities(F, g.num_edges)
    assert 0 in members[0]
    assert 1 in members[1]
    # all-zero rows excluded
    for c in range(3):
        assert 2 not in members[c] or F[2].max() > 0


def test_conductance_guards(tiny_graph):
    g = tiny_graph
    total_degree = int(g.degrees().sum())
    for u in range(g.num_nodes):
        c = oracle.conductance(g.indptr, g.indices, u, total_degree)
        # reference formula: cut/min(volS, volT) — can exceed 1 when the
        # complement volume volT is small; guards give 0.0 / 1.0 exactly.
        assert c >= 0.0 and np.isfinite(c)


def test_reference_matches_oracle_random_graphs():
    """Hypothesis fuzz: the torch fp32 reference matches the float64
    NumPy oracle on random tiny graphs and random F (SURVEY §4 unit net,
    broadened beyond the fixed fixtures)."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    import numpy as np
    import torch

    from bigclam.config import BigClamConfig
    from bigclam.io.edgelist import build_graph
    from bigclam.ops import reference as ref_ops
    import oracle

    @settings(max_examples=25, deadline=None)
    @given(
        st.lists(
            st.tuples(st.integers(0, 12), st.integers(0, 12)),
            min_size=3, max_size=40,
        ).filter(lambda ps: any(a != b for a, b in ps)),
        st.integers(0, 2 ** 31 - 1),
    )
    def check(pairs, seed):
        g = build_graph(np.array(pairs, dtype=np.int64))
        k = 5
        rng = np.random.default_rng(seed)
        F = (rng.random((g.num_nodes, k)) * 0.6).astype(np.float32)
        cfg = BigClamConfig(k=k, device="cpu")
        Ft = torch.from_numpy(F)
        sumF = Ft.sum(0)
        grad, llh = ref_ops.edge_grad_llh(
            Ft, torch.from_numpy(g.indptr),
            torch.from_numpy(g.indices.astype(np.int64)).int(), sumF, cfg,
        )
        F64 = F.astype(np.float64)
        s64 = F64.sum(0)
        for u in range(g.num_nodes):
            og, ol = oracle.node_grad_llh(
                F64, s64, g.indptr, g.indices, u
            )
            np.testing.assert_allclose(
                grad[u].numpy(), og, rtol=5e-4, atol=5e-4
            )
            assert abs(llh[u].item() - ol) < 1e-4 * max(1.0, abs(ol))

    check()


# ---------------------------------------------------------------------------
# Numerics contract (docs/kernels.md): vectorised oracle, fixtures, constants
# and sharpness.  Everything below runs on the CPU against the oracle alone
# or the fp32 torch reference; the HIP kernels meet the same rules in
# tests/test_gpu_contract.py.
import functools

import contract_fixtures as cf


def test_vec_oracle_matches_loop_oracle(tiny_graph, small_graph):
    import torch  # noqa: F401
    from bigclam.config import BigClamConfig

    cfg = BigClamConfig(k=4, device="cpu")
    for g, seed in ((tiny_graph, 1), (small_graph, 2)):
        F = _rand_F(g.num_nodes, 4, seed=seed)
        # the kernels receive fp32 sumF: keep it exactly representable
        sumF = F.sum(axis=0).astype(np.float32).astype(np.float64)
        o = oracle.vec_grad_llh(F, sumF, g.indptr, g.indices, cfg)
        assert o["n_min_p"] == 0 and o["n_max_p"] == 0
        mo = oracle.vec_margins(F, sumF, g.indptr, g.indices, cfg, o["grad"],
                                o["llh"])
        lad = cfg.ladder()
        for u in range(g.num_nodes):
            og, ol = oracle.node_grad_llh(F, sumF, g.indptr, g.indices, u)
            np.testing.assert_allclose(o["grad"][u], og, rtol=1e-12, atol=1e-12)
            assert abs(o["llh"][u] - ol) < 1e-10 * max(1.0, abs(ol))
            s = oracle.line_search(F, sumF, g.indptr, g.indices, u, og, ol)
            j = int(mo["pick"][u])
            assert (s == 0.0 and j < 0) or (j >= 0 and np.isclose(s, lad[j]))
            # margins against the loop formula (the fp32 rounding of the
            # ladder and of max_p moves them by ~1e-7 relative of the scale)
            for jj in (0, 3, 9):
                fu_new = oracle.project(F[u] + lad[jj] * og)
                t = oracle.node_llh(F, sumF, g.indptr, g.indices, u, fu_new,
                                    sumF - F[u] + fu_new)
                m = t - ol - oracle.ALPHA * lad[jj] * float(og @ og)
                # fp32 ladder: <= 1e-7 M; fp32 max_p on a clamped edge
                # moves log(1 - p) by 3e-4
                assert abs(mo["m"][u, jj] - m) < (
                    1e-6 * mo["M"][u, jj] + 4e-4 * g.degrees()[u]
                )
    # commit
    st = np.array([0.0, 1.0, 0.1] * 3)[: tiny_graph.num_nodes]
    F = _rand_F(tiny_graph.num_nodes, 4, seed=3)
    G = _rand_F(tiny_graph.num_nodes, 4, seed=4, scale=4000.0) - 1000.0
    out = oracle.vec_commit(F, G, st, cfg)
    for u in range(tiny_graph.num_nodes):
        exp = F[u] if st[u] == 0 else oracle.project(F[u] + st[u] * G[u])
        np.testing.assert_array_equal(out[u], exp)


@functools.lru_cache(maxsize=None)
def _analysis(t):
    """Reference + oracle on one fixture (shared by the tests below)."""
    c = cf.make_case(*t)
    r = cf.ref_run(c)
    F64 = r["F"].double().numpy()
    s64 = r["sumF"].double().numpy()
    g = c.graph
    o = oracle.vec_grad_llh(F64, s64, g.indptr, g.indices, c.cfg)
    mo = oracle.vec_margins(F64, s64, g.indptr, g.indices, c.cfg,
                            r["grad"].numpy(), r["llh"].numpy())
    safe = lambda a: np.where(a > 0, a, 1.0)  # noqa: E731  (0 error on 0 scale)
    err = dict(
        grad=float((np.abs(r["grad"].double().numpy() - o["grad"])
                    / (oracle.EPS32 * safe(o["A"]))).max()),
        llh=float((np.abs(r["llh"].numpy() - o["llh"])
                   / (oracle.EPS32 * safe(o["L"]))).max()),
        margin=float((np.abs(r["trials"].numpy() - mo["trial"])
                      / (oracle.EPS32 * safe(mo["M"]))).max()),
    )
    return c, r, F64, s64, o, mo, err


_ALL = cf.all_cases()
_IDS = [cf.case_id(t) for t in _ALL]


@pytest.mark.parametrize("t", _ALL, ids=_IDS)
def test_fixture_conditions(t):
    """The fixtures can tell a constant-pick or clamp-blind kernel from a
    right one: picks spread over the ladder, clamps active where meant."""
    c, r, F64, s64, o, mo, err = _analysis(t)
    n = c.graph.num_nodes
    vals, cnt = np.unique(mo["pick"], return_counts=True)
    assert len(vals) >= 4, dict(zip(vals.tolist(), cnt.tolist()))
    assert cnt.max() <= 0.6 * n, dict(zip(vals.tolist(), cnt.tolist()))
    if c.regime == "saturated":
        assert o["n_min_p"] > 0
        x_big = o["n_min_p"] / len(c.graph.indices)
        assert x_big > 0.5  # x >= -log(min_p) ~ 9.2 on most edges
    if c.regime == "sparse":
        assert o["n_max_p"] > 0
        zeros = float((c.F0 == 0).mean())
        assert 0.85 < zeros < 0.97, zeros
        assert ((c.F0 != 0).sum(axis=1) == 0).sum() >= 3  # all-zero rows
    if c.regime == "dense":
        assert o["n_min_p"] == 0 and o["n_max_p"] == 0
    if c.regime == "capped":
        assert mo["n_max_f"] > 0
        assert (c.F0 == 0).any() and (c.F0 == 0.5).any()
        assert c.cfg.min_f == 0.0
    if c.regime == "short":
        assert len(c.cfg.ladder()) == 8 < 16
    # isolated nodes and exact centre degrees
    deg = c.graph.degrees()
    assert (deg == 0).sum() >= 3
    want = cf.SMALL_DEGREES if c.kind == "small" else cf.HUB_DEGREES
    assert sorted(deg[c.label >= 0].tolist()) == sorted(want)
    assert (np.argsort(-deg, kind="stable") != np.arange(n)).any()


@pytest.mark.parametrize("t", _ALL, ids=_IDS)
def test_reference_meets_contract(t):
    """The fp32 torch reference passes the full acceptance rules on every
    fixture, its normalised errors stay under C/8 (this is where the
    constants are measured), and its picks differ from the exact ones on at
    most half the allowed share."""
    c, r, F64, s64, o, mo, err = _analysis(t)
    print(f"{c.id}: normalised errors {err}")
    assert err["grad"] <= oracle.C_GRAD / 8
    assert err["llh"] <= oracle.C_LLH / 8
    assert err["margin"] <= oracle.C_MARGIN / 8
    assert len(oracle.grad_violations(r["grad"].numpy(), o)) == 0
    assert len(oracle.llh_violations(r["llh"].numpy(), o)) == 0
    rung = oracle.steps_to_rungs(r["best"].numpy(), c.cfg)
    bad, differ = oracle.pick_violations(rung, mo)
    assert len(bad) == 0, cf.degree_class(c.label, c.graph, bad)
    n = c.graph.num_nodes
    assert len(differ) <= 0.5 * oracle.PICK_CAP[c.dtype] * n, len(differ)
    assert oracle.pick_cap_ok(len(differ), n, c.dtype)
    # pad columns of the reference grad are exactly zero too
    assert not r["grad"][:, c.k:].any()


def test_contract_constants_are_the_measured_ones():
    """C = 8 x the largest normalised reference error over ALL fixtures,
    rounded up to a power of two.  The maximum moves a little with the
    host's vector width (torch's fp32 sum order and exp/log1p differ), so
    the constant must cover this host's maximum and may exceed its 8x by at
    most the power-of-two rounding plus one binade."""
    mx = dict(grad=0.0, llh=0.0, margin=0.0)
    where = {}
    for t in _ALL:
        err = _analysis(t)[-1]
        for k in mx:
            if err[k] > mx[k]:
                mx[k], where[k] = err[k], cf.case_id(t)
    print("measured maxima:", mx, where)
    for k, c in (("grad", oracle.C_GRAD), ("llh", oracle.C_LLH),
                 ("margin", oracle.C_MARGIN)):
        assert c == 2.0 ** round(np.log2(c))
        assert 8 * mx[k] <= c < 32 * mx[k], (k, mx[k], c)
        assert c == 2.0 ** np.ceil(np.log2(8 * oracle.MEASURED_MAX[k]))


# --- sharpness: the torch reference, mutated, must FAIL the comparison ---
_SHARP = [("small", "dense", "fp32", 65), ("small", "dense", "bf16", 5000),
          ("hub", "capped", "fp32", 68), ("hub", "saturated", "bf16", 264)]
_SHARP_IDS = [cf.case_id(t) for t in _SHARP]


def _fails(c, o, grad, llh):
    return (len(oracle.grad_violations(grad.numpy(), o))
            + len(oracle.llh_violations(llh.numpy(), o))) > 0


@pytest.mark.parametrize("t", _SHARP, ids=_SHARP_IDS)
def test_contract_catches_dropped_edge(t):
    """A kernel that skips ONE edge of ONE node fails grad/llh — for the
    deg-1 centre and for the largest hub alike."""
    import torch
    from bigclam.ops import reference as ref_ops

    c, r, F64, s64, o, mo, err = _analysis(t)
    g = c.graph
    for d in (1, 17, max(c.label)):
        u = int(np.flatnonzero(c.label == d)[0])
        e = int(g.indptr[u + 1]) - 1  # u's last edge
        indices = np.delete(g.indices, e)
        indptr = g.indptr.copy()
        indptr[u + 1:] -= 1
        grad, llh = ref_ops.edge_grad_llh(
            r["F"], torch.from_numpy(indptr), torch.from_numpy(indices).int(),
            r["sumF"], c.cfg)
        assert _fails(c, o, grad, llh), f"dropped edge of deg-{d} node passes"
        bad_rows = set(oracle.grad_violations(grad.numpy(), o)[:, 0].tolist())
        assert bad_rows <= {u}


@pytest.mark.parametrize("t", _SHARP, ids=_SHARP_IDS)
def test_contract_catches_missing_k_tail(t):
    """A kernel that drops the last 4 columns of ONE neighbour row fails."""
    import torch
    from bigclam.ops import reference as ref_ops

    c, r, F64, s64, o, mo, err = _analysis(t)
    g = c.graph
    deg = g.degrees()
    leaves = np.flatnonzero((c.label == -1) & (deg >= 2))
    tail = np.abs(F64[leaves, max(c.k - 4, 0): c.k]).sum(axis=1)
    v = int(leaves[np.argmax(tail)])
    F = r["F"].clone()
    F[v, max(c.k - 4, 0): c.k] = 0
    grad, llh = ref_ops.edge_grad_llh(F, r["indptr"], r["indices"], r["sumF"],
                                      c.cfg)
    # only v's neighbours read the row as fv (v's own row is not judged)
    nb = g.indices[g.indptr[v]: g.indptr[v + 1]]
    viol = oracle.grad_violations(grad.numpy(), o)
    assert len(set(viol[:, 0].tolist()) & set(nb.tolist())) > 0


# `saturated` is left out here on purpose: with every edge on the min_p
# clamp the trial value is llh + s|g|^2 until the F-clamp bites, and since
# beta >= alpha the rung after the exact pick also clears the previous
# rung's threshold — the swapped implementation returns the SAME picks, so
# there is nothing to catch.  The short ladder takes its place.
_SWAP = _SHARP[:3] + [("hub", "short", "fp32", 260)]


@pytest.mark.parametrize("t", _SWAP, ids=[cf.case_id(t) for t in _SWAP])
def test_contract_catches_swapped_rungs(t):
    """Trial values of adjacent rungs exchanged (j <-> j^1) fail the pick
    rules."""
    c, r, F64, s64, o, mo, err = _analysis(t)
    tr = r["trials"].clone()
    J = tr.shape[1]
    idx = np.arange(J) ^ 1
    tr = tr[:, idx]
    rung = cf.picks_from_trials(tr, r["llh"], r["grad"], c.cfg)
    bad, differ = oracle.pick_violations(rung, mo)
    assert len(bad) > 0
    # and the unswapped trials pass
    rung0 = cf.picks_from_trials(r["trials"], r["llh"], r["grad"], c.cfg)
    assert len(oracle.pick_violations(rung0, mo)[0]) == 0


def test_contract_catches_missing_upper_clamp():
    """Phase B and the commit without the max_f clamp fail on `capped`."""
    import dataclasses

    for t in [x for x in cf.c2_cases() if x[1] == "capped"]:
        c, r, F64, s64, o, mo, err = _analysis(t)
        loose = dataclasses.replace(c.cfg, max_f=1e30)
        tr = cf.ref_trials(r["F"], r["indptr"], r["indices"], r["sumF"],
                           r["grad"], loose)
        rung = cf.picks_from_trials(tr, r["llh"], r["grad"], c.cfg)
        bad, differ = oracle.pick_violations(rung, mo)
        assert len(bad) > 0, c.id
