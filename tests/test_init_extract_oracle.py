"""K5 / K6 / K7 contract on the CPU (docs/kernels.md, "K5 / K6 / K7
contract"): the host reference implementations equal the exact oracles of
tests/oracle.py on every fixture, the fixtures reach the kernel edges they
were built for, and every listed mutation of a kernel-shaped stand-in
disagrees with the oracle on the fixture named next to it.  Every
comparison is exact equality.
"""
import numpy as np
import pytest
import torch

import contract_fixtures as cf
import oracle
from bigclam.core.init import (
    conductance_ranking,
    conductance_ranking_device,
    conductances,
    seed_init_local_F,
)
from bigclam.engine.extract import local_memberships

K7_IDS = [cf.k7_id(t) for t in cf.k7_cases()]
K5_NAMES = ("ladder-small", "ladder-hub", "K2", "K3", "K65", "K66",
            "star257", "two-K20", "clique-ladder", "rmat9")


# ----------------------------------------------------------------------- K7
def k7_model(F, k_true, delta, mut=None):
    """K7 as the kernel computes it: 256 threads, thread i owns the columns
    [min(i chunk, K), min(i chunk + chunk, K)) and emits its members in
    thread order.  ``F``: fp64 [n, ld].  ``mut`` selects one deliberate
    defect."""
    n, ld = F.shape
    K = ld if mut == "pads-included" else k_true
    chunk = -(-K // cf.K7_BLOCK)
    cols = []
    for i in range(cf.K7_BLOCK):
        c0 = min(i * chunk, K)
        c1 = min(c0 + chunk, K)
        if mut == "last-chunk-unclipped" and c0 < K and c0 + chunk >= K:
            c1 = c0 + chunk
        own = list(range(c0, c1))
        cols += own[::-1] if mut == "reversed-in-chunk" else own
    cols = np.asarray(cols, dtype=np.int64)
    t = float(delta) if mut == "fp64-threshold" else float(np.float32(delta))
    flat = np.concatenate([F.ravel(), np.zeros(chunk)])  # reads past the end
    counts = np.zeros(n, dtype=np.int64)
    comms = []
    for u in range(n):
        vals = flat[u * ld + cols]
        mem = vals > t if mut == "gt-not-ge" else vals >= t
        if not mem.any() and vals.max() > 0:
            mem = vals == vals.max()
            if mut == "first-argmax-only":
                mem = np.arange(len(cols)) == np.flatnonzero(mem)[0]
        counts[u] = int(mem.sum())
        comms.append(cols[mem])
    return counts, np.concatenate(comms).astype(np.int32)


def _rows_differing(got, want):
    """Row indices on which two (counts, comms) results differ."""
    (gc, gm), (wc, wm) = got, want
    go = np.concatenate([[0], np.cumsum(gc)])
    wo = np.concatenate([[0], np.cumsum(wc)])
    return [u for u in range(len(wc))
            if not np.array_equal(gm[go[u]:go[u + 1]], wm[wo[u]:wo[u + 1]])]


@pytest.mark.parametrize("t", cf.k7_cases(), ids=K7_IDS)
def test_k7_reference_matches_oracle(t):
    k_true, kp, dtype = t
    F = cf.k7_rows(*t)
    counts, comms = local_memberships(F, k_true, cf.K7_DELTA, use_hip=False)
    wc, wm = cf.k7_oracle(*t)
    np.testing.assert_array_equal(counts, wc)
    np.testing.assert_array_equal(comms, wm)
    assert comms.dtype == np.int32 and counts.dtype == np.int64
    # the kernel-shaped stand-in without a defect is the oracle too
    mc, mm = k7_model(F.double().numpy(), k_true, cf.K7_DELTA)
    np.testing.assert_array_equal(mc, wc)
    np.testing.assert_array_equal(mm, wm)


def test_k7_fixture_conditions():
    chunks = {cf.k7_chunk(t[0]) for t in cf.k7_cases()}
    assert chunks == {1, 2, 3, 20, 98}
    for t in cf.k7_cases():
        k_true, kp, dtype = t
        F = cf.k7_rows(*t)
        names = cf.k7_row_names(*t)
        wc, _ = cf.k7_oracle(*t)
        assert F.shape == (len(names), kp) and len(names) <= 64
        assert ("pads-only" in names) == (kp > k_true)
        by = dict(zip(names, wc.tolist()))
        assert by["zero"] == 0 and by["member-all"] == k_true
        assert by["exact-t"] == 1 and by["just-below-t"] == 1
        assert by["fallback-all-tied"] == k_true
        assert by["fallback-min-normal"] == 1
        assert by.get("pads-only", 0) == 0
        assert by["fallback-tie-across-threads"] == min(2, k_true)
        if cf.k7_chunk(k_true) > 1:
            assert by["fallback-tie-in-chunk"] == 2
        # consecutive offsets repeat at the tail
        assert wc[-6:].tolist() == [0, k_true] * 3
    # float32(delta) < delta: the fp32 rule and an fp64 comparison differ
    v = cf.k7_values("fp32")
    assert v["at"] == float(np.float32(cf.K7_DELTA)) < cf.K7_DELTA


# mutation -> (fixture, row) on which it must disagree with the oracle
K7_SHARP = {
    "gt-not-ge": ((257, 260, "fp32"), "member-every-chunk-end"),
    "fp64-threshold": ((5000, 5000, "fp32"), "member-every-chunk-end"),
    "first-argmax-only": ((5000, 5000, "bf16"), "fallback-tie-bf16-word"),
    "pads-included": ((257, 264, "bf16"), "pads-only"),
    "reversed-in-chunk": ((25000, 25000, "bf16"), "fallback-tie-in-chunk"),
    "last-chunk-unclipped": ((257, 281, "fp32"), "fallback-col0"),
}


@pytest.mark.parametrize("mut", sorted(K7_SHARP))
def test_k7_sharpness(mut):
    t, row = K7_SHARP[mut]
    assert t in cf.k7_cases()
    F = cf.k7_rows(*t).double().numpy()
    got = k7_model(F, t[0], cf.K7_DELTA, mut)
    bad = _rows_differing(got, cf.k7_oracle(*t))
    names = cf.k7_row_names(*t)
    assert row in [names[u] for u in bad], (
        f"{mut} not caught by {cf.k7_id(t)}/{row}; differing rows: "
        f"{[names[u] for u in bad]}")


# ----------------------------------------------------------------------- K5
def k5_model(g, mut=None):
    """K5 as the kernel computes it: per node u, every neighbour v's row is
    walked, an endpoint w is inside iff w == u or a search of u's sorted
    row finds it; one double division at the end."""
    indptr, indices = g.indptr, g.indices
    total = len(indices)
    out = np.zeros(g.num_nodes, dtype=np.float64)
    for u in range(g.num_nodes):
        nu = indices[indptr[u]:indptr[u + 1]]
        deg = len(nu)
        if deg == 0:
            continue
        srch = {"search-drops-last": nu[:-1],
                "search-drops-first": nu[1:]}.get(mut, nu)
        z, cut = deg, 0
        for i, v in enumerate(nu):
            if mut == "every-fifth-edge-skipped" and i % 5 == 4:
                continue
            row = indices[indptr[v]:indptr[v + 1]]
            z += len(row)
            if mut == "element-64-skipped" and len(row) > 64:
                row = np.delete(row, 64)
            inside = np.isin(row, srch)
            if mut != "self-not-inside":
                inside |= row == u
            cut += int(np.count_nonzero(~inside))
        vol_s = z - cut
        vol_t = total - vol_s - 2 * cut
        if vol_s == 0:
            out[u] = 0.0
        elif vol_t == 0:
            out[u] = 1.0
        else:
            out[u] = np.float64(cut) / np.float64(max(min(vol_s, vol_t), 1))
    return out


def test_k5_graph_names():
    assert tuple(cf.k5_graphs()) == K5_NAMES


@pytest.mark.parametrize("name", K5_NAMES)
def test_k5_host_conductances_bitwise(name):
    g = cf.k5_graphs()[name]
    o = cf.k5_oracle(name)
    np.testing.assert_array_equal(np.diff(g.indptr), o["deg"])
    assert np.array_equal(conductances(g), o["cond"])
    assert np.array_equal(k5_model(g), o["cond"])
    # the loop oracle of tests/oracle.py (no max(.., 1) guard either)
    if g.num_nodes <= 160:
        old = [oracle.conductance(g.indptr, g.indices, u, len(g.indices))
               for u in range(g.num_nodes)]
        assert np.array_equal(np.asarray(old, dtype=np.float64), o["cond"])


@pytest.mark.parametrize("name", K5_NAMES)
def test_k5_ranking_device_on_cpu_matches_host(name):
    g = cf.k5_graphs()[name]
    cond = cf.k5_oracle(name)["cond"]
    host = conductance_ranking(g, cond=cond)
    dev = conductance_ranking_device(g, torch.from_numpy(cond))
    np.testing.assert_array_equal(dev, host)


def test_k5_fixture_conditions():
    cf.assert_k5_fixture_conditions()
    # tie-heavy: far fewer distinct conductances than nodes
    for name in ("ladder-small", "ladder-hub", "clique-ladder"):
        cond = cf.k5_oracle(name)["cond"]
        assert len(np.unique(cond)) < len(cond) // 3


# mutation -> the graph on which it must disagree with the oracle
K5_SHARP = {
    "search-drops-last": "K65",
    "search-drops-first": "K66",
    "self-not-inside": "K3",
    "element-64-skipped": "star257",
    "every-fifth-edge-skipped": "ladder-small",
}


@pytest.mark.parametrize("mut", sorted(K5_SHARP))
def test_k5_sharpness(mut):
    name = K5_SHARP[mut]
    got = k5_model(cf.k5_graphs()[name], mut)
    assert not np.array_equal(got, cf.k5_oracle(name)["cond"]), (
        f"{mut} not caught by {name}")


# ----------------------------------------------------------------------- K6
def k6_model(g, seeds, start, stop, kp, include_seed, fill, mut=None):
    """K6 as the kernel computes it, on a flat buffer with one spare row
    after the shard (where an accepted v == stop lands).  Returns
    [stop - start + 1, kp]."""
    n_local = stop - start
    buf = np.full((n_local + 1) * kp, float(fill), dtype=np.float64)
    for c, s in enumerate(seeds):
        s = int(s)
        col = c % 256 if mut == "column-mod-256" else c
        for v in g.indices[g.indptr[s]:g.indptr[s + 1]]:
            v = int(v)
            hi_ok = v <= stop if mut == "stop-accepted" else v < stop
            if v >= start and hi_ok:
                buf[(v - start) * kp + col] = 1.0
        if (include_seed or mut == "seed-always-written") and start <= s < stop:
            buf[(s - start) * kp + col] = 1.0
    return buf.reshape(n_local + 1, kp)


def _k6_cases():
    return [(ns, sh, inc) for ns in sorted(cf.K6_KP)
            for sh in cf.k6_all_shards() for inc in (False, True)]


def _k6_id(c):
    return f"{c[0]}seeds-rows{c[1][0]}:{c[1][1]}-{'incl' if c[2] else 'excl'}"


def test_k6_host_matches_scatter():
    g, label = cf.ladder_graph("hub")
    for ns, (a, b), inc in _k6_cases():
        seeds = cf.k6_seed_lists()[ns]
        host = seed_init_local_F(g, ns, a, b, seeds=seeds, include_seed=inc)
        want = cf.k6_oracle(ns, (a, b), inc, 0.0)
        assert host.shape == (b - a, ns)
        assert np.array_equal(host.astype(np.float64), want[:, :ns]), (
            _k6_id((ns, (a, b), inc)))
        assert not want[:, ns:].any()  # n_seeds < kp: pad columns untouched
        assert np.array_equal(
            k6_model(g, seeds, a, b, cf.K6_KP[ns], inc, 0.25)[:-1],
            cf.k6_oracle(ns, (a, b), inc, 0.25))


def test_k6_fixture_conditions():
    g, label = cf.ladder_graph("hub")
    lists = cf.k6_seed_lists()
    assert sorted(lists) == [8, 37, 600] and cf.K6_KP == {8: 8, 37: 40, 600: 608}
    deg = np.diff(g.indptr)
    for ns, seeds in lists.items():
        assert deg[seeds[:6]].tolist() == [1, 255, 256, 257, 513, 600]
        assert label[seeds[6]] == -1 and label[seeds[7]] == -2
    assert len(set(lists[600].tolist())) < 600  # nodes repeat
    sh = cf.k6_shards()
    (_, a), (a2, b), (b2, n) = sh["split"]
    assert a == a2 and b == b2 and n == g.num_nodes and sh["empty"] == (a, a)
    nbrs = set()
    for s in lists[8]:
        nbrs |= set(g.neighbors(int(s)).tolist())
    assert {a, b - 1, b} <= nbrs  # on start, stop - 1 and stop
    # the three shards stacked are the whole-graph result
    for ns in lists:
        for inc in (False, True):
            parts = [cf.k6_oracle(ns, s, inc, 0.25) for s in sh["split"]]
            assert np.array_equal(np.concatenate(parts),
                                  cf.k6_oracle(ns, sh["full"], inc, 0.25))


def _k6_mid():
    return cf.k6_shards()["split"][1]


# mutation -> (number of seeds, shard, include_seed) on which it must fail
K6_SHARP = {
    "stop-accepted": lambda: (8, _k6_mid(), False),
    "seed-always-written": lambda: (8, cf.k6_shards()["full"], False),
    "column-mod-256": lambda: (600, cf.k6_shards()["full"], False),
}


@pytest.mark.parametrize("mut", sorted(K6_SHARP))
def test_k6_sharpness(mut):
    ns, (a, b), inc = K6_SHARP[mut]()
    g, _ = cf.ladder_graph("hub")
    got = k6_model(g, cf.k6_seed_lists()[ns], a, b, cf.K6_KP[ns], inc, 0.25,
                   mut)
    want = cf.k6_oracle(ns, (a, b), inc, 0.25)
    spare_clean = (got[-1] == 0.25).all()
    assert not (np.array_equal(got[:-1], want) and spare_clean), (
        f"{mut} not caught by {_k6_id((ns, (a, b), inc))}")
