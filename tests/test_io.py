import numpy as np
import pytest

from bigclam.io import build_graph, load_graph, planted_partition, rmat_graph
from bigclam.io.edgelist import parse_edge_array


def test_build_graph_dedup_and_remap():
    # duplicate edges (both directions), self loop, gappy raw ids
    edges = np.array([[10, 20], [20, 10], [10, 30], [30, 30], [20, 30], [10, 20]])
    g = build_graph(edges)
    assert g.num_nodes == 3
    assert g.num_edges == 3
    assert g.num_directed_edges == 6
    assert list(g.raw_ids) == [10, 20, 30]
    # node 0 (raw 10) neighbors: raw 20, 30 -> internal 1, 2
    assert sorted(g.neighbors(0).tolist()) == [1, 2]
    # symmetric
    for u in range(3):
        for v in g.neighbors(u):
            assert u in g.neighbors(int(v))


def test_rows_sorted():
    g, _ = planted_partition(2, 10, seed=1)
    for u in range(g.num_nodes):
        nb = g.neighbors(u).tolist()
        assert nb == sorted(nb)
        assert len(set(nb)) == len(nb)
        assert u not in nb


def test_parse_file(tmp_path):
    p = tmp_path / "edges.txt"
    p.write_text("# a comment\n# another\n1 2\n2 3\n3\t1\n")
    arr = parse_edge_array(str(p))
    assert arr.shape == (3, 2)
    g = load_graph(str(p))
    assert g.num_nodes == 3
    assert g.num_edges == 3


def test_parse_file_messy(tmp_path):
    """Real-world edge-list quirks: CRLF line endings, repeated tabs and
    spaces, leading whitespace, blank lines, no trailing newline."""
    p = tmp_path / "messy.txt"
    p.write_bytes(
        b"# header\r\n"
        b"\r\n"
        b"1\t\t2\r\n"
        b"  2   3\n"
        b"\n"
        b"3\t 1"
    )
    arr = parse_edge_array(str(p))
    assert arr.shape == (3, 2)
    g = load_graph(str(p))
    assert g.num_nodes == 3
    assert g.num_edges == 3


def test_rmat_properties():
    g = rmat_graph(10, 8.0, seed=3)
    assert g.num_nodes <= 1024
    assert g.num_edges > 1000
    deg = g.degrees()
    assert deg.min() >= 1
    # power-law-ish: max degree well above mean
    assert deg.max() > 5 * deg.mean()


def test_rmat_with_target_edges():
    from bigclam.io import rmat_graph_with_edges

    g = rmat_graph_with_edges(2000, 8000, seed=5)
    assert g.num_edges == 8000


def test_planted_partition_labels():
    g, labels = planted_partition(3, 15, p_in=0.6, p_out=0.01, seed=2)
    assert g.num_nodes <= 45
    assert len(labels) == 45


def test_shaped_graph_exact_counts():
    from bigclam.io import shaped_graph

    g = shaped_graph(5000, 14000, seed=9)
    assert g.num_nodes == 5000
    assert g.num_edges == 14000
    assert g.degrees().min() >= 1
    assert g.degrees().max() > 20  # heavy tail present


import os
import pytest as _pytest

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@_pytest.fixture(scope="session")
def snap_files(tmp_path_factory):
    """The two SNAP datasets the reference ships, re-materialized as
    edge-list text from the stored edge arrays (tests/golden/*.edges.npz:
    every line of the original files, in file order, as uint16 id pairs).
    Email-Enron keeps its '#' header, tab separators and CRLF line ends;
    facebook_combined is space-separated with no header."""
    import numpy as np

    d = tmp_path_factory.mktemp("snap")
    enron = np.load(os.path.join(_GOLDEN, "Email-Enron.edges.npz"))["edges"]
    with open(d / "Email-Enron.txt", "w", newline="") as f:
        f.write(
            "# Directed graph (each unordered pair of nodes is saved once): "
            "Email-Enron.txt \r\n"
            "# Enron email network (edge indicated that email was exchanged, "
            "undirected edges)\r\n"
            "# Nodes: 36692 Edges: 367662\r\n"
            "# FromNodeId\tToNodeId\r\n"
        )
        f.write("".join(f"{a}\t{b}\r\n" for a, b in enron.tolist()))
    fb = np.load(os.path.join(_GOLDEN, "facebook_combined.edges.npz"))["edges"]
    with open(d / "facebook_combined.txt", "w", newline="") as f:
        f.write("".join(f"{a} {b}\n" for a, b in fb.tolist()))
    return str(d)


def test_parse_reference_datasets(snap_files):
    """The two SNAP datasets bundled with the reference parse to their
    documented shapes (Email-Enron header: 36692 nodes / 183831
    undirected edges stored as 367662 directed lines; facebook_combined:
    4039 nodes / 88234 undirected edges, no header)."""
    from bigclam.io import load_graph

    g = load_graph(os.path.join(snap_files, "Email-Enron.txt"))
    assert g.num_nodes == 36692
    assert g.num_edges == 183831  # undirected
    assert len(g.indices) == 2 * 183831

    fb = load_graph(os.path.join(snap_files, "facebook_combined.txt"))
    assert fb.num_nodes == 4039
    assert fb.num_edges == 88234


def test_fit_real_enron_smoke(snap_files):
    """Two sweeps on the REAL Email-Enron graph (CPU): LLH finite and
    improving — the reference's own manual verification procedure
     on its own dataset."""
    import torch

    from bigclam.config import BigClamConfig
    from bigclam.engine.trainer import Trainer
    from bigclam.io import load_graph

    g = load_graph(os.path.join(snap_files, "Email-Enron.txt"))
    cfg = BigClamConfig(k=8, device="cpu", max_sweeps=2, seed=1)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cpu"))
    res = tr.fit(init="random")
    assert len(res.llh_history) == 2
    assert all(l == l for l in res.llh_history)  # finite
    assert res.llh_history[-1] > res.llh_history[0]


def test_fit_facebook_k25_baseline_config(snap_files):
    """BASELINE.json config #1: facebook_combined K=25 on CPU (gloo ws=1
    plumbing config) — converging fit on the real fixture."""
    import numpy as np
    import torch

    from bigclam.config import BigClamConfig
    from bigclam.engine.trainer import Trainer
    from bigclam.io import load_graph

    g = load_graph(os.path.join(snap_files, "facebook_combined.txt"))
    assert g.num_nodes == 4039 and g.num_edges == 88234
    cfg = BigClamConfig(k=25, device="cpu", max_sweeps=4, seed=2)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cpu"))
    res = tr.fit(init="random")
    assert np.isfinite(res.llh)
    assert res.llh > res.llh_history[0]


def test_build_graph_properties_random():
    """Property test over random edge lists: symmetric CSR, sorted rows,
    no self-loops/duplicates, degree sum == 2E."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    from bigclam.io.edgelist import build_graph

    @settings(max_examples=60, deadline=None)
    @given(
        st.lists(
            st.tuples(st.integers(0, 40), st.integers(0, 40)),
            min_size=1,
            max_size=200,
        )
    )
    def check(pairs):
        import numpy as np

        edges = np.array(pairs, dtype=np.int64)
        g = build_graph(edges)
        und = {tuple(sorted(p)) for p in pairs if p[0] != p[1]}
        if not und:
            return
        assert g.num_edges == len(und)
        assert len(g.indices) == 2 * len(und)
        indptr, idx = g.indptr, g.indices
        for u in range(g.num_nodes):
            row = idx[indptr[u]:indptr[u + 1]]
            assert np.all(np.diff(row) > 0), "sorted, no duplicates"
            assert u not in row, "no self-loops"
            for v in row:  # symmetry
                vr = idx[indptr[v]:indptr[v + 1]]
                assert u in vr

    check()


def test_shaped_graph_cross_process_deterministic():
    """bench.py relies on every torchrun rank generating the IDENTICAL
    graph from the seed; verify determinism across fresh processes."""
    import hashlib
    import subprocess
    import sys

    code = (
        "from bigclam.io import shaped_graph\n"
        "import hashlib\n"
        "g = shaped_graph(3000, 9000, locality=0.7, seed=42)\n"
        "h = hashlib.sha256()\n"
        "h.update(g.indptr.tobytes()); h.update(g.indices.tobytes())\n"
        "print(h.hexdigest())\n"
    )
    outs = {
        subprocess.run(
            [sys.executable, "-c", code], capture_output=True, text=True,
            check=True,
        ).stdout.strip()
        for _ in range(2)
    }
    assert len(outs) == 1, outs


def test_native_csr_matches_numpy(monkeypatch):
    """Parallel native build_csr == the numpy reference path exactly
    (dups, self-loops, sparse id space) and is thread-count invariant."""
    import numpy as np

    from bigclam import _io_native
    from bigclam.io.edgelist import build_graph

    rng = np.random.default_rng(5)
    ids = rng.choice(100000, size=3000, replace=False)
    e = ids[rng.integers(0, 3000, size=(50000, 2))]
    monkeypatch.setenv("BIGCLAM_NATIVE_CSR", "1")
    g1 = build_graph(e)
    monkeypatch.setenv("BIGCLAM_NATIVE_CSR", "0")
    g2 = build_graph(e)
    np.testing.assert_array_equal(g1.indptr, g2.indptr)
    np.testing.assert_array_equal(g1.indices, g2.indices)
    np.testing.assert_array_equal(g1.raw_ids, g2.raw_ids)
    ip1, ix1, rid1 = _io_native.build_csr(np.ascontiguousarray(e), True, 1)
    np.testing.assert_array_equal(np.asarray(ip1), g1.indptr)
    np.testing.assert_array_equal(np.asarray(ix1), g1.indices)


def test_native_rmat_deterministic():
    """Counter-based native R-MAT: same output for any thread count."""
    import numpy as np

    from bigclam import _io_native

    a = np.asarray(_io_native.rmat_edges(12, 4.0, 0.57, 0.19, 0.19, 7, 1))
    b = np.asarray(_io_native.rmat_edges(12, 4.0, 0.57, 0.19, 0.19, 7, 8))
    np.testing.assert_array_equal(a, b)
    assert a.shape == (4 * (1 << 12), 2)
    assert a.min() >= 0 and a.max() < (1 << 12)
    # power-law-ish: the scramble keeps hubs (distinct counts sane)
    from bigclam.io.edgelist import build_graph

    g = build_graph(a)
    assert g.degrees().max() > 5 * g.degrees().mean()


def test_empty_graph_friendly_error(tmp_path):
    """A file with only comments/self-loops produces a clear error at
    Trainer construction instead of an obscure downstream crash."""
    import pytest as _pytest
    import torch

    from bigclam.config import BigClamConfig
    from bigclam.engine.trainer import Trainer
    from bigclam.io.edgelist import load_graph

    p = tmp_path / "empty.txt"
    p.write_text("# only a comment\n7 7\n")
    g = load_graph(str(p))
    assert g.num_nodes == 0
    with _pytest.raises(ValueError, match="empty graph"):
        Trainer(g, BigClamConfig(k=4, device="cpu"), rank=0, world_size=1,
                device=torch.device("cpu"))


@pytest.mark.parametrize(
    "name,edges",
    [
        ("star_hub", [[0, i] for i in range(1, 1001)]),
        ("dup_heavy", [[1, 2], [2, 1], [1, 2], [3, 3], [2, 3]] * 10),
        ("single_edge", [[7, 9]]),
        # sparse 64-bit-ish id space just under the native builder's
        # 2^31 presence-bitmap bound (io_native.cpp build_csr)
        ("boundary_ids", [[0, 1 << 27], [5, 1 << 27], [0, 5], [123456789, 5]]),
    ],
)
def test_native_csr_adversarial_shapes(monkeypatch, name, edges):
    """Native build_csr == numpy reference on hub rows, heavy duplication,
    minimal inputs and sparse high-id spaces (same dedupe/self-loop/remap
    semantics, bit-identical CSR)."""
    pytest.importorskip("bigclam._io_native")
    e = np.asarray(edges, dtype=np.int64)
    monkeypatch.setenv("BIGCLAM_NATIVE_CSR", "1")
    g1 = build_graph(e)
    monkeypatch.setenv("BIGCLAM_NATIVE_CSR", "0")
    g2 = build_graph(e)
    np.testing.assert_array_equal(g1.indptr, g2.indptr)
    np.testing.assert_array_equal(g1.indices, g2.indices)
    np.testing.assert_array_equal(g1.raw_ids, g2.raw_ids)


def test_native_csr_large_id_fallback(monkeypatch):
    """Raw ids >= 2^31 must take the numpy path (the native builder's
    presence bitmap cannot cover them) and still build correctly."""
    e = np.array([[1 << 33, 4], [4, 1 << 40], [1 << 33, 1 << 40]], dtype=np.int64)
    monkeypatch.setenv("BIGCLAM_NATIVE_CSR", "1")
    g = build_graph(e)
    assert g.num_nodes == 3 and g.num_edges == 3
    assert list(g.raw_ids) == [4, 1 << 33, 1 << 40]
