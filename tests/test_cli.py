"""CLI end-to-end tests (CPU): fit -> communities + checkpoint -> extract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bigclam.io import planted_partition

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_edgelist(path, g):
    with open(path, "w") as f:
        f.write("# test graph\n")
        for u in range(g.num_nodes):
            for v in g.neighbors(u):
                if u < v:
                    f.write(f"{g.raw_ids[u]} {g.raw_ids[v]}\n")


def _run(args):
    return subprocess.run(
        [sys.executable, "-m", "bigclam"] + args,
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=300,
    )


def test_cli_fit_and_extract(tmp_path):
    g, _ = planted_partition(3, 12, p_in=0.5, p_out=0.02, seed=21)
    edges = tmp_path / "g.txt"
    _write_edgelist(edges, g)
    out = tmp_path / "coms.txt"
    ckpt = tmp_path / "ckpt"
    metrics = tmp_path / "metrics.jsonl"
    r = _run(
        [
            "fit",
            str(edges),
            "--k",
            "3",
            "--device",
            "cpu",
            "--max-sweeps",
            "10",
            "--init",
            "random",
            "--out",
            str(out),
            "--checkpoint-dir",
            str(ckpt),
            "--metrics",
            str(metrics),
            "--quiet",
        ]
    )
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["k"] == 3 and np.isfinite(res["llh"])
    assert out.exists() and ckpt.exists()
    # metrics JSONL has per-sweep records
    lines = [json.loads(l) for l in open(metrics)]
    assert any("llh" in l for l in lines)
    # community lines parse: "<cid>: id id id"
    for line in open(out):
        cid, rest = line.split(":", 1)
        int(cid)
        assert all(tok.isdigit() for tok in rest.split())

    # extract from the checkpoint reproduces a valid output
    out2 = tmp_path / "coms2.txt"
    r2 = _run(["extract", str(ckpt), str(edges), "--out", str(out2)])
    assert r2.returncode == 0, r2.stderr
    assert out2.read_text() == out.read_text()


def test_cli_select_k(tmp_path):
    g, _ = planted_partition(3, 10, p_in=0.6, p_out=0.02, seed=22)
    edges = tmp_path / "g.txt"
    _write_edgelist(edges, g)
    r = _run(
        [
            "select-k",
            str(edges),
            "--device",
            "cpu",
            "--max-sweeps",
            "8",
            "--k-min",
            "2",
            "--k-max",
            "6",
            "--k-div",
            "3",
            "--quiet",
        ]
    )
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert "grid" in res and res["grid"][0] == 2


def test_cli_bench_delegates(capfd):
    """`python -m bigclam bench` forwards to the repo-root harness and
    prints the driver-contract JSON line."""
    import json as _json

    from bigclam.cli import main

    main([
        "bench", "--steps", "1", "--warmup", "0", "--nodes", "400",
        "--edges", "1200", "--k", "16",
    ])
    out = capfd.readouterr().out.strip().splitlines()[-1]
    rec = _json.loads(out)
    # the full driver contract (BASELINE metric + required fields)
    assert rec["metric"] == "edges/sec per grad iter"
    assert rec["steps"] == 1 and rec["n_gpus"] == 1
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "strong"
    assert rec["unit"] == "edges/s"
    assert rec["dtype"] in ("bf16", "fp32")
    assert rec["data"] == "synthetic"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert "parallelism" in rec["config"] and "k" in rec["config"]


_BENCH_TINY = [
    "bench", "--steps", "2", "--warmup", "1", "--nodes", "400",
    "--edges", "1200", "--k", "16",
]


def test_bench_plain_vs_full(capfd):
    """A plain run measures the headline dtype only; --full adds the
    second-dtype variant next to it."""
    import json as _json

    from bigclam.cli import main

    main(_BENCH_TINY)
    plain = _json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert plain["variants"] == {}
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0
    main(_BENCH_TINY + ["--full"])
    full = _json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert full["dtype"] == plain["dtype"] == "bf16"
    assert full["variants"]["fp32"]["value"] > 0
    assert full["variants"]["fp32"]["ms_per_step"] > 0


def test_bench_dump_outputs(tmp_path, capfd, monkeypatch):
    """--dump-outputs writes the last timed sweep's arrays as float .npy
    files, identical from run to run (seeded graph + init), and they are
    the outputs of exactly --steps sweeps after --warmup.  Pinned to the
    CPU path (also on a GPU box) so the hand-driven run below is
    bit-comparable."""
    import numpy as np
    import torch

    from bigclam.cli import main
    from bigclam.config import BigClamConfig
    from bigclam.engine.trainer import Trainer
    from bigclam.io import shaped_graph

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    args = _BENCH_TINY + ["--dtype", "fp32"]
    a, b = tmp_path / "a", tmp_path / "b"
    main(args + ["--dump-outputs", str(a)])
    main(args + ["--dump-outputs", str(b)])
    capfd.readouterr()
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    assert {"llh.npy", "steps.npy", "steps_next.npy", "grad_rows.npy",
            "F_rows.npy", "sumF.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64)
        assert np.isfinite(x).all()
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20

    # the same 1 warmup + 2 timed sweeps, driven by hand
    g = shaped_graph(400, 1200, locality=0.7, seed=42)
    cfg = BigClamConfig(k=16, dtype="fp32", device="cpu", seed=7)
    tr = Trainer(g, cfg, rank=0, world_size=1, device=torch.device("cpu"))
    tr.init_F("random")
    carry, _ = tr.prologue()
    for _ in range(3):
        carry, llh, steps = tr.pipelined_sweep(carry)
    rows = np.load(a / "matrix_rows.npy").astype(np.int64)
    vrows = np.load(a / "vector_rows.npy").astype(np.int64)
    assert np.load(a / "llh.npy")[0] == llh
    np.testing.assert_array_equal(np.load(a / "steps.npy"),
                                  steps.numpy()[vrows])
    np.testing.assert_array_equal(np.load(a / "steps_next.npy"),
                                  carry[1].numpy()[vrows])
    np.testing.assert_array_equal(np.load(a / "grad_rows.npy"),
                                  carry[0].numpy()[rows][:, :16])
    np.testing.assert_array_equal(np.load(a / "F_rows.npy"),
                                  tr.state.F_local_k.numpy()[rows])


def test_cli_fit_resume(tmp_path):
    """CLI --resume continues a checkpointed fit: the resumed run picks up
    the saved sweep/llh and matches an uninterrupted run's final LLH."""
    g, _ = planted_partition(3, 12, p_in=0.5, p_out=0.02, seed=23)
    edges = tmp_path / "g.txt"
    _write_edgelist(edges, g)
    base = ["fit", str(edges), "--k", "3", "--device", "cpu",
            "--init", "random", "--quiet"]
    # uninterrupted 8-sweep run
    r_full = _run(base + ["--max-sweeps", "8", "--tol", "0"])
    assert r_full.returncode == 0, r_full.stderr
    llh_full = json.loads(r_full.stdout.strip().splitlines()[-1])["llh"]
    # 4 sweeps -> checkpoint -> resume 4 more
    ck = tmp_path / "ck"
    r1 = _run(base + ["--max-sweeps", "4", "--tol", "0",
                      "--checkpoint-dir", str(ck)])
    assert r1.returncode == 0, r1.stderr
    # max-sweeps counts sweeps RUN THIS INVOCATION (4 more -> 8 total)
    r2 = _run(base + ["--max-sweeps", "4", "--tol", "0",
                      "--resume", str(ck)])
    assert r2.returncode == 0, r2.stderr
    res2 = json.loads(r2.stdout.strip().splitlines()[-1])
    assert res2["llh"] == pytest.approx(llh_full, rel=1e-12)
