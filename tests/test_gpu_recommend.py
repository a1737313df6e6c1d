"""K11 (k11_topn_links) on the GPU: bitwise agreement with the CPU
implementation on ids, scores and candidate counts — there is no tolerance
in this feature — across the LDS and the global-table path, the edge
fixture, random models, reproducibility, the wrapper's validation and an
end-to-end fit with a hold-out split."""
import numpy as np
import pytest
import torch

import link_fixtures as lfx
from bigclam.config import BigClamConfig
from bigclam.core.sparse_model import SparseModel
from bigclam.engine.recommend import (
    gather_sparse_model,
    heldout_ranking,
    recommend,
    recommend_trainer,
)
from bigclam.engine.trainer import Trainer
from bigclam.io import planted_overlap
from bigclam.io.holdout import split_edges
from bigclam.ops.links_cpu import topn_links_cpu

pytestmark = pytest.mark.gpu

NAMES = ("top_id", "top_score", "n_cand")
DTYPES = (np.int32, np.float32, np.int32)


def _cpu(F, graph, q, n):
    model = SparseModel.from_F(torch.from_numpy(F))
    return topn_links_cpu(model, graph.indptr, graph.indices, q, n)


def _device_args(F, graph, q):
    dev = torch.device("cuda")
    return (SparseModel.from_F(torch.from_numpy(F).to(dev)),
            torch.from_numpy(graph.indptr).to(dev),
            torch.from_numpy(graph.indices).to(dev),
            torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(dev))


def _gpu(F, graph, q, n, **kw):
    from bigclam.ops import hip as hip_ops

    *out, info = hip_ops.topn_links(*_device_args(F, graph, q), n, **kw)
    return tuple(t.cpu().numpy() for t in out), info


def _assert_same(cpu, gpu, what):
    for name, dt, c, g in zip(NAMES, DTYPES, cpu, gpu):
        assert g.dtype == dt and c.dtype == dt, f"{what}: {name} dtype"
        assert g.shape == c.shape, f"{what}: {name} shape"
        assert g.tobytes() == c.tobytes(), f"{what}: {name}"


@pytest.fixture(scope="module")
def edge():
    F, graph = lfx.edge_fixture()
    q = lfx.EDGE_QUERIES
    return F, graph, q, {n: _cpu(F, graph, q, n) for n in (1, 10, 64)}


@pytest.mark.parametrize("n", [1, 10, 64])
@pytest.mark.parametrize("lds_slots", [64, 128, None],
                         ids=["lds64", "lds128", "default-lds"])
def test_edge_fixture(edge, lds_slots, n):
    F, graph, q, cpu = edge
    gpu, info = _gpu(F, graph, q, n, lds_slots=lds_slots)
    _assert_same(cpu[n], gpu, f"edge lds_slots={lds_slots} n={n}")
    assert info["n_lds"] + info["n_global"] == len(q)
    if lds_slots == 64:
        assert info["n_lds"] >= 1 and info["n_global"] >= 1
    if lds_slots is None:
        assert info["n_global"] == 0 and info["global_batches"] == 0


@pytest.fixture(scope="module")
def random_inputs():
    out = {}
    for bf16 in (False, True):
        F, graph, q = lfx.random_inputs(seed=7, bf16=bf16)
        out[bf16] = (F, graph, q, _cpu(F, graph, q, 10))
    return out


@pytest.mark.parametrize("lds_slots", [64, None], ids=["lds64", "default-lds"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_random_model(random_inputs, bf16, lds_slots):
    F, graph, q, cpu = random_inputs[bf16]
    if bf16:  # the model is built from bf16 storage, as a bf16 fit's is
        dev = torch.device("cuda")
        stored = torch.from_numpy(F).to(dev).to(torch.bfloat16)
        model = SparseModel.from_F(stored)
        assert model.row_val.dtype == torch.float32
        assert torch.equal(model.row_val,
                           _device_args(F, graph, q)[0].row_val)
    gpu, info = _gpu(F, graph, q, 10, lds_slots=lds_slots)
    _assert_same(cpu, gpu, f"random bf16={bf16} lds_slots={lds_slots}")
    assert (cpu[2] >= 10).any()
    if lds_slots == 64:
        assert info["n_global"] >= 1


def test_reproducible_and_independent_of_the_launch(random_inputs):
    F, graph, q, cpu = random_inputs[False]
    a, _ = _gpu(F, graph, q, 10, lds_slots=64)
    b, _ = _gpu(F, graph, q, 10, lds_slots=64)
    for name, x, y in zip(NAMES, a, b):
        assert x.tobytes() == y.tobytes(), name
    # alone or in the full list, in LDS or in global scratch
    for i in (0, 17, len(q) - 1):
        for lds_slots in (0, None):
            alone, info = _gpu(F, graph, q[i:i + 1], 10, lds_slots=lds_slots)
            assert info["n_global"] == (1 if lds_slots == 0 else 0)
            for name, x, y in zip(NAMES, alone, a):
                assert x[0].tobytes() == y[i].tobytes(), (name, i, lds_slots)
    # a scratch budget that forces several global batches
    many, info = _gpu(F, graph, q, 10, lds_slots=0,
                      scratch_bytes=8 * 4 * info_max_slots(F, graph, q))
    assert info["n_lds"] == 0 and info["global_batches"] > 1
    _assert_same(cpu, many, "batched global tables")
    # another block size
    for block in (64, 128):
        other, _ = _gpu(F, graph, q, 10, lds_slots=64, block=block)
        _assert_same(cpu, other, f"block={block}")


def info_max_slots(F, graph, q):
    return _gpu(F, graph, q, 1)[1]["max_slots"]


def test_wrapper_validation(edge):
    from bigclam.ops import hip as hip_ops

    F, graph, q, _ = edge
    model, indptr, indices, qd = _device_args(F, graph, q)
    max_n = hip_ops.link_max_n()
    assert max_n == 64 == hip_ops.ensure_loaded().LINK_MAX_N
    for bad in (0, max_n + 1):
        with pytest.raises(RuntimeError, match="n must be"):
            hip_ops.topn_links(model, indptr, indices, qd, bad)
    with pytest.raises(RuntimeError, match="dtype"):
        hip_ops.topn_links(model, indptr, indices, qd.long(), 10)
    with pytest.raises(RuntimeError, match="dtype"):
        hip_ops.topn_links(model, indptr, indices.long(), qd, 10)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_ops.topn_links(model, indptr, indices, qd[::2], 10)
    with pytest.raises(RuntimeError, match="GPU"):
        hip_ops.topn_links(model, indptr, indices, qd.cpu(), 10)
    with pytest.raises(RuntimeError, match="GPU"):
        hip_ops.topn_links(model.to("cpu"), indptr, indices, qd, 10)
    for bad in (-1, lfx.EDGE_N):
        qb = qd.clone()
        qb[3] = bad
        with pytest.raises(RuntimeError, match="out of range"):
            hip_ops.topn_links(model, indptr, indices, qb, 10)
    with pytest.raises(RuntimeError, match="lengths"):
        hip_ops.topn_links(model, indptr[:-1].contiguous(), indices, qd, 10)
    with pytest.raises(RuntimeError, match="lds_slots"):
        hip_ops.topn_links(model, indptr, indices, qd, 10, lds_slots=8193)
    with pytest.raises(RuntimeError, match="scratch_bytes"):
        hip_ops.topn_links(model, indptr, indices, qd, 10, lds_slots=0,
                           scratch_bytes=64)
    # the binding checks what it is handed, too
    ext = hip_ops.ensure_loaded()
    dev = qd.device
    sel = torch.arange(2, device=dev, dtype=torch.int32)
    top_id = torch.full((len(q), 10), -1, device=dev, dtype=torch.int32)
    top_score = torch.zeros((len(q), 10), device=dev)
    n_cand = torch.zeros(len(q), device=dev, dtype=torch.int32)
    e64 = torch.empty(0, device=dev, dtype=torch.int64)
    e32 = torch.empty(0, device=dev, dtype=torch.int32)
    ef = torch.empty(0, device=dev)
    arrays = (model.row_ptr, model.row_col, model.row_val, model.col_ptr,
              model.col_row, model.col_val, indptr, indices, qd)
    for tab, match in (([64, 96], "powers of two"), ([32, 64], "powers of"),
                       ([64, 1024], "exceeds lds_slots")):
        with pytest.raises(RuntimeError, match=match):
            ext.topn_links(
                *arrays, sel,
                torch.tensor(tab, device=dev, dtype=torch.int32), e64, e32,
                ef, 10, 512, 256, top_id, top_score, n_cand)
    with pytest.raises(RuntimeError, match="outside the scratch"):
        ext.topn_links(
            *arrays, sel,
            torch.tensor([512, 512], device=dev, dtype=torch.int32),
            torch.tensor([0, 512], device=dev), torch.empty(
                1000, device=dev, dtype=torch.int32),
            torch.empty(1000, device=dev), 10, 0, 256, top_id, top_score,
            n_cand)
    assert (top_id == -1).all() and (n_cand == 0).all()  # nothing launched


def test_no_queries(edge):
    from bigclam.ops import hip as hip_ops

    F, graph, q, _ = edge
    model, indptr, indices, qd = _device_args(F, graph, q)
    top_id, top_score, n_cand, info = hip_ops.topn_links(
        model, indptr, indices, qd[:0], 10)
    assert top_id.is_cuda and top_id.shape == (0, 10)
    assert top_id.dtype == torch.int32 and top_score.shape == (0, 10)
    assert top_score.dtype == torch.float32
    assert n_cand.shape == (0,) and n_cand.dtype == torch.int32
    assert info["n_lds"] == info["n_global"] == 0
    res = recommend(graph, model, queries=[], n=10, device="cuda")
    assert res["top_id"].shape == (0, 10) and res["exact_frac"] == 0.0


def test_fit_recommend_device_equals_cpu():
    g, _ = planted_overlap(60, 30, 5, 0.5, 0, seed=42)
    split = split_edges(g, 0.2, 0)
    cfg = BigClamConfig(k=60, device="cuda", seed=3, max_sweeps=40)
    tr = Trainer(split.train, cfg, rank=0, world_size=1,
                 device=torch.device("cuda"))
    assert tr.state.use_hip
    tr.fit(init="seed")
    res = recommend_trainer(tr, n=10)
    assert res["n_lds"] + res["n_global"] == g.num_nodes
    ref = recommend(split.train, gather_sparse_model(tr).to("cpu"), n=10,
                    device="cpu")
    for key in NAMES + ("prob", "queries"):
        assert res[key].dtype == ref[key].dtype, key
        assert res[key].tobytes() == ref[key].tobytes(), key
    for key in ("work", "exact_frac", "columns_dropped", "n"):
        assert res[key] == ref[key], key
    assert (res["n_cand"] > 0).any()
    hr = heldout_ranking(res, split)
    assert hr == heldout_ranking(ref, split)
    assert hr["heldout_rank_queries"] > 0
    print("recall@10", hr["heldout_recall_at_n"], "hit rate",
          hr["heldout_hit_rate"], "exact_frac", res["exact_frac"])
    assert 0.0 < hr["heldout_recall_at_n"] <= 1.0
    # the global-table path end to end
    forced = recommend_trainer(tr, n=10, lds_slots=64)
    assert forced["n_global"] > 0
    for key in NAMES:
        assert forced[key].tobytes() == ref[key].tobytes(), key
