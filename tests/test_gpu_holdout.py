"""K9 (k9_pair_dot_t) on the GPU against the fp64 dot of the stored values,
the wrapper's validation, and the held-out metrics end to end (device path
against the CPU path fed the same F).

Tolerance (derived, not tuned).  Every term of a dot is non-negative and a
bf16 x bf16 product is exact in fp32, so the computed value differs from the
exact one by at most ``2 * d * 2**-24 * x``, d = the longest fp32 addition
chain of the kernel's documented layout: the elements one lane folds
(vectors per lane x elements per vector) plus the 6 butterfly levels.  The
factor 2 covers second-order terms and the final rounding.  ``atol`` is 0.
"""
import numpy as np
import pytest
import torch

from bigclam.config import BigClamConfig
from bigclam.engine.holdout import (
    heldout_metrics,
    metrics_from_scores,
    score_pairs,
)
from bigclam.engine.trainer import Trainer
from bigclam.io import planted_overlap
from bigclam.io.holdout import split_edges
from bigclam.ops import reference as ref_ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
N_OWN, N_EXTRA = 9, 6
# row roles (the same in both buffers): a row at max_f, two rows with
# disjoint supports; every other row is dense random in [0, 1]
ROW_MAX, ROW_EVEN, ROW_ODD = 3, 4, 5
XR_MAX, XR_EVEN, XR_ODD = 1, 2, 3


def chain(kp, dtype):
    """d: per-lane elements + 6 butterfly levels."""
    epv = 8 if dtype == torch.bfloat16 else 4
    nvec = kp // epv
    return -(-nvec // 64) * epv + 6


def bound(x64, kp, dtype):
    return 2.0 * chain(kp, dtype) * 2.0 ** -24 * x64


def _rows(n, kp, dtype, r_max, r_even, r_odd, gen):
    F = torch.rand(n, kp, generator=gen)
    F[r_max] = 1000.0  # max_f
    cols = torch.arange(kp)
    F[r_even, cols % 2 == 1] = 0.0
    F[r_odd, cols % 2 == 0] = 0.0
    return F.to(dtype)


def _pairs(p, n_extra, gen):
    """Fixed specials first, random pairs after; with n_extra == 0 the
    specials stay inside F_own."""
    if n_extra:
        special = [
            (ROW_MAX, N_OWN + XR_MAX),  # max_f x max_f across the buffers
            (ROW_EVEN, ROW_ODD),  # disjoint supports: exactly 0
            (N_OWN + XR_EVEN, ROW_ODD),  # ... u in extra, v in own
            (2, 2),  # pu == pv
            (N_OWN - 1, N_OWN),  # the two rows at the buffer boundary
        ]
    else:
        special = [(ROW_MAX, ROW_MAX), (ROW_EVEN, ROW_ODD),
                   (ROW_ODD, ROW_EVEN), (2, 2), (N_OWN - 1, 0)]
    n = N_OWN + n_extra
    rnd = torch.randint(0, n, (max(p - 5, 0), 2), generator=gen).tolist()
    pairs = (special + [tuple(r) for r in rnd])[:p]
    t = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)
    return t[:, 0].contiguous(), t[:, 1].contiguous()


@pytest.mark.parametrize(
    "dtype,kp",
    [(torch.float32, k) for k in (4, 256, 260, 8200)]
    + [(torch.bfloat16, k) for k in (8, 256, 264, 512, 520, 8200)],
    ids=lambda v: str(v).replace("torch.", ""),
)
def test_k9_against_fp64(dtype, kp):
    from bigclam.ops import hip as hip_ops

    gen = torch.Generator().manual_seed(kp)
    own = _rows(N_OWN, kp, dtype, ROW_MAX, ROW_EVEN, ROW_ODD, gen)
    ext = _rows(N_EXTRA, kp, dtype, XR_MAX, XR_EVEN, XR_ODD, gen)
    own_d, ext_d = own.to(DEV), ext.to(DEV)
    for n_extra in (N_EXTRA, 0):
        e, e_d = ext[:n_extra], ext_d[:n_extra]
        all64 = torch.cat([own, e]).double()
        for p in (0, 1, 5, 1031):
            pu, pv = _pairs(p, n_extra, gen)
            x = hip_ops.pair_dot(own_d, e_d, pu.to(DEV), pv.to(DEV))
            assert x.dtype == torch.float32 and x.shape == (p,)
            want = (all64[pu.long()] * all64[pv.long()]).sum(-1).numpy()
            got = x.cpu().double().numpy()
            err = np.abs(got - want)
            tol = bound(want, kp, dtype)
            worst = float((err / np.maximum(tol, 1e-300)).max()) if p else 0.0
            print(f"kp={kp} n_extra={n_extra} P={p} d={chain(kp, dtype)} "
                  f"max err/bound={worst:.3f}")
            assert (err <= tol).all(), (kp, n_extra, p, worst)
            if p >= 5:
                # disjoint supports: exactly 0 (tol is 0 there as well)
                assert want[1] == 0.0 and want[2] == 0.0
                assert got[1] == 0.0 and got[2] == 0.0
                assert want[0] == kp * 1e6 and got[3] > 0
            if p == 1031:
                # the same pairs in one launch and split over two launches,
                # and a second run: bitwise equal
                a = hip_ops.pair_dot(own_d, e_d, pu[:400].to(DEV),
                                     pv[:400].to(DEV))
                b = hip_ops.pair_dot(own_d, e_d, pu[400:].to(DEV),
                                     pv[400:].to(DEV))
                again = hip_ops.pair_dot(own_d, e_d, pu.to(DEV), pv.to(DEV))
                assert torch.equal(torch.cat([a, b]), x)
                assert torch.equal(again, x)
                # and the torch formulation agrees within both bounds
                ref = ref_ops.pair_dot(own_d, e_d, pu.to(DEV), pv.to(DEV))
                ref_tol = 2.0 * (kp + 6) * 2.0 ** -24 * want
                assert (np.abs(ref.cpu().double().numpy() - want)
                        <= ref_tol).all()


def test_k9_rows_beyond_2_31_elements():
    """Row offsets past 2^31 elements (a 4 GiB bf16 shard): the row
    address arithmetic is 64-bit."""
    from bigclam.ops import hip as hip_ops

    kp = 8
    n_own = (1 << 28) + 8  # n_own * kp = 2^31 + 64 elements
    own = torch.zeros(n_own, kp, device=DEV, dtype=torch.bfloat16)
    ext = torch.zeros(2, kp, device=DEV, dtype=torch.bfloat16)
    vals = torch.arange(1, kp + 1, dtype=torch.float32)
    own[n_own - 1] = vals.to(DEV)
    own[n_own - 3] = (2 * vals).to(DEV)
    own[5] = 1.0
    ext[1] = 3.0
    pu = torch.tensor([n_own - 3, 5, n_own - 1, 5], dtype=torch.int32)
    pv = torch.tensor([n_own - 1, n_own - 1, n_own + 1, n_own - 2],
                      dtype=torch.int32)
    x = hip_ops.pair_dot(own, ext, pu.to(DEV), pv.to(DEV)).cpu()
    s1, s2 = float(vals.sum()), float((vals * vals).sum())
    assert x.tolist() == [2 * s2, s1, 3 * s1, 0.0]


def test_wrapper_validation():
    from bigclam.ops import hip as hip_ops

    own = torch.rand(7, 16, device=DEV)
    ext = torch.rand(3, 16, device=DEV)
    pu = torch.tensor([0, 9, 3], dtype=torch.int32, device=DEV)
    pv = torch.tensor([1, 2, 8], dtype=torch.int32, device=DEV)
    assert hip_ops.pair_dot(own, ext, pu, pv).shape == (3,)
    bad = [
        ("dtype", (own.half(), ext.half(), pu, pv)),
        ("dtype", (own.double(), ext.double(), pu, pv)),
        ("dtype", (own, ext.bfloat16(), pu, pv)),
        ("dtype", (own, ext, pu.long(), pv)),
        ("dtype", (own, ext, pu, pv.long())),
        ("contiguous", (own[:, ::2], ext[:, ::2], pu, pv)),
        ("contiguous", (own, torch.rand(3, 32, device=DEV)[:, ::2], pu, pv)),
        ("contiguous", (own, ext, torch.stack([pu, pu], 1)[:, 0], pv)),
        ("GPU", (own.cpu(), ext, pu, pv)),
        ("GPU", (own, ext.cpu(), pu, pv)),
        ("GPU", (own, ext, pu.cpu(), pv)),
        ("GPU", (own, ext, pu, pv.cpu())),
        ("kp", (own, torch.rand(3, 20, device=DEV), pu, pv)),
        ("kp", (own[:, :6].contiguous(), ext[:, :6].contiguous(), pu, pv)),
        ("same length", (own, ext, pu, pv[:2])),
        ("range", (own, ext, pu, torch.full_like(pv, 10))),
        ("range", (own, ext, torch.full_like(pu, -1), pv)),
        ("range", (own, ext[:0], pu, pv)),  # 9 and 8 need the extra rows
    ]
    for what, args in bad:
        with pytest.raises(RuntimeError, match=what):
            hip_ops.pair_dot(*args)
    # P == 0 launches nothing, whatever the buffers hold
    assert hip_ops.pair_dot(own, ext[:0], pu[:0], pv[:0]).shape == (0,)


def test_select_k_holdout_on_device():
    """The held-out select-k loop end to end on the GPU (K9 scoring inside
    every grid point): same graph, grid and seeds as the CPU test."""
    from bigclam.engine.model_select import select_k

    g, _ = planted_overlap(8, 24, 6, 0.5, 0, seed=11)
    cfg = BigClamConfig(device="cuda", seed=3, k_min=2, k_max=8, k_div=1)
    out = select_k(g, cfg, init="random", holdout=0.2, holdout_seed=0)
    hist = {h["k"]: h for h in out["history"]}
    print({k: (h["heldout_llh"], h["heldout_auc"]) for k, h in hist.items()})
    assert out["grid"] == [2, 8] and set(hist) == {2, 8}
    assert out["k"] == 8
    assert hist[8]["heldout_auc"] > 0.85
    assert hist[8]["heldout_auc"] > hist[2]["heldout_auc"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_heldout_metrics_device_against_cpu_path(dtype):
    """Fit on the GPU, then score the same F on both paths.

    x: per pair within ``bound`` (both paths err by at most d ulps-of-x
    from the exact dot: 4-8 fp32 roundings at k = 8 against d = 10 / 14).
    LLH: within twice the first-order propagation
    ``sum_pos |dx| p/(1-p) + neg_weight/Q * sum_neg |dx|`` of those bounds.
    AUC: a (pos, neg) pair can change its order only if its CPU scores are
    closer than the two per-pair bounds together; each such pair (both
    exactly 0 excluded — they stay tied) moves the AUC by at most
    1/(P*Q)."""
    g, _ = planted_overlap(8, 24, 6, 0.5, 0, seed=11)
    sp = split_edges(g, 0.2, 0)
    cfg = BigClamConfig(k=8, device="cuda", seed=3, dtype=dtype,
                        max_sweeps=40)
    tr = Trainer(sp.train, cfg, rank=0, world_size=1, device=DEV)
    assert tr.state.use_hip
    tr.fit(init="random")
    n_pos = len(sp.pos)
    pairs = np.concatenate([sp.pos, sp.neg])
    x_gpu = score_pairs(tr, pairs)
    hm = heldout_metrics(tr, sp)

    F = tr.gather_F()  # CPU fp32 [N, 8]: the stored values
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    pu = torch.from_numpy(pairs[:, 0].copy())
    pv = torch.from_numpy(pairs[:, 1].copy())
    x_cpu = ref_ops.pair_dot(F, F[:0], pu, pv).numpy()
    ref = metrics_from_scores(x_cpu[:n_pos], x_cpu[n_pos:], sp.neg_weight,
                              sp.requested, cfg.min_p, cfg.max_p)

    x64 = x_cpu.astype(np.float64)
    b = bound(x64, tr.state.kp, tdt)
    dx = np.abs(x_gpu.astype(np.float64) - x64)
    print(f"max |dx|/bound = {float((dx / np.maximum(b, 1e-300)).max()):.3f}")
    assert (dx <= b).all()
    assert ((x_gpu == 0) == (x_cpu == 0)).all()

    p = np.clip(np.exp(-x64[:n_pos]), cfg.min_p, cfg.max_p)
    llh_tol = 2.0 * ((b[:n_pos] * p / (1.0 - p)).sum()
                     + sp.neg_weight / (len(pairs) - n_pos) * b[n_pos:].sum())
    print(f"heldout_llh gpu {hm['heldout_llh']!r} cpu {ref['heldout_llh']!r}"
          f" tol {llh_tol:.3e}")
    assert abs(hm["heldout_llh"] - ref["heldout_llh"]) <= llh_tol

    xp, xn = x64[:n_pos], x64[n_pos:]
    close = np.abs(xp[:, None] - xn[None, :]) <= (
        b[:n_pos][:, None] + b[n_pos:][None, :])
    close &= ~((xp[:, None] == 0) & (xn[None, :] == 0))
    auc_tol = close.sum() / (len(xp) * len(xn))
    print(f"heldout_auc gpu {hm['heldout_auc']!r} cpu {ref['heldout_auc']!r}"
          f" tol {auc_tol:.3e}")
    assert abs(hm["heldout_auc"] - ref["heldout_auc"]) <= auc_tol
    for key in ("heldout_pos", "heldout_neg", "heldout_requested"):
        assert hm[key] == ref[key]
    assert hm["heldout_auc"] > 0.5  # a fitted model beats chance
