"""Fixtures of the numerics contract (docs/kernels.md): degree-ladder
graphs, F regimes and the fp32 torch stand-in implementation.

Imported by both the CPU tests (tests/test_oracle.py: fixture conditions,
constant measurement, sharpness) and the GPU tests
(tests/test_gpu_contract.py).  Everything here is deterministic.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

from bigclam.config import BigClamConfig
from bigclam.io.edgelist import Graph
from bigclam.ops import reference as ref_ops

# centre degrees: 0 (isolated centre), the 4-wave edge split (1..5), the
# 16-row MFMA tile (15/16/17, 31/32/33), the 64-row KF_TG tile group
# (63/64/65), 127/128/129; hub adds kw_grad_t's 256-edge tile, k2_ls_tiled's
# 512-edge tile and one off-grid hub.
SMALL_DEGREES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127,
                 128, 129)
HUB_DEGREES = SMALL_DEGREES + (255, 256, 257, 511, 512, 513, 600)

# C1 K matrix: (dtype, K) -> NSLOT class is decided by the padded width kp
FP32_KS = (1, 4, 17, 65, 1021, 1025, 2049, 4097, 8189, 8193, 10001)
BF16_KS = (1, 9, 33, 250, 2041, 2049, 4097, 5000, 8185, 8193, 16377, 16385)
# sparse regime: one K per NSLOT class (fp32 1/2/4/8 + the unfused regime,
# bf16 1/2/4/8 + the LDS-only NSLOT=0 variant)
FP32_SPARSE_KS = (1021, 1025, 2049, 8189, 10001)
BF16_SPARSE_KS = (2041, 2049, 5000, 8193, 16385)
# C2 degree matrix
C2_KS = (("fp32", 68), ("fp32", 260), ("bf16", 264))
C2_REGIMES = ("dense", "saturated", "capped", "short")


def padded_k(k: int, dtype: str) -> int:
    return (k + 7) & ~7 if dtype == "bf16" else (k + 3) & ~3


@functools.lru_cache(maxsize=None)
def ladder_graph(kind: str):
    """Degree-ladder graph.  For each target degree d a centre node joins
    the first d nodes of a shared leaf pool (centres never join each other:
    centre degrees are exact, leaf degrees vary), plus two isolated nodes;
    ids are permuted so the degree-descending order is not the identity.
    Built directly: build_graph would drop the isolated ids.

    Returns (Graph, label [N] int64): label = the centre's target degree,
    -1 for leaves, -2 for the two isolated nodes.
    """
    degs = SMALL_DEGREES if kind == "small" else HUB_DEGREES
    pool = max(degs)
    n = pool + len(degs) + 2
    rng = np.random.default_rng(1234 + len(degs))
    perm = rng.permutation(n)
    label = np.full(n, -1, dtype=np.int64)
    src, dst = [], []
    for i, d in enumerate(degs):
        c = perm[pool + i]
        label[c] = d
        leaves = perm[:d]
        src += [np.full(d, c), leaves]
        dst += [leaves, np.full(d, c)]
    label[perm[pool + len(degs):]] = -2
    src = np.concatenate(src).astype(np.int64)
    dst = np.concatenate(dst).astype(np.int64)
    o = np.lexsort((dst, src))  # sorted rows (canonical CSR)
    src, dst = src[o], dst[o]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, src + 1, 1)
    indptr = np.cumsum(indptr)
    g = Graph(indptr=indptr, indices=dst.astype(np.int32),
              raw_ids=np.arange(n, dtype=np.int64))
    return g, label


def degree_class(label: np.ndarray, graph: Graph, nodes) -> list:
    """Readable degree classes of ``nodes`` for assertion messages."""
    return _classes(graph.indptr, label, nodes)


# --------------------------------------------------------------- F regimes
def _row_scales(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=n))


def regime_cfg(regime: str, k: int, dtype: str, device: str = "cpu"):
    kw = {}
    if regime == "capped":
        kw = dict(max_f=0.5)  # min_f stays 0: non-zero would write pads
    if regime == "short":
        kw = dict(ls_steps=7, beta=0.5, alpha=0.1)
    return BigClamConfig(k=k, device=device, dtype=dtype, **kw)


def make_F(graph: Graph, k: int, regime: str, seed: int = 0) -> np.ndarray:
    """fp32 [N, k] initial F for a regime.  Per-row log-uniform scales in
    every regime so gradient magnitudes — and the Armijo picks — vary.

    Every edge joins a centre and a leaf, so x = fu.fv ~ 0.39 r_c r_l with
    separate scale ranges (centres, leaves) per regime: the leaf range is
    wide because a node's accepted step is roughly its own scale over the
    mean scale (the -sumF term dominates the gradient at these sizes)."""
    n = graph.num_nodes
    rng = np.random.default_rng(1000 * seed + 17 * k + len(regime))
    u = rng.uniform(0.25, 1.0, size=(n, k))
    rk = 1.0 / np.sqrt(k)
    centres = _centres(graph)
    (clo, chi), (llo, lhi) = _SCALES[regime]
    r = _row_scales(rng, n, llo, lhi)
    r[centres] = _row_scales(rng, len(centres), clo, chi)
    F = u * r[:, None] * rk
    if regime in ("dense", "short", "saturated"):
        pass  # dense/short: x between the p-clamps; saturated: x >= 10
    elif regime == "capped":
        # max_f = 0.5 with entries at exactly 0 and exactly 0.5
        F = np.minimum(F, 0.5)
        sel = rng.random((n, k))
        F[sel < 0.10] = 0.0
        F[(sel > 0.95) & (r[:, None] >= 1.0)] = 0.5
    elif regime == "sparse":
        # ~90% exact zeros; the kept entries are scaled up so overlapping
        # supports still give x of order 1
        keep = rng.random((n, k)) < 0.10
        F = np.where(keep, F * 10.0, 0.0)
        if k >= 2:
            # disjoint supports on adjacent pairs: every centre keeps only
            # odd columns, every third leaf only even ones -> x exactly 0
            # on those edges (max_p active)
            F[np.ix_(centres, np.arange(0, k, 2))] = 0.0
            leaves = np.setdiff1d(np.arange(n), centres)[::3]
            F[np.ix_(leaves, np.arange(1, k, 2))] = 0.0
        zero_rows = rng.choice(n, size=4, replace=False)
        F[zero_rows] = 0.0  # a few all-zero rows
    else:
        raise ValueError(regime)
    return F.astype(np.float32)


# per-row scale ranges ((centres), (leaves and isolated)), tuned on the CPU
# until the oracle satisfies the fixture conditions
# (tests/test_oracle.py::test_fixture_conditions)
_SCALES = {
    "dense": ((0.5, 2.5), (0.01, 3.0)),
    "short": ((0.3, 2.5), (0.3, 2.5)),
    "saturated": ((40.0, 120.0), (0.2, 30.0)),
    "capped": ((0.5, 4.0), (0.02, 4.0)),
    "sparse": ((0.5, 2.5), (0.3, 3.0)),
}


# seeds tuned like the scales: `capped` at K=68 needs a draw on which the
# upper F-clamp decides at least one pick (so a kernel without it fails)
_SEEDS = {("capped", 68): 2}


def _centres(graph: Graph) -> np.ndarray:
    for kind in ("small", "hub"):
        g, label = ladder_graph(kind)
        if g is graph:
            return np.flatnonzero(label >= 0)
    raise ValueError("not a ladder graph")


@dataclass
class Case:
    kind: str
    regime: str
    dtype: str
    k: int
    graph: Graph
    label: np.ndarray
    cfg: BigClamConfig
    F0: np.ndarray  # fp32 [N, k] before storage rounding

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.regime}-{self.dtype}-k{self.k}"

    @property
    def kp(self) -> int:
        return padded_k(self.k, self.dtype)

    def stored_F(self) -> torch.Tensor:
        """[N, kp] in the storage dtype, pad columns zero (what
        ShardState.set_local_F installs)."""
        sd = torch.bfloat16 if self.dtype == "bf16" else torch.float32
        F = torch.zeros(self.graph.num_nodes, self.kp, dtype=sd)
        F[:, : self.k] = torch.from_numpy(self.F0).to(sd)
        return F


@functools.lru_cache(maxsize=None)
def make_case(kind: str, regime: str, dtype: str, k: int) -> Case:
    g, label = ladder_graph(kind)
    return Case(kind, regime, dtype, k, g, label,
                regime_cfg(regime, k, dtype),
                make_F(g, k, regime, seed=_SEEDS.get((regime, k), 0)))


def c1_cases():
    out = [("small", "dense", "fp32", k) for k in FP32_KS]
    out += [("small", "dense", "bf16", k) for k in BF16_KS]
    out += [("small", "sparse", "fp32", k) for k in FP32_SPARSE_KS]
    out += [("small", "sparse", "bf16", k) for k in BF16_SPARSE_KS]
    return out


def c2_cases():
    return [("hub", r, d, k) for d, k in C2_KS for r in C2_REGIMES]


def c4_cases():
    return [("hub", "dense", d, 37) for d in ("fp32", "bf16")]


def c5_cases():
    return [("hub", "sparse", d, 512) for d in ("fp32", "bf16")]


def all_cases():
    return c1_cases() + c2_cases() + c4_cases() + c5_cases()


def case_id(t) -> str:
    return "-".join(str(x) for x in t)


# ------------------------------------------- fp32 torch stand-in (CPU)
def csr_tensors(graph_or_shard):
    return (torch.from_numpy(np.asarray(graph_or_shard.indptr)),
            torch.from_numpy(np.asarray(graph_or_shard.indices)).int())


def ref_trials(F, indptr, indices, sumF, grad, cfg, n_local=None):
    """fp32 torch evaluation of ALL ladder rungs' trial values, the same
    formula as reference.linesearch without the accept masking.
    Returns fp64 [n_local, n_ladder]."""
    n_local = n_local if n_local is not None else len(indptr) - 1
    src = ref_ops._edge_src(indptr)
    Fl = F[:n_local].float()
    sf = sumF.float()
    Fv = F[indices.long()].float()
    lad = cfg.ladder()
    out = torch.empty(n_local, len(lad), dtype=torch.float64)
    for j, s_val in enumerate(lad):
        Fc = torch.clamp(Fl + s_val * grad, cfg.min_f, cfg.max_f)
        x = (Fc[src] * Fv).sum(-1)
        p = torch.clamp(torch.exp(-x), cfg.min_p, cfg.max_p)
        edge = torch.zeros(n_local, dtype=torch.float64)
        edge.index_add_(0, src, torch.log1p(-p).double() + x.double())
        sf_adj = sf.unsqueeze(0) - Fl + Fc
        node = (-(Fc * sf_adj).sum(-1) + (Fc * Fc).sum(-1)).double()
        out[:, j] = edge + node
    return out


def picks_from_trials(trials, llh, grad, cfg):
    """First-accept rung per node from trial values (-1 = no step), with
    the reference's fp64 Armijo threshold."""
    gg = (grad.double() ** 2).sum(-1)
    lad = torch.tensor(cfg.ladder(), dtype=torch.float64)
    ok = trials >= llh.unsqueeze(1) + cfg.alpha * lad.unsqueeze(0) * gg.unsqueeze(1)
    ok = ok.numpy()
    return np.where(ok.any(axis=1), ok.argmax(axis=1), -1)


def ref_run(case: Case):
    """The fp32 torch reference on a case: dict(F, sumF, grad, llh, best,
    trials), all torch CPU tensors."""
    F = case.stored_F()
    indptr, indices = csr_tensors(case.graph)
    sumF = F.float().sum(dim=0)
    grad, llh = ref_ops.edge_grad_llh(F, indptr, indices, sumF, case.cfg)
    best = ref_ops.linesearch(F, indptr, indices, sumF, grad, llh, case.cfg)
    trials = ref_trials(F, indptr, indices, sumF, grad, case.cfg)
    return dict(F=F, sumF=sumF, grad=grad, llh=llh, best=best, trials=trials,
                indptr=indptr, indices=indices)


# --------------------------------------------------- the comparison itself
def _classes(indptr, label, nodes):
    deg = np.diff(np.asarray(indptr))
    out = []
    for u in np.atleast_1d(nodes)[:12]:
        kind = {-1: "leaf", -2: "isolated"}.get(int(label[u]), "centre")
        out.append(f"{kind}(deg={int(deg[u])},node={int(u)})")
    return out


def assert_grad_llh(tag, o, indptr, label, k, grad=None, llh=None, rows=None):
    """grad within C_GRAD eps32 A of grad64 (pad columns exactly zero) and
    llh within C_LLH eps32 L of llh64, for ``rows`` (default: all)."""
    import oracle

    sel = (lambda idx: idx) if rows is None else (
        lambda idx: idx[np.isin(idx, rows)])
    if grad is not None:
        grad = np.asarray(grad)
        assert not grad[:, k:].any(), f"{tag}: pad columns of grad not zero"
        v = oracle.grad_violations(grad, o)
        bad = sel(np.unique(v[:, 0]))
        if len(bad):
            u = int(bad[0])
            ks = v[v[:, 0] == u][:4, 1]
            e = np.abs(grad[u, ks].astype(np.float64) - o["grad"][u, ks])
            raise AssertionError(
                f"{tag}: grad outside {oracle.C_GRAD:g}*eps32*A on "
                f"{len(bad)} nodes {_classes(indptr, label, bad)}; node {u} "
                f"cols {ks.tolist()} err/(eps32*A) = "
                f"{(e / (oracle.EPS32 * o['A'][u, ks])).tolist()}")
    if llh is not None:
        llh = np.asarray(llh, dtype=np.float64)
        bad = sel(oracle.llh_violations(llh, o))
        if len(bad):
            e = np.abs(llh[bad] - o["llh"][bad]) / (oracle.EPS32 * o["L"][bad])
            raise AssertionError(
                f"{tag}: llh outside {oracle.C_LLH:g}*eps32*L on "
                f"{_classes(indptr, label, bad)}; err/(eps32*L) = "
                f"{e[:12].tolist()}")


def assert_picks(tag, mo, indptr, label, cfg, dtype, best,
                 bf16_candidates=False, rows=None):
    """The acceptance rule of the contract for EVERY node (or ``rows``),
    plus the cap on the share of picks that differ from the exact pick.
    ``bf16_candidates`` may be a per-node bool array."""
    import oracle

    rung = oracle.steps_to_rungs(np.asarray(best), cfg)
    n = len(rung)
    flag = np.broadcast_to(np.asarray(bf16_candidates, dtype=bool), (n,))
    bad0, differ = oracle.pick_violations(rung, mo, bf16_candidates=False)
    bad1, _ = oracle.pick_violations(rung, mo, bf16_candidates=True)
    bad = np.union1d(bad0[~flag[bad0]], bad1[flag[bad1]])
    if rows is not None:
        bad = bad[np.isin(bad, rows)]
        differ = differ[np.isin(differ, rows)]
        n = len(rows)
    if len(bad):
        u = int(bad[0])
        T = oracle.C_MARGIN * oracle.EPS32 * mo["M"][u] + (
            oracle.BF16_CAND_EPS * mo["B"][u] if flag[u] else 0.0)
        raise AssertionError(
            f"{tag}: pick breaks the Armijo contract on {len(bad)} nodes "
            f"{_classes(indptr, label, bad)}; node {u}: picked rung "
            f"{int(rung[u])}, exact {int(mo['pick'][u])}, margins "
            f"{mo['m'][u].tolist()}, tolerances {T.tolist()}")
    assert oracle.pick_cap_ok(len(differ), n, dtype), (
        f"{tag}: {len(differ)} of {n} picks differ from the exact pick "
        f"{_classes(indptr, label, differ)}")


def bf16_rne(v):
    """Round-to-nearest-even of non-negative fp64 values to bf16 (8
    significant bits), returned as fp64, with the bf16 ulp at v and the
    distance of v to the nearest rounding midpoint."""
    v = np.asarray(v, dtype=np.float64)
    _, ex = np.frexp(np.where(v > 0, v, 1.0))
    ulp = np.ldexp(1.0, ex - 8)
    q = v / ulp
    r = np.rint(q) * ulp  # np.rint: ties to even
    mid = np.abs(q - np.floor(q) - 0.5) * ulp
    return np.where(v > 0, r, 0.0), ulp, mid


def assert_commit(tag, F_before, F_after, grad, steps, cfg):
    """K3 contract.  Rows with step 0 bitwise unchanged; fp32 within 1 ulp
    of the fp64 commit rounded to fp32; bf16 equal to the RNE rounding of
    the fp64 commit, 1 bf16 ulp allowed where the fp64 value lies within 2
    fp32 ulps of a bf16 rounding midpoint."""
    import oracle

    steps_np = steps.float().cpu().numpy()
    idle = torch.from_numpy(steps_np <= 0)
    a = F_after.cpu()
    b = F_before.cpu()
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(a[idle].view(it), b[idle].view(it)), (
        f"{tag}: rows with step 0 changed")
    want = oracle.vec_commit(b.double().numpy(), grad.double().cpu().numpy(),
                             steps_np, cfg)
    got = a.double().numpy()
    if a.dtype == torch.float32:
        w32 = want.astype(np.float32)
        ulp = np.spacing(np.abs(w32)).astype(np.float64)
        bad = np.abs(got - w32.astype(np.float64)) > ulp
    else:
        r, ulp, mid = bf16_rne(want)
        near = mid <= 2.0 * ulp * 2.0 ** -16  # 2 fp32 ulps
        bad = np.where(near, np.abs(got - r) > ulp, got != r)
    assert not bad.any(), (
        f"{tag}: {int(bad.sum())} committed entries off; first at "
        f"{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r} want "
        f"{want[bad][0]!r}")
    return want


def assert_colsum(tag, sums, F_after):
    """fp32 column sums vs the fp64 column sum of the POST-rounding values:
    |err| <= C_GRAD eps32 sum|F| (the A-style bound)."""
    import oracle

    F = F_after.double().cpu().numpy()
    ref = F.sum(axis=0)
    tol = oracle.C_GRAD * oracle.EPS32 * np.abs(F).sum(axis=0)
    err = np.abs(np.asarray(sums, dtype=np.float64) - ref)
    assert (err <= tol).all(), (
        f"{tag}: column sum off at {np.flatnonzero(err > tol)[:8].tolist()}")


class Judge:
    """Oracle of one (F, sumF, CSR) with margins cached per distinct
    (grad, llh) — paths sharing phase A bitwise share one margin pass."""

    def __init__(self, F, sumF, indptr, indices, cfg, label, k, dtype,
                 n_local=None):
        import oracle

        self.F64 = F.double().cpu().numpy()
        self.s64 = sumF.double().cpu().numpy()
        self.indptr, self.indices = np.asarray(indptr), np.asarray(indices)
        self.cfg, self.label, self.k, self.dtype = cfg, label, k, dtype
        self.n_local = n_local
        self.o = oracle.vec_grad_llh(self.F64, self.s64, self.indptr,
                                     self.indices, cfg, n_local=n_local)
        self._mo = {}

    def margins(self, grad, llh):
        import oracle

        key = (hash(grad.tobytes()), hash(llh.tobytes()))
        if key not in self._mo:
            self._mo[key] = oracle.vec_margins(
                self.F64, self.s64, self.indptr, self.indices, self.cfg,
                grad, llh, n_local=self.n_local)
        return self._mo[key]

    def check(self, tag, grad, llh, best=None, bf16_candidates=False,
              rows=None, check_grad=True):
        """Returns the figures it printed: (largest normalised grad error,
        largest normalised llh error, picks differing from the exact pick
        or None)."""
        import oracle

        if torch.cuda.is_available():
            torch.cuda.synchronize()
        g = grad.cpu().numpy()
        l = llh.cpu().numpy()
        # the figures first (pytest -s shows them), then the assertions
        o = self.o
        sel = slice(None) if rows is None else rows
        with np.errstate(invalid="ignore", divide="ignore"):
            eg = np.nanmax((np.abs(g - o["grad"]) / (oracle.EPS32 * o["A"]))[sel]
                           ) if check_grad else float("nan")
            el = np.nanmax((np.abs(l - o["llh"]) / (oracle.EPS32 * o["L"]))[sel])
        msg = f"{tag}: grad {eg:.1f}/{oracle.C_GRAD:g} llh {el:.1f}/{oracle.C_LLH:g}"
        nd = None
        if best is not None:
            mo = self.margins(g, l)
            rung = oracle.steps_to_rungs(best.cpu().numpy(), self.cfg)
            nd = int((rung != mo['pick'])[sel].sum())
            msg += f" picks differing {nd}"
        print(msg)
        assert_grad_llh(tag, self.o, self.indptr, self.label, self.k,
                        g if check_grad else None, l, rows=rows)
        if best is not None:
            assert_picks(tag, self.margins(g, l), self.indptr, self.label,
                         self.cfg, self.dtype, best.cpu().numpy(),
                         bf16_candidates=bf16_candidates, rows=rows)
        return float(eg), float(el), nd


def rescan(Fh, r):
    """(columns, values) of row r's non-zeros, ascending — what KAF emits."""
    ks = np.flatnonzero(Fh[r])
    return ks, Fh[r, ks]


def assert_lists(tag, Fh, rows, scount, sidx, sval, cap):
    """Counts and lists of ``rows`` equal a numpy rescan of F (ascending
    columns); an over-cap row has its count only.  ``rows`` index the
    buffer the pools belong to: owned rows and, past n_local, halo rows."""
    for r in rows:
        ks, vs = rescan(Fh, r)
        assert scount[r] == len(ks), f"{tag}: row {r} count"
        if len(ks) > cap:
            continue
        sl = slice(r * cap, r * cap + len(ks))
        np.testing.assert_array_equal(sidx[sl], ks, err_msg=f"{tag}: row {r}")
        np.testing.assert_array_equal(sval[sl], vs, err_msg=f"{tag}: row {r}")


# ===========================================================================
# K5 / K6 / K7 fixtures (docs/kernels.md, "K5 / K6 / K7 contract").  The
# kernels that bracket the sweep produce integers, exact 0/1 values or one
# IEEE division of exact integers, so everything built here is compared
# with exact equality (tests/test_init_extract_oracle.py on the CPU,
# tests/test_gpu_init_extract.py on the device).

# ------------------------------------------------------------------ K7 rows
K7_BLOCK = 256  # threads per row; each owns chunk = ceil(k_true/256) columns
# membership_threshold(149, 1200) = 0.33944688306...: its fp32 rounding lies
# BELOW it, so an entry equal to float32(delta) is a member under the fp32
# rule and is not under an fp64 comparison.
K7_DELTA = float(np.sqrt(-np.log1p(-2.0 * 1200 / (149 * 148))))
assert float(np.float32(K7_DELTA)) < K7_DELTA
# chunk: 1 (<= 256), 2 (257..512), 3 (513), 20 (5000, 5001), 98 (25000)
K7_WIDTHS = (1, 2, 255, 256, 257, 511, 512, 513, 5000, 5001, 25000)
K7_WIDE_LD = (257, 5000)  # also run with ldF = width + 24


def k7_cases():
    """(k_true, kp, dtype) of every K7 fixture.  The wide-ld cases add 24
    to k_true (fp32; 281 is an odd row stride) or to the padded width
    (bf16: a bf16 row stride must be even, K7 reads 32-bit words)."""
    out = []
    for dtype in ("fp32", "bf16"):
        out += [(k, padded_k(k, dtype), dtype) for k in K7_WIDTHS]
        out += [((k, k + 24, dtype) if dtype == "fp32"
                 else (k, padded_k(k, dtype) + 24, dtype)) for k in K7_WIDE_LD]
    return out


def k7_id(t) -> str:
    return f"k{t[0]}-ld{t[1]}-{t[2]}"


def k7_chunk(k_true: int) -> int:
    return -(-k_true // K7_BLOCK)


def _f32_bits(x) -> int:
    return int(np.array(x, dtype=np.float32).view(np.uint32))


def _from_bits(b: int) -> float:
    return float(np.array(b, dtype=np.uint32).view(np.float32))


def bf16_ceil(x: float) -> float:
    """Smallest bf16 value >= the positive fp32 value x."""
    b = _f32_bits(x)
    lo = b & 0xFFFF0000
    return _from_bits(lo if lo == b else lo + 0x10000)


def bf16_below(x: float) -> float:
    """Largest bf16 value < the positive fp32 value x."""
    b = _f32_bits(x)
    lo = b & 0xFFFF0000
    return _from_bits(lo - 0x10000 if lo == b else lo)


def k7_values(dtype: str, delta: float = K7_DELTA) -> dict:
    """The special values of the K7 rows, each representable in ``dtype``:
    ``at`` the smallest value that is a member, ``below`` the largest that
    is not, ``hi`` about 2t, ``lo`` > ``lo2`` well below t, ``tiny`` the
    smallest positive normal."""
    t = float(np.float32(delta))
    if dtype == "bf16":
        v = dict(at=bf16_ceil(t), below=bf16_below(t),
                 hi=bf16_ceil(float(np.float32(2 * t))))
    else:
        v = dict(at=t, below=float(np.nextafter(np.float32(t), np.float32(0))),
                 hi=float(np.float32(2 * t)))
    v.update(t=t, lo=0.125, lo2=0.0625, tiny=2.0 ** -126)
    assert v["tiny"] < v["lo2"] < v["lo"] < v["below"] < t <= v["at"] < v["hi"]
    return v


@functools.lru_cache(maxsize=None)
def _k7_build(k_true: int, kp: int, dtype: str, delta: float):
    v = k7_values(dtype, delta)
    at, below, hi, lo, lo2 = v["at"], v["below"], v["hi"], v["lo"], v["lo2"]
    chunk = k7_chunk(k_true)
    last = k_true - 1
    nthr = -(-k_true // chunk)  # threads that own at least one column
    tm = (nthr - 1) // 2  # a mid-row thread with a right neighbour
    m0 = tm * chunk  # first / last column of its chunk, and a middle one
    m1 = min(m0 + chunk, k_true) - 1
    mm = min(m0 + chunk // 2, last)
    firsts = np.arange(0, k_true, chunk)
    lasts = np.minimum(firsts + chunk, k_true) - 1
    rows, names = [], []

    def add(name, base, **cols):
        r = np.full(k_true, base, dtype=np.float64)
        for val, idx in cols.values():
            r[idx] = val
        rows.append(r)
        names.append(name)

    # plain membership
    add("zero", 0.0)
    add("member-col0", 0.0, a=(hi, 0))
    add("member-last", 0.0, a=(hi, last))
    add("member-chunk-first", 0.0, a=(hi, m0))
    add("member-chunk-last", 0.0, a=(hi, m1))
    # firsts sit exactly on the threshold, lasts well above it (chunk 1:
    # first == last, so odd columns take the high value)
    add("member-every-chunk-end", 0.0, a=(at, firsts),
        b=(hi, lasts if chunk > 1 else np.arange(1, k_true, 2)))
    add("member-all", at)
    # threshold
    add("exact-t", below, a=(at, mm))
    add("just-below-t", lo, a=(below, mm))
    # fallback: nothing reaches t
    add("fallback-col0", lo2, a=(lo, 0))
    add("fallback-last", lo2, a=(lo, last))
    add("fallback-mid-chunk", lo2, a=(lo, mm))
    add("fallback-tie-in-chunk", lo2, a=(lo, [m0, m1]))
    add("fallback-tie-across-threads", lo2, a=(lo, [m1, min(m1 + 1, last)]))
    e = mm & ~1
    add("fallback-tie-bf16-word", lo2, a=(lo, [e, min(e + 1, last)]))
    add("fallback-all-tied", lo)
    add("fallback-min-normal", 0.0, a=(v["tiny"], mm))
    if kp > k_true:
        add("pads-only", 0.0)  # its only large values are the poisoned pads
    exact_rows = len(rows)
    rng = np.random.default_rng(7000 + k_true + (dtype == "bf16"))
    for i in range(4):
        r = rng.uniform(0.0, 2 * v["t"], size=k_true)
        add(f"random-sparse-{i}", 0.0,
            a=(r, slice(None)), b=(0.0, rng.random(k_true) < 0.9))
    for i in range(4):
        add(f"random-dense-{i}", 0.0,
            a=(rng.uniform(0.0, 2 * v["t"], size=k_true), slice(None)))
    # zero-count and full rows alternate: consecutive offsets repeat
    for i in range(3):
        add(f"tail-zero-{i}", 0.0)
        add(f"tail-full-{i}", hi)
    F = np.full((len(rows), kp), hi, dtype=np.float32)  # pads poisoned: 2t
    F[:, :k_true] = np.stack(rows)
    sd = torch.bfloat16 if dtype == "bf16" else torch.float32
    Ft = torch.from_numpy(F).to(sd)
    back = Ft.double().numpy()
    assert (back[:exact_rows, :k_true] == np.stack(rows[:exact_rows])).all(), (
        "a structured K7 value is not representable in " + dtype)
    assert (back[:, k_true:] == hi).all() and len(rows) <= 64
    return Ft, tuple(names)


def k7_rows(k_true: int, kp: int, dtype: str, delta: float = K7_DELTA):
    """[<= 64, kp] CPU tensor in the storage dtype (shared: do not modify).
    Column positions follow chunk = ceil(k_true/256); pad columns
    [k_true, kp) of every row hold 2t."""
    return _k7_build(k_true, kp, dtype, float(delta))[0]


def k7_row_names(k_true: int, kp: int, dtype: str, delta: float = K7_DELTA):
    return _k7_build(k_true, kp, dtype, float(delta))[1]


# ---------------------------------------------------------------- K5 graphs
def _csr_graph(n: int, src, dst) -> Graph:
    """Canonical CSR (sorted rows) from DIRECTED pairs holding both
    directions of every edge.  Built directly, like ladder_graph, so
    isolated ids survive."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    assert not ((src[1:] == src[:-1]) & (dst[1:] == dst[:-1])).any()
    assert not (src == dst).any()
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, src + 1, 1)
    return Graph(indptr=np.cumsum(indptr), indices=dst.astype(np.int32),
                 raw_ids=np.arange(n, dtype=np.int64))


def _clique_pairs(nodes):
    nodes = np.asarray(nodes, dtype=np.int64)
    a, b = np.meshgrid(nodes, nodes, indexing="ij")
    m = a != b
    return a[m], b[m]


def _hub_pool():
    """The hub ladder's leaf pool in join order (centre d joins the first d
    of it): the permutation ladder_graph drew."""
    g, label = ladder_graph("hub")
    n = g.num_nodes
    perm = np.random.default_rng(1234 + len(HUB_DEGREES)).permutation(n)
    pool = perm[: max(HUB_DEGREES)]
    c65 = int(np.flatnonzero(label == 65)[0])
    assert set(g.neighbors(c65).tolist()) == set(pool[:65].tolist())
    return pool


@functools.lru_cache(maxsize=None)
def k5_graphs() -> dict:
    """name -> Graph, all canonical with sorted rows."""
    from bigclam.io import rmat_graph

    out = {"ladder-small": ladder_graph("small")[0],
           "ladder-hub": ladder_graph("hub")[0]}
    # complete graphs: every search hits, vol_T == 0, neighbour rows of
    # length 64 (K65) and 65 (K66)
    for m in (2, 3, 65, 66):
        out[f"K{m}"] = _csr_graph(m, *_clique_pairs(np.arange(m)))
    # star: the centre's row is 257 long (5 lane rounds), centre id inside
    # the id range so leaves miss on both sides
    centre = 100
    leaves = np.setdiff1d(np.arange(258), [centre])
    out["star257"] = _csr_graph(
        258, np.concatenate([np.full(257, centre), leaves]),
        np.concatenate([leaves, np.full(257, centre)]))
    # two K20 joined by one bridge: 0 < cond < 1
    s0, d0 = _clique_pairs(np.arange(20))
    s1, d1 = _clique_pairs(np.arange(20, 40))
    out["two-K20"] = _csr_graph(
        40, np.concatenate([s0, s1, [5, 30]]),
        np.concatenate([d0, d1, [30, 5]]))
    # hub ladder + a clique over the first 70 pool leaves: triangles on the
    # centres, so searches hit at both ends of long rows
    hub = out["ladder-hub"]
    hs = np.repeat(np.arange(hub.num_nodes), np.diff(hub.indptr))
    cs, cd = _clique_pairs(_hub_pool()[:70])
    out["clique-ladder"] = _csr_graph(
        hub.num_nodes, np.concatenate([hs, cs]),
        np.concatenate([hub.indices.astype(np.int64), cd]))
    out["rmat9"] = rmat_graph(9, 6.0, seed=31)
    return out


@functools.lru_cache(maxsize=None)
def k5_oracle(name: str) -> dict:
    """The integer oracle on one K5 graph: deg, z, cut int64 [N] and cond
    float64 [N] (computed once per process)."""
    import oracle

    g = k5_graphs()[name]
    rows = [oracle.conductance_int(g.indptr, g.indices, u)
            for u in range(g.num_nodes)]
    deg, z, cut, cond = (np.array(c) for c in zip(*rows))
    return dict(deg=deg.astype(np.int64), z=z.astype(np.int64),
                cut=cut.astype(np.int64), cond=cond.astype(np.float64))


@functools.lru_cache(maxsize=None)
def k5_fixture_conditions() -> dict:
    """Which kernel edges the K5 graph set reaches (condition -> the first
    graph that shows it, or None).  A search is the lookup of a 2-hop
    endpoint w != u in u's sorted row."""
    found = {}

    def mark(cond, name):
        found.setdefault(cond, name)

    for name, g in k5_graphs().items():
        o = k5_oracle(name)
        vol_s = o["z"] - o["cut"]
        vol_t = len(g.indices) - vol_s - 2 * o["cut"]
        assert (vol_t >= 0).all()  # the max(.., 1) guard cannot fire
        assert ((vol_s == 0) == (o["deg"] == 0)).all()
        if (o["deg"] == 0).any():
            mark("deg==0", name)
        if ((vol_t == 0) & (o["deg"] > 0)).any():
            mark("vol_T==0", name)
        if ((o["cond"] > 0) & (o["cond"] < 1)).any():
            mark("0<cond<1", name)
        if (o["cond"] > 1).any():
            mark("cond>1", name)
        for d in (1, 2, 3, 4, 5):
            if (o["deg"] == d).any():
                mark(f"deg(u)=={d}", name)
        deg = np.diff(g.indptr)
        for u in range(g.num_nodes):
            nu = g.neighbors(u)
            if not len(nu):
                continue
            for ln in (63, 64, 65):
                if (deg[nu] == ln).any():
                    mark(f"neighbour row of {ln}", name)
            w = np.concatenate([g.neighbors(int(v)) for v in nu])
            w = w[w != u]
            if (w == nu[0]).any():
                mark("hit on first", name)
            if (w == nu[-1]).any():
                mark("hit on last", name)
            if (w < nu[0]).any():
                mark("miss below", name)
            if (w > nu[-1]).any():
                mark("miss above", name)
    return found


K5_CONDITIONS = (
    "deg==0", "vol_T==0", "0<cond<1", "cond>1", "hit on first",
    "hit on last", "miss below", "miss above", "neighbour row of 63",
    "neighbour row of 64", "neighbour row of 65", "deg(u)==1", "deg(u)==2",
    "deg(u)==3", "deg(u)==4", "deg(u)==5")


def assert_k5_fixture_conditions():
    found = k5_fixture_conditions()
    missing = [c for c in K5_CONDITIONS if c not in found]
    assert not missing, f"K5 graphs never reach: {missing}"


# ----------------------------------------------------------------- K6 cases
K6_KP = {8: 8, 37: 40, 600: 608}  # number of seeds -> padded width


@functools.lru_cache(maxsize=None)
def k6_seed_lists() -> dict:
    """number of seeds -> int64 seed list on the hub ladder.  Every list
    starts with the centres of degree 1, 255, 256, 257, 513 and 600, one
    leaf and one isolated node; the 600-seed list (more than one 256-column
    round, longer than a block) repeats nodes, which is fine: columns
    differ."""
    g, label = ladder_graph("hub")
    base = [int(np.flatnonzero(label == d)[0])
            for d in (1, 255, 256, 257, 513, 600)]
    base += [int(np.flatnonzero(label == -1)[0]),
             int(np.flatnonzero(label == -2)[0])]
    rest = [int(u) for u in np.flatnonzero(label >= 0) if int(u) not in base]
    rest += [int(u) for u in np.flatnonzero(label == -1)[1:11]]
    rng = np.random.default_rng(600)
    many = base + rng.integers(0, g.num_nodes, size=592).tolist()
    out = {8: base, 37: base + rest[:29], 600: many}
    assert all(len(v) == k for k, v in out.items())
    return {k: np.asarray(v, dtype=np.int64) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def k6_shards() -> dict:
    """Row ranges on the hub ladder: the whole graph, a 3-way split whose
    middle shard [a, b) has seed neighbours exactly on a (start), b - 1
    (stop - 1) and b (stop), and the empty shard (a, a)."""
    g, label = ladder_graph("hub")
    n = g.num_nodes
    nb = set(g.neighbors(int(np.flatnonzero(label == 600)[0])).tolist())
    a = next(x for x in range(n // 3, n) if x in nb)
    b = next(x for x in range(2 * n // 3, n - 1) if x in nb and x - 1 in nb)
    assert 0 < a < b - 1 < b < n
    return {"full": (0, n), "split": ((0, a), (a, b), (b, n)),
            "empty": (a, a)}


@functools.lru_cache(maxsize=None)
def k7_oracle(k_true: int, kp: int, dtype: str):
    """oracle.memberships on one K7 fixture (computed once per process)."""
    import oracle

    F = k7_rows(k_true, kp, dtype)
    return oracle.memberships(F.double().numpy(), k_true, K7_DELTA)


@functools.lru_cache(maxsize=None)
def k6_oracle(n_seeds: int, shard: tuple, include_seed: bool, fill: float):
    """oracle.seed_scatter on the hub ladder at the padded width of the
    seed list (computed once per process)."""
    import oracle

    g, _ = ladder_graph("hub")
    return oracle.seed_scatter(g.indptr, g.indices, k6_seed_lists()[n_seeds],
                               shard[0], shard[1], K6_KP[n_seeds],
                               include_seed, fill)


def k6_all_shards():
    s = k6_shards()
    return (s["full"],) + s["split"] + (s["empty"],)
