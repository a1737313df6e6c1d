"""Three row shards driven in lockstep in ONE process (docs/kernels.md, C6).

``Lockstep`` holds one ``ShardState`` per rank and provides the two
collectives that are no-ops without a process group: the halo exchange
(``exchange``) and the sumF all-reduce (``reduce_sumF``).  One sweep is
exchange -> grad_ls_auto per rank -> (judge) -> apply_commit per rank ->
reduce_sumF, the order of ``Trainer.prologue`` / ``pipelined_sweep``.

With ``device="cpu"`` the states run the fp32 torch reference, so the driver
itself, the fixture conditions and the sharpness of the judge are checked
without a GPU (tests/test_shard_lockstep_oracle.py); on the device the same
driver runs the sparse sweep kernels (tests/test_gpu_shard_sparse.py).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import contract_fixtures as cf
from bigclam.core.shard import make_shard
from bigclam.core.state import ShardState

WORLD = 3
SWEEPS = 4
# The C6 fixture is the C5 state (hub ladder, sparse regime, K=512) with
# three changes, each found on the CPU reference (docs/kernels.md, C6):
#  - the ladder stops at 1e-6 (ls_steps=6).  With the full 16-rung ladder
#    every node that rejects the first seven rungs picks among steps of
#    1e-7 .. 1e-15, which move no fp32 entry: those picks are coin tosses,
#    and from the second sweep on 13-70 of the 627 reference picks differ
#    from the exact pick (cap: 12) on every seed tried.
#  - seed 4 of make_F.  After a commit some edges have x in [1e-4, 5e-4];
#    there the rounding of p = exp(-x), which the scale A does not model,
#    puts the REFERENCE's own gradient at up to 1250 eps32 A on some seeds
#    (C_GRAD = 512).  Of 48 seeds, 4 is the one whose four-sweep reference
#    trajectory stays furthest inside the constants (grad 13 / 512,
#    llh 2.5 / 128, no differing pick).
#  - two settings of cap / wcap, because on this trajectory only leaves
#    accept steps (a centre's edges to disjoint supports sit on the max_p
#    clamp, its gradient is ~1e4 |fv| and only steps below 1e-6 pass):
#    "wide" (4096 / 144) routes the mid-degree centres, the owned nodes
#    that read the halo lists of leaves that CHANGED in the last commit,
#    but its dense class is the hubs, which never move; "tight"
#    (320 / 144) puts ~15 % of every rank (accepting leaves among them)
#    into the dense class, so the listed dense commit, the dirty flags and
#    the list-mode rescan have work on every sweep.
C6_LS_STEPS = 6
C6_SEED = 4
CONFIGS = {"wide": (4096, 144), "tight": (320, 144)}  # name -> (cap, wcap)
CAP, WCAP = CONFIGS["tight"]
OVER_CAP = 256  # BIGCLAM_SPARSE_CAP of the over-cap halo fixture
OVER_NNZ = 400  # support of a densified leaf row


@functools.lru_cache(maxsize=None)
def c6_case(dtype):
    base = cf.make_case("hub", "sparse", dtype, 512)
    return dataclasses.replace(
        base, cfg=dataclasses.replace(base.cfg, ls_steps=C6_LS_STEPS),
        F0=cf.make_F(base.graph, base.k, "sparse", seed=C6_SEED))


def c6_cases():
    return ("fp32", "bf16")


def bits(F):
    return F.view(torch.int16 if F.dtype == torch.bfloat16 else torch.int32)


class NoWait:
    """Halo work handle whose rows are already in place; counts its calls."""

    def __init__(self):
        self.calls = 0

    def wait(self):
        self.calls += 1


class LateHalo:
    """Halo work handle that delivers the true halo rows only inside
    ``wait()`` (a copy on the current stream), and counts its calls."""

    def __init__(self, dst, rows):
        self.dst, self.rows, self.calls = dst, rows, 0

    def wait(self):
        self.calls += 1
        self.dst.copy_(self.rows)


class Lockstep:
    def __init__(self, case, world_size=WORLD, device="cpu"):
        self.case = case
        self.ws = world_size
        self.device = torch.device(device)
        g = case.graph
        self.cfg = dataclasses.replace(case.cfg, device=self.device.type)
        F0 = case.stored_F()
        sumF = F0.float().sum(dim=0)
        self.states = []
        for r in range(world_size):
            sh = make_shard(g, r, world_size)
            st = ShardState(sh, self.cfg, device=self.device)
            nl = sh.n_local
            st.F[:nl] = F0[sh.start: sh.stop].to(self.device)
            st.F[nl:] = F0[torch.from_numpy(sh.halo_globals)].to(self.device)
            st.sumF = sumF.to(self.device)
            self.states.append(st)
        self.sumF = sumF.to(self.device)  # the global sumF every rank holds
        self.outs = [None] * world_size  # (grad, llh, best, pack) per rank

    # ------------------------------------------------------- collectives
    def global_F(self):
        """Owned rows of every rank stitched back to [N, kp]."""
        return torch.cat([st.F_local for st in self.states], dim=0)

    def halo_rows(self, r, G=None):
        """The current owners' rows of rank r's halo section (a copy)."""
        G = self.global_F() if G is None else G
        hg = torch.from_numpy(self.states[r].shard.halo_globals)
        return G[hg.to(self.device)]

    def exchange(self):
        """Every halo row bitwise from its owner's F_local."""
        G = self.global_F()
        for r, st in enumerate(self.states):
            st.F[st.n_local:].copy_(self.halo_rows(r, G))

    def reduce_sumF(self):
        """After all ranks committed: every st.sumF is that rank's partial
        (the all-reduce did nothing); add them in rank order in fp32 and
        give each state its own copy of the total."""
        total = self.states[0].sumF.clone()
        for st in self.states[1:]:
            total = total + st.sumF
        for st in self.states:
            st.sumF = total.clone()
        self.sumF = total
        return total

    # ------------------------------------------------------------ phases
    def grad_ls(self, r, handle=None):
        self.outs[r] = self.states[r].grad_ls_auto(handle)
        return self.outs[r]

    def commit(self, r):
        grad, _, best, pack = self.outs[r]
        self.states[r].apply_commit(grad, best, pack)

    def judge(self):
        """Oracle of the CURRENT global state (call before the commits)."""
        c = self.case
        return cf.Judge(self.global_F(), self.sumF, c.graph.indptr,
                        c.graph.indices, self.cfg, c.label, c.k, c.dtype)

    def stitched(self, grads=None):
        """(grad [N, kp], llh [N], best [N]) of all nodes by global id, on
        the CPU.  ``grads`` overrides the per-rank gradient rows (the
        rebuilt compact gradients of a routed sweep)."""
        gs = [o[0] for o in self.outs] if grads is None else grads
        cpu = lambda t: torch.as_tensor(t).cpu()  # noqa: E731
        return (torch.cat([cpu(x) for x in gs]),
                torch.cat([cpu(o[1]) for o in self.outs]),
                torch.cat([cpu(o[2]) for o in self.outs]))

    def sweep(self, tag=None, check=True):
        """One lockstep sweep; with ``check`` every node is judged against
        the oracle of the global state.  Returns the judge's figures."""
        self.exchange()
        for r in range(self.ws):
            self.grad_ls(r, NoWait())
        fig = None
        if check:
            fig = self.judge().check(tag or self.case.id, *self.stitched())
        for r in range(self.ws):
            self.commit(r)
        self.reduce_sumF()
        return fig


# --------------------------------------------------- routing emulation (CPU)
def row_has_halo(shard):
    """bool [n_local]: the node has a neighbour in the halo section."""
    remote = np.asarray(shard.indices) >= shard.n_local
    cs = np.concatenate([[0], np.cumsum(remote)])
    ip = np.asarray(shard.indptr)
    return (cs[ip[1:]] - cs[ip[:-1]]) > 0


def emulated_classes(st, cap, wcap):
    """Routing classes of one rank from the rows it holds NOW, by
    ``ShardState.sparse_bounds``: dict(nnz [n_rows], bound [n_local],
    wave / block / dense: local node ids)."""
    nnz = (st.F.float() != 0).sum(dim=1).to(torch.int32).cpu()
    bound, _ = ShardState.sparse_bounds(
        nnz, st.indptr.cpu(), st.indices.cpu().long(), st.n_local)
    bound = bound.numpy()
    return dict(nnz=nnz.numpy(), bound=bound,
                wave=np.flatnonzero(bound <= wcap),
                block=np.flatnonzero((bound > wcap) & (bound <= cap)),
                dense=np.flatnonzero(bound > cap))


# ------------------------------------------------- over-cap halo fixture
@functools.lru_cache(maxsize=None)
def over_cap_leaves(kind="hub", world_size=WORLD):
    """Global ids of the leaves the over-cap fixture densifies: per rank the
    three halo leaves of smallest degree (ties by id), so that few centres
    leave the routed classes.  Deterministic; the conditions it must meet
    are asserted in tests/test_shard_lockstep_oracle.py."""
    g, label = cf.ladder_graph(kind)
    deg = np.diff(np.asarray(g.indptr))
    chosen = []
    for r in range(world_size):
        sh = make_shard(g, r, world_size)
        hg = sh.halo_globals
        leaves = hg[label[hg] == -1]
        o = np.lexsort((leaves, deg[leaves]))
        chosen += leaves[o[:3]].tolist()
    return tuple(sorted(set(chosen)))


@functools.lru_cache(maxsize=None)
def over_cap_case(dtype):
    """The C5 case with the chosen leaf rows densified to OVER_NNZ
    non-zeros (columns and values drawn once, values of the size the
    sparse regime's kept entries have)."""
    base = cf.make_case("hub", "sparse", dtype, 512)
    F0 = base.F0.copy()
    rng = np.random.default_rng(4242)
    for v in over_cap_leaves():
        cols = rng.choice(base.k, size=OVER_NNZ, replace=False)
        F0[v] = 0.0
        F0[v, cols] = rng.uniform(0.05, 0.4, size=OVER_NNZ)
    return cf.Case(base.kind, base.regime, dtype, base.k, base.graph,
                   base.label, base.cfg, F0.astype(np.float32))


# --------------------------------- list-based stand-in of the sparse path
class ListLockstep(Lockstep):
    """CPU stand-in of the sparse sweep's data flow: every rank keeps
    persistent support lists (count, ascending columns, values; one
    ``cap``-strided slot per row of its buffer, halo rows included) and
    computes the sweep from the rows REBUILT FROM THE LISTS, as
    ops/sparse_cpu.py computes from CSR rows.  ``stale`` names (rank, local
    row) pairs whose list is not rescanned: the defect a wrong halo slice
    would cause."""

    def __init__(self, case, cap=CAP, device="cpu", stale=()):
        super().__init__(case, device=device)
        self.cap = cap
        self.stale = set(stale)
        self.lists = [None] * self.ws

    def scan(self, r):
        st = self.states[r]
        n_rows, cap = st.F.shape[0], self.cap
        Fh = st.F.float().numpy()
        if self.lists[r] is None:
            self.lists[r] = (np.zeros(n_rows, np.int32),
                             np.full(n_rows * cap, -1, np.int32),
                             np.zeros(n_rows * cap, np.float32))
            skip = set()
        else:
            skip = {row for (rk, row) in self.stale if rk == r}
        sc, si, sv = self.lists[r]
        for row in range(n_rows):
            if row in skip:
                continue
            ks, vs = cf.rescan(Fh, row)
            sc[row] = len(ks)
            if len(ks) <= cap:
                si[row * cap: row * cap + len(ks)] = ks
                sv[row * cap: row * cap + len(ks)] = vs

    def rebuilt(self, r):
        st = self.states[r]
        sc, si, sv = self.lists[r]
        cap = self.cap
        Fh = np.zeros(tuple(st.F.shape), np.float32)
        for row in range(Fh.shape[0]):
            if sc[row] > cap:  # over-cap rows are read dense
                Fh[row] = st.F[row].float().numpy()
                continue
            sl = slice(row * cap, row * cap + int(sc[row]))
            Fh[row, si[sl]] = sv[sl]
        return torch.from_numpy(Fh).to(st.F.dtype)

    def grad_ls(self, r, handle=None):
        if handle is not None:
            handle.wait()
        self.scan(r)
        st = self.states[r]
        F_true = st.F
        st.F = self.rebuilt(r)
        try:
            self.outs[r] = st.grad_ls_auto(None)
        finally:
            st.F = F_true
        return self.outs[r]
