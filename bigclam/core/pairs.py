"""Pair plan for scoring arbitrary node pairs against a row-sharded F.

A pair ``(u, v)`` with ``u < v`` belongs to the rank that owns row ``u``.
Row ``v`` may live on another rank; the distinct off-shard ``v`` rows of a
rank's pairs form its *extra* section, in ascending global id (which is
also ascending owner-rank order), exactly like the halo section of
``core/shard.py``.  Every rank derives the whole exchange plan from the
global pair list and the trainer's partition bounds, so the plan needs no
bootstrap communication.

Local row space of a pair shard: ``[0, n_own)`` = the rank's owned F rows,
``[n_own, n_own + n_extra)`` = the extra rows.  The two sections are two
separate buffers (K9 takes both base pointers); ``ShardState``'s own halo
section and F buffer are not involved.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from .. import comm
from .shard import HaloPlan


@dataclass
class PairShard:
    rank: int
    world_size: int
    start: int  # first owned global id
    stop: int  # one past the last owned global id
    sel: np.ndarray  # int64: which of the global pairs this rank scores
    pu: np.ndarray  # int32 [len(sel)], local row index of u (always owned)
    pv: np.ndarray  # int32 [len(sel)], local row index of v (owned or extra)
    extra_globals: np.ndarray  # int64 [n_extra], ascending
    plan: HaloPlan
    counts: List[int]  # pairs per rank (rank 0 sizes its receives from it)

    @property
    def n_own(self) -> int:
        return self.stop - self.start

    @property
    def n_extra(self) -> int:
        return len(self.extra_globals)


def pair_owner(u: np.ndarray, bounds: np.ndarray) -> np.ndarray:
    """Rank owning each row of ``u`` under contiguous ``bounds`` (ranks
    with an empty range own nothing)."""
    return np.searchsorted(bounds, u, side="right") - 1


def make_pair_shard(pairs: np.ndarray, bounds: np.ndarray, rank: int,
                    world_size: int) -> PairShard:
    """Build rank's share of ``pairs`` (int64 [P, 2], ``u <= v``, global
    ids, any order) and the all-to-all plan that fetches its extra rows."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    bounds = np.asarray(bounds, dtype=np.int64)
    n = int(bounds[-1])
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= n):
        raise IndexError(f"pair ids must be in [0, {n})")
    if (pairs[:, 0] > pairs[:, 1]).any():
        raise ValueError("pairs must be canonical (u <= v)")
    u, v = pairs[:, 0], pairs[:, 1]
    owner = pair_owner(u, bounds)
    start, stop = int(bounds[rank]), int(bounds[rank + 1])

    # every rank's extra list (needed for both sides of the plan)
    extras = []
    for p in range(world_size):
        ps, pe = int(bounds[p]), int(bounds[p + 1])
        vp = v[owner == p]
        extras.append(np.unique(vp[(vp < ps) | (vp >= pe)]))
    mine = extras[rank]

    send_idx: List[np.ndarray] = []
    recv_counts: List[int] = []
    for p in range(world_size):
        ps, pe = int(bounds[p]), int(bounds[p + 1])
        if p == rank:
            send_idx.append(np.empty(0, dtype=np.int64))
            recv_counts.append(0)
            continue
        want = extras[p]
        send_idx.append(want[(want >= start) & (want < stop)] - start)
        recv_counts.append(int(((mine >= ps) & (mine < pe)).sum()))

    sel = np.flatnonzero(owner == rank)
    n_own = stop - start
    vs = v[sel]
    off = (vs < start) | (vs >= stop)
    pv = np.empty(len(sel), dtype=np.int64)
    pv[~off] = vs[~off] - start
    pv[off] = n_own + np.searchsorted(mine, vs[off])
    return PairShard(
        rank=rank,
        world_size=world_size,
        start=start,
        stop=stop,
        sel=sel,
        pu=(u[sel] - start).astype(np.int32),
        pv=pv.astype(np.int32),
        extra_globals=mine,
        plan=HaloPlan(send_idx=send_idx, recv_counts=recv_counts),
        counts=np.bincount(owner, minlength=world_size).tolist(),
    )


def fetch_extra_rows(state, ps: PairShard) -> torch.Tensor:
    """The extra rows of ``ps`` as a ``[n_extra, kp]`` buffer of its own,
    in F's storage dtype: one dense all-to-all of the owners' current
    rows.  Collective — every rank calls it, also with nothing to fetch.
    On gloo, bf16 travels as fp32 (exact), as in
    ``ShardState.halo_exchange``."""
    recv = torch.empty(
        ps.n_extra, state.kp, device=state.device, dtype=state.storage_dtype
    )
    if ps.world_size == 1:
        return recv
    plan = ps.plan
    idx = torch.from_numpy(
        np.concatenate(plan.send_idx) if plan.total_send
        else np.empty(0, dtype=np.int64)
    ).to(state.device)
    send = state.F_local.index_select(0, idx)
    if state.storage_dtype == torch.bfloat16 and comm.backend() == "gloo":
        recv32 = torch.empty_like(recv, dtype=torch.float32)
        comm.all_to_all(
            recv32, send.float(), plan.recv_counts, plan.send_counts
        )
        recv.copy_(recv32)
        return recv
    comm.all_to_all(recv, send, plan.recv_counts, plan.send_counts)
    return recv
