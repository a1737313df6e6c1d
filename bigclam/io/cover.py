"""Covers (sets of possibly overlapping communities) and their file format.

A cover file has one community per line, whitespace-separated raw node ids.
Two dialects are accepted: the SNAP ``*.cmty.txt`` ground-truth format (no
prefix) and this project's own ``fit --out`` format (``<community-id>: ids``,
engine/extract.py).  ``#`` starts a comment; blank lines are skipped.

:class:`Cover` holds the membership pairs over DENSE node ids ``0..n-1``
sorted by (community, node), in both CSR views the evaluation needs:
group-major (members of each community) and node-major (communities of each
node, ascending — the shape K7 emits).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class Cover:
    n: int  # number of nodes the dense ids range over
    num_comms: int  # G (empty communities included)
    grp_ptr: np.ndarray  # int64 [G+1]
    grp_nodes: np.ndarray  # int32 [M] members, ascending per community
    node_ptr: np.ndarray  # int64 [n+1]
    node_comm: np.ndarray  # int32 [M] communities, ascending per node
    sizes: np.ndarray  # int32 [G]
    dropped: int = 0  # member ids that were not in the graph (loader)
    _dev: dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def num_pairs(self) -> int:
        return len(self.grp_nodes)

    @property
    def comms(self) -> np.ndarray:
        """Community id of every (community, node) pair, int32 [M]."""
        return np.repeat(
            np.arange(self.num_comms, dtype=np.int32), self.sizes
        )

    @property
    def nodes(self) -> np.ndarray:
        return self.grp_nodes

    def members(self, c: int) -> np.ndarray:
        return self.grp_nodes[self.grp_ptr[c] : self.grp_ptr[c + 1]]

    @classmethod
    def from_pairs(
        cls, comms, nodes, n: int, num_comms: Optional[int] = None,
        dropped: int = 0,
    ) -> "Cover":
        """From (community, node) membership pairs in any order (duplicates
        merged) — what ``extract_communities_sharded`` returns on rank 0."""
        comms = np.asarray(comms, dtype=np.int64).reshape(-1)
        nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
        if len(comms) != len(nodes):
            raise ValueError("comms and nodes differ in length")
        n = int(n)
        if n >= 1 << 31:
            raise ValueError("covers support N < 2^31 nodes")
        if num_comms is None:
            num_comms = int(comms.max()) + 1 if len(comms) else 0
        g = int(num_comms)
        if len(comms):
            if comms.min() < 0 or comms.max() >= g:
                raise ValueError("community id out of range")
            if nodes.min() < 0 or nodes.max() >= n:
                raise ValueError("node id out of range")
        # one int64 key sort gives (community, node) order and the dedupe
        key = np.unique(comms * max(n, 1) + nodes)
        c = key // max(n, 1)
        u = key % max(n, 1)
        sizes = np.bincount(c, minlength=g).astype(np.int32)
        grp_ptr = np.zeros(g + 1, dtype=np.int64)
        np.cumsum(sizes, out=grp_ptr[1:])
        # node-major view: stable sort by node keeps communities ascending
        order = np.argsort(u, kind="stable")
        node_ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(u, minlength=n), out=node_ptr[1:])
        return cls(
            n=n,
            num_comms=g,
            grp_ptr=grp_ptr,
            grp_nodes=u.astype(np.int32),
            node_ptr=node_ptr,
            node_comm=c[order].astype(np.int32),
            sizes=sizes,
            dropped=int(dropped),
        )

    @classmethod
    def from_members(
        cls, members: Sequence[np.ndarray], n: int, dropped: int = 0
    ) -> "Cover":
        """From per-community arrays of DENSE node ids."""
        lens = np.array([len(m) for m in members], dtype=np.int64)
        comms = np.repeat(np.arange(len(members), dtype=np.int64), lens)
        nodes = (
            np.concatenate([np.asarray(m, dtype=np.int64) for m in members])
            if len(members) and lens.sum()
            else np.empty(0, dtype=np.int64)
        )
        return cls.from_pairs(
            comms, nodes, n, num_comms=len(members), dropped=dropped
        )

    @classmethod
    def from_raw_members(
        cls, members: Sequence[np.ndarray], raw_ids: np.ndarray
    ) -> "Cover":
        """From per-community arrays of RAW ids and a graph's sorted
        ``raw_ids`` table: ids are mapped to dense ids by ``searchsorted``;
        ids that are not in the table are dropped and counted in
        ``dropped`` (a community may end up empty)."""
        raw_ids = np.asarray(raw_ids, dtype=np.int64)
        n = len(raw_ids)
        lens = np.array([len(m) for m in members], dtype=np.int64)
        comms = np.repeat(np.arange(len(members), dtype=np.int64), lens)
        raw = (
            np.concatenate([np.asarray(m, dtype=np.int64) for m in members])
            if len(members) and lens.sum()
            else np.empty(0, dtype=np.int64)
        )
        pos = np.searchsorted(raw_ids, raw)
        ok = pos < n
        ok[ok] = raw_ids[pos[ok]] == raw[ok]
        # duplicates within a line are merged by from_pairs; count each
        # unknown (community, id) once
        bad = np.stack([comms[~ok], raw[~ok]], axis=1)
        dropped = len(np.unique(bad, axis=0)) if len(bad) else 0
        return cls.from_pairs(
            comms[ok], pos[ok], n, num_comms=len(members), dropped=dropped
        )


def read_cover_lines(path: str) -> List[np.ndarray]:
    """Parse a cover file into per-community arrays of raw ids (duplicates
    within a line removed, ascending).  ``<id>:`` with no members is an
    empty community; blank and ``#`` lines are skipped."""
    out: List[np.ndarray] = []
    with open(path, "r") as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            if ":" in line:
                line = line.split(":", 1)[1]
            toks = line.split()
            ids = (
                np.array([int(t) for t in toks], dtype=np.int64)
                if toks
                else np.empty(0, dtype=np.int64)
            )
            out.append(np.unique(ids))
    return out


def load_cover(path: str, raw_ids: Optional[np.ndarray] = None) -> Cover:
    """Load a cover file.  With ``raw_ids`` (a graph's sorted raw-id table)
    members map to that graph's dense ids and unknown ids are dropped
    (``Cover.dropped``); without, ids are densified over the file's own."""
    members = read_cover_lines(path)
    if raw_ids is None:
        raw_ids = (
            np.unique(np.concatenate(members))
            if any(len(m) for m in members)
            else np.empty(0, dtype=np.int64)
        )
    return Cover.from_raw_members(members, raw_ids)
