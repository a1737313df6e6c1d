"""Sparse form of a fitted affiliation matrix F, in both orientations.

A converged F is a fraction of a percent dense, so everything that asks
"which nodes share a community with u" wants the nonzeros only, by row and
by column:

  row-major     row_ptr int64 [N+1], row_col int32 [nnz] ascending per row,
                row_val float32 [nnz]
  column-major  col_ptr int64 [K+1], col_row int32 [nnz] ascending per
                column, col_val float32 [nnz]

Both describe the same (row, column, value) triples.  Values are fp32
whatever F's storage type (the bf16 -> fp32 upcast is exact), so there is
one value type downstream.  Only the first ``k`` columns of F are read:
storage padding is not part of the model.  The tensors live on the device F
lives on; ``numpy()`` gives the host arrays the CPU implementation takes.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict

import numpy as np
import torch

DEFAULT_MAX_NNZ = 1 << 28


def _ptr(ids: torch.Tensor, size: int) -> torch.Tensor:
    """CSR pointer [size+1] of sorted ids in [0, size)."""
    ptr = torch.zeros(size + 1, device=ids.device, dtype=torch.int64)
    if ids.numel():
        torch.cumsum(torch.bincount(ids, minlength=size), 0, out=ptr[1:])
    return ptr


@dataclass
class SparseModel:
    n: int
    k: int
    row_ptr: torch.Tensor
    row_col: torch.Tensor
    row_val: torch.Tensor
    col_ptr: torch.Tensor
    col_row: torch.Tensor
    col_val: torch.Tensor
    columns_dropped: int = 0

    @property
    def nnz(self) -> int:
        return int(self.row_col.shape[0])

    @property
    def device(self) -> torch.device:
        return self.row_ptr.device

    @classmethod
    def from_triples(cls, rows: torch.Tensor, cols: torch.Tensor,
                     vals: torch.Tensor, n: int, k: int) -> "SparseModel":
        """From the nonzeros listed in row-major order (rows ascending,
        columns ascending within a row)."""
        rows = rows.to(torch.int64)
        cols = cols.to(torch.int64)
        vals = vals.to(torch.float32)
        order = torch.sort(cols, stable=True).indices
        return cls(
            n=int(n), k=int(k),
            row_ptr=_ptr(rows, n),
            row_col=cols.to(torch.int32),
            row_val=vals.contiguous(),
            col_ptr=_ptr(cols, k),
            col_row=rows[order].to(torch.int32),
            col_val=vals[order].contiguous(),
        )

    @classmethod
    def from_F(cls, F: torch.Tensor, k: int = None,
               max_nnz: int = DEFAULT_MAX_NNZ) -> "SparseModel":
        """From a dense F [N, >= k] (fp32 or bf16), on F's device."""
        k = F.shape[1] if k is None else int(k)
        rows, cols, vals = nonzero_triples(F, k, max_nnz=max_nnz)
        return cls.from_triples(rows, cols, vals, F.shape[0], k)

    def drop_columns_larger_than(self, m: int) -> "SparseModel":
        """A model without the columns that have more than ``m`` members,
        removed from BOTH orientations, so a score is consistently the dot
        over the remaining columns.  ``columns_dropped`` counts them."""
        sizes = self.col_ptr[1:] - self.col_ptr[:-1]
        big = sizes > int(m)
        dropped = int(big.sum())
        if dropped == 0:
            return replace(self)
        keep_r = ~big[self.row_col.long()]
        col_ids = torch.repeat_interleave(
            torch.arange(self.k, device=self.device), sizes
        )
        keep_c = ~big[col_ids]
        row_ids = torch.repeat_interleave(
            torch.arange(self.n, device=self.device),
            self.row_ptr[1:] - self.row_ptr[:-1],
        )
        return SparseModel(
            n=self.n, k=self.k,
            row_ptr=_ptr(row_ids[keep_r], self.n),
            row_col=self.row_col[keep_r],
            row_val=self.row_val[keep_r],
            col_ptr=_ptr(col_ids[keep_c], self.k),
            col_row=self.col_row[keep_c],
            col_val=self.col_val[keep_c],
            columns_dropped=self.columns_dropped + dropped,
        )

    def to(self, device) -> "SparseModel":
        return replace(self, **{
            f: getattr(self, f).to(device) for f in _ARRAYS
        })

    def numpy(self) -> Dict[str, np.ndarray]:
        return {f: getattr(self, f).cpu().numpy() for f in _ARRAYS}


_ARRAYS = ("row_ptr", "row_col", "row_val", "col_ptr", "col_row", "col_val")


def nonzero_triples(F: torch.Tensor, k: int, row_offset: int = 0,
                    max_nnz: int = DEFAULT_MAX_NNZ):
    """``(rows int64, cols int64, vals float32)`` of the nonzeros of
    ``F[:, :k]`` in row-major order, rows shifted by ``row_offset``.  The
    nonzeros are counted first: a dense F is refused, not materialised."""
    sub = F[:, :k]
    count = int(torch.count_nonzero(sub))
    if count > max_nnz:
        raise ValueError(
            f"F has {count} nonzeros, more than max_nnz = {max_nnz}: the "
            "sparse model form is for a fitted (sparse) F"
        )
    idx = torch.nonzero(sub)  # row-major
    rows, cols = idx[:, 0], idx[:, 1]
    return rows + int(row_offset), cols, sub[rows, cols].to(torch.float32)
