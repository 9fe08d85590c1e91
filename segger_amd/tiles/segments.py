"""Rows grouped into contiguous segments: the one store behind partition tiles, shards and prediction bins."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor


class Segments:
    """``n`` contiguous segments of a row store: segment ``t`` owns rows ``[indptr[t], indptr[t + 1])``.

    ``sizes`` and ``indptr`` (``[n + 1]``) live on the device of the labels / sizes they were built from; ``ptr`` is the
    host copy of ``indptr``, so that slicing and offset arithmetic never synchronise.  ``perm`` is the stable order that
    produced the grouping (``from_labels`` only)."""

    __slots__ = ("sizes", "indptr", "ptr", "perm")

    def __init__(self, sizes: Tensor, perm: Optional[Tensor] = None):
        """Segments of the given sizes, in order (a 1-d integer tensor)."""
        self.sizes = sizes
        self.indptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
        self.ptr: List[int] = self.indptr.tolist()
        self.perm = perm

    @classmethod
    def from_labels(cls, labels: Tensor, n: int, what: str = "rows") -> "Segments":
        """Group rows by their label in ``[0, n)``: ``perm`` is the stable argsort, so rows keep their order inside a
        segment."""
        labels = labels.long()
        if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= n):
            raise ValueError(f"{what}: tile labels must lie in [0, {n})")
        return cls(torch.bincount(labels, minlength=n), torch.argsort(labels, stable=True))

    def with_ends(self) -> "Segments":
        """The segments of a store that keeps one extra entry behind every segment of this one: segment ``t`` owns
        ``[ptr[t] + t, ptr[t + 1] + t + 1)`` there, i.e. the same segments, each one longer."""
        return Segments(self.sizes + 1)

    def span(self, t: int) -> Tuple[int, int]:
        return self.ptr[t], self.ptr[t + 1]

    def size(self, t: int) -> int:
        return self.ptr[t + 1] - self.ptr[t]

    def view(self, v: Tensor, t: int, dim: int = 0) -> Tensor:
        """Segment ``t`` of ``v`` along ``dim``: always a view."""
        return self.take(v, (t,), dim)

    def take(self, v: Tensor, ids: Sequence[int], dim: int = 0) -> Tensor:
        """Segments ``ids`` of ``v`` back to back: the view for one id, an empty view for none, else one copy."""
        p = self.ptr
        if len(ids) == 1:                                    # every single-tile step, per attribute: no further call
            a, b = p[ids[0]], p[ids[0] + 1]
            return v[a:b] if dim == 0 else v[:, a:b] if dim == 1 else v.narrow(dim, a, b - a)
        if not ids:
            return v.narrow(dim, 0, 0)
        if dim == 0:                                         # (a prediction tile takes dozens of bins: no call per segment)
            return torch.cat([v[p[t]:p[t + 1]] for t in ids])
        if dim == 1:
            return torch.cat([v[:, p[t]:p[t + 1]] for t in ids], 1)
        return torch.cat([v.narrow(dim, p[t], p[t + 1] - p[t]) for t in ids], dim)

    def layout(self, ids: Sequence[int]) -> Tuple[List[int], List[int], int]:
        """Host lists for segments ``ids`` laid back to back: their sizes, the first row of each, the total."""
        p = self.ptr
        sizes, bases, run = [], [], 0
        for t in ids:
            bases.append(run)
            sizes.append(p[t + 1] - p[t])
            run += sizes[-1]
        return sizes, bases, run
