"""The ring layer of the Python side, shared by :mod:`segger_amd.morphology` and :mod:`segger_amd.geometry` as
csrc/rings.h is by their kernels: a CSR of rings is ``ring_offsets`` ``[P + 1]`` and ``xy`` ``[V, 2]``, polygon ``p`` being
``xy[ring_offsets[p]:ring_offsets[p + 1]]``, either orientation, with or without a closing duplicate of its first vertex.
"""
from typing import Tuple

import torch
from torch import Tensor

from . import _lib as L

__all__ = ["ring_csr", "raise_ring_errors", "rings_from_padded"]


def ring_csr(who: str, ring_offsets: Tensor, xy: Tensor) -> Tuple[Tensor, Tensor, int, int]:
    """The CSR as the device code reads it (int64 offsets, float64 ``xy``, contiguous) and its sizes, or ``ValueError`` in
    the name of the caller ``who``.  Waits for the device once (the longest ring)."""
    if not isinstance(ring_offsets, Tensor) or not isinstance(xy, Tensor):
        raise ValueError(f"{who}: ring_offsets and xy are tensors")
    if ring_offsets.dim() != 1 or ring_offsets.numel() < 1 or ring_offsets.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: ring_offsets is an int64 (or int32) vector of n_polygons + 1 entries")
    if xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_floating_point():
        raise ValueError(f"{who}: xy is a floating-point [n_vertices, 2] tensor")
    if ring_offsets.device != xy.device:
        raise ValueError(f"{who}: ring_offsets and xy are on different devices")
    n_polygons, n_vertices = int(ring_offsets.numel()) - 1, int(xy.shape[0])
    ring_offsets = ring_offsets.detach().to(torch.int64).contiguous()
    xy = xy.detach().to(torch.float64).contiguous()
    if n_polygons > 0:
        # the cap is refused here, before the call: the ring lengths are device memory the C entry point cannot read
        # without a synchronisation (a closing duplicate vertex does not count, hence the + 1)
        longest, where = (ring_offsets[1:] - ring_offsets[:-1]).max(dim=0)
        longest, where = int(longest), int(where)
        if longest > L.MORPH_MAX_VERTS + 1 or (longest == L.MORPH_MAX_VERTS + 1 and not torch.equal(
                xy[int(ring_offsets[where])], xy[int(ring_offsets[where + 1]) - 1])):
            raise ValueError(f"{who}: polygon {where} has {longest} vertices, more than SEGGER_MORPH_MAX_VERTS = "
                             f"{L.MORPH_MAX_VERTS}")
    return ring_offsets, xy, n_polygons, n_vertices


def raise_ring_errors(who: str, flag: int, ring_offsets: Tensor, n_vertices: int) -> None:
    """``ValueError`` for a non-zero error word ``flag`` (``ws[:4]``; reading it is the caller's synchronisation): bad offsets
    name the first polygon that has them, every other bit, a unit's own included, is reported as the word."""
    if flag & L.MORPH_ERR_OFFSETS:                                   # == PJOIN_ERR_OFFSETS: csrc/rings.h asserts it
        bad = (ring_offsets[:-1] < 0) | (ring_offsets[1:] < ring_offsets[:-1]) | (ring_offsets[1:] > n_vertices)
        raise ValueError(f"{who}: ring_offsets of polygon {int(bad.nonzero()[0])} are negative, descending or beyond the "
                         f"{n_vertices} vertices")
    if flag:
        raise ValueError(f"{who}: the device reported error word {flag}")


def rings_from_padded(vertices: Tensor, counts: Tensor) -> Tuple[Tensor, Tensor]:
    """``(ring_offsets, xy)`` from padded rings: ``vertices`` ``[P, L, 2]`` of which row ``p`` uses its first
    ``counts[p]`` entries (Xenium's boundaries are fixed 13- or 25-vertex rings).  Plain torch on the tensors' device."""
    if vertices.dim() != 3 or vertices.shape[2] != 2 or counts.dim() != 1 or counts.numel() != vertices.shape[0]:
        raise ValueError("rings_from_padded: vertices is [P, L, 2] and counts [P]")
    counts = counts.to(torch.int64)
    if counts.numel() and (int(counts.min()) < 0 or int(counts.max()) > vertices.shape[1]):
        raise ValueError("rings_from_padded: counts outside 0 .. L")
    ring_offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=vertices.device)
    torch.cumsum(counts, 0, out=ring_offsets[1:])
    used = torch.arange(vertices.shape[1], device=vertices.device)[None, :] < counts[:, None]
    return ring_offsets, vertices[used]
