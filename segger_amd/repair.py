"""Ring repair on the device: what every boundary intake of the reference ends in, ``fix_invalid_geometry``
(``src/segger/io/utils.py:127-159``; called at ``io/preprocessor.py:311``, ``:316`` and ``:472``)::

    invalid = ~gdf.geometry.is_valid
    gdf.loc[invalid, "geometry"] = gdf.loc[invalid, "geometry"].apply(resort_coordinates)   # by arctan2 around the mean
    invalid = ~gdf.geometry.is_valid                                                        # and only then buffer(0)

on the project's ring CSR, between :func:`segger_amd.rings_simple` (the ``is_valid`` of a single-shell ring) and the ring
consumers (``polygon_props``, ``morphology_features``, ``points_in_polygons``, ``polygon_overlaps``), for all of which an
invalid ring gives wrong signed areas, wrong point-in-polygon answers and wrong overlap areas.

:func:`resort_rings` is ``resort_coordinates`` (``io/utils.py:83-102``) for the rings a mask selects: the vertices re-sorted
by the EXACT angle of their rounded float64 differences from the mean of the closed coordinate sequence, ties by exact
squared length, then by input index (include/segger_amd.h has the contract, DESIGN 3.5o the reasoning, csrc/repair.hip the
kernels).  :func:`repair_rings` is the whole of ``fix_invalid_geometry`` up to its fallback: check, re-sort the invalid
rings, check those again.  Both are checked for equality against a sequential oracle in exact rationals
(tests/repair_cases.py).

UNPINNED: numpy's own order among vertices whose float64 ``arctan2`` values tie or invert by rounding -- ``np.argsort`` is
not stable there, so the reference's order among such vertices is an accident of its sort; the exact order is this
project's contract.  Where all angular gaps exceed the rounding the two agree (tests/test_repair_oracle.py).

NOT BUILT: the ``buffer(0)`` fallback with its largest-component rule (GEOS's answer on a self-crossing ring depends on
winding, and neither shapely nor GEOS could be run where this was written) -- a ring that is still invalid after the
re-sort is reported, kept or dropped, never rebuilt; holes and multi-part polygons; rings above
``SEGGER_MORPH_MAX_VERTS`` (refused, naming the polygon)."""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L
from .rings import raise_ring_errors, ring_csr
from .simplify import _small_max, rings_simple

__all__ = ["resort_rings", "repair_rings", "COUNTER_NAMES", "STATUS_VALID", "STATUS_REPAIRED", "STATUS_INVALID"]

COUNTER_NAMES = ("n_invalid_in", "n_resorted", "n_still_invalid")
STATUS_VALID, STATUS_REPAIRED, STATUS_INVALID = 0, 1, 2
_HINT = "tests/repair_cases.py holds the CPU oracle"


def _own(given: Tensor, used: Tensor) -> Tensor:
    """the caller's tensor where the device code read it as it is"""
    return given if given.dtype == used.dtype and given.data_ptr() == used.data_ptr() and given.is_contiguous() else used


def _sub_csr(ring_offsets: Tensor, which: Tensor):
    """The CSR of the rings ``which`` (ascending int64 ids): its offsets and the rows of ``xy`` it takes, in order."""
    starts, counts = ring_offsets[:-1][which], (ring_offsets[1:] - ring_offsets[:-1])[which]
    off = torch.zeros(which.numel() + 1, dtype=torch.int64, device=ring_offsets.device)
    torch.cumsum(counts, 0, out=off[1:])
    ring_of = torch.repeat_interleave(torch.arange(which.numel(), device=off.device), counts)
    rows = torch.arange(ring_of.numel(), device=off.device) - off[ring_of] + starts[ring_of]
    return off, rows


def resort_rings(ring_offsets: Tensor, xy: Tensor, select: Optional[Tensor] = None, *, _route: Optional[str] = None) -> Dict[str, Tensor]:
    """Re-sort the vertices of the selected rings of a CSR (``ring_offsets`` ``[P + 1]``, ``xy`` ``[V, 2]`` on the device, as
    ``rings_simple`` takes them) by angle around their centre, as the reference's ``resort_coordinates`` does per polygon.

    ``select`` is a ``[P]`` bool or uint8 tensor on the same device (non-zero: re-sort this ring) or ``None`` for all.

    Returns ``xy`` ``[V, 2]`` float64 -- the input's bytes, permuted inside the selected rings and copied through
    elsewhere -- and ``vertex_index`` ``[V]`` int64, the input row of each output row.  A ring keeps its vertex count:
    ``ring_offsets`` is the caller's.

    The order within a selected ring of ``n >= 3`` open vertices: ascending exact angle in ``(-pi, pi]`` of
    ``d_k = (fl(x_k - c_x), fl(y_k - c_y))`` around ``c = (sum v_k + v_0) / (n + 1)`` (the reference sorts the closed
    sequence, so vertex 0 counts twice; the sum runs in the one order the header states), ``d = (0, 0)`` at angle 0, the
    negative x ray at ``+pi`` and last; ties by ascending exact squared length, then by input index.  The result is
    counter-clockwise around ``c``.  The comparison is exact -- neither a float ``atan2`` key nor a float cross product.
    A ring of fewer than 3 open vertices passes through; a ring given with a closing duplicate keeps it next to its twin.

    ``_route`` (tests and timing only): ``"large"`` sends every ring through the 4096-vertex LDS tier; the bytes are the same.

    With ``select`` all false nothing is launched and ``xy`` is the input.  Waits for the device (the longest ring, the mask,
    the error word).  Raises ``ValueError`` for bad shapes or dtypes, a ring above ``SEGGER_MORPH_MAX_VERTS`` (naming the
    polygon) or offsets the device found out of range, and ``SeggerAmdError`` for CPU tensors: there is no CPU fallback."""
    who = "resort_rings"
    small_max = _small_max(who, _route)
    given = xy
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    if select is not None:
        if not isinstance(select, Tensor) or select.dtype not in (torch.bool, torch.uint8) or select.dim() != 1 or \
                select.numel() != n_polygons:
            raise ValueError(f"{who}: select is a bool or uint8 [n_polygons] tensor ({n_polygons} polygons) or None")
        if select.device != xy.device:
            raise ValueError(f"{who}: select and xy are on different devices")
    L.need_device(who, ring_offsets, xy, hint=_HINT)
    dev = xy.device
    if n_polygons == 0 or n_vertices == 0 or (select is not None and not bool(select.any())):
        return {"xy": _own(given, xy), "vertex_index": torch.arange(n_vertices, dtype=torch.int64, device=dev)}
    if select is not None:
        select = select.detach().to(torch.uint8).contiguous()
    xy_out = torch.empty_like(xy)
    vertex_index = torch.empty(n_vertices, dtype=torch.int64, device=dev)
    ws, ws_bytes = L.workspace("segger_simplify_rings_workspace_bytes", dev, n_polygons, 0)
    L.call("segger_rings_resort", dev, ring_offsets.data_ptr(), xy.data_ptr(), n_polygons, n_vertices, L.ptr(select), xy_out.data_ptr(),
           vertex_index.data_ptr(), small_max, ws.data_ptr(), ws_bytes)
    raise_ring_errors(who, int(ws[:4].view(torch.int32)), ring_offsets, n_vertices)
    return {"xy": xy_out, "vertex_index": vertex_index}


def repair_rings(ring_offsets: Tensor, xy: Tensor, on_failure: str = "raise") -> Dict[str, Tensor]:
    """The reference's ``fix_invalid_geometry`` on a ring CSR, up to its ``buffer(0)`` fallback: :func:`rings_simple` on
    every ring, :func:`resort_rings` of the invalid ones, :func:`rings_simple` of those again.

    Returns ``ring_offsets`` and ``xy`` (the repaired CSR), ``vertex_index`` (the row of the input ``xy`` behind each row
    of the result), ``status`` ``[P]`` int8 (0 valid as given, 1 repaired by the re-sort, 2 still invalid),
    ``reason_before`` and ``reason_after`` (``[P, 3]`` int32, ``rings_simple``'s ``(code, i, j)`` before and after the
    re-sort; equal for the rings that were valid) and ``counters`` (int64, :data:`COUNTER_NAMES`: rings invalid as given,
    of those the rings the re-sort repaired, and the rings still invalid).

    ``on_failure`` decides about the rings that are still invalid -- where the reference goes on to ``buffer(0)``, which is
    NOT BUILT: ``"raise"`` (default) raises ``ValueError`` naming the first such polygon and its reason; ``"keep"`` returns
    them re-sorted with ``status`` 2; ``"drop"`` compacts them out of ``ring_offsets``, ``xy`` and ``vertex_index`` and adds
    ``kept`` ``[P']`` int64, the input polygon of each remaining ring (``status`` and the reasons stay ``[P]``).  A ring of
    fewer than 3 distinct vertices is invalid before and after.

    With no invalid ring no sort kernel is launched and ``xy`` is the input tensor.  Waits for the device.  Raises as
    :func:`resort_rings` does."""
    who = "repair_rings"
    if on_failure not in ("raise", "keep", "drop"):
        raise ValueError(f"{who}: on_failure is 'raise', 'keep' or 'drop', got {on_failure!r}")
    given = xy
    ring_offsets, xy, n_polygons, n_vertices = ring_csr(who, ring_offsets, xy)
    L.need_device(who, ring_offsets, xy, hint=_HINT)
    dev = xy.device
    ok, reason_before = rings_simple(ring_offsets, xy)
    bad = ~ok
    n_invalid = int(bad.sum())
    status = torch.zeros(n_polygons, dtype=torch.int8, device=dev)
    out = {"ring_offsets": ring_offsets, "xy": _own(given, xy), "status": status, "reason_before": reason_before, "reason_after": reason_before}
    n_still = 0
    if n_invalid == 0:
        out["vertex_index"] = torch.arange(n_vertices, dtype=torch.int64, device=dev)
    else:
        r = resort_rings(ring_offsets, xy, bad)
        out["xy"], out["vertex_index"] = r["xy"], r["vertex_index"]
        which = bad.nonzero().reshape(-1)
        sub_off, rows = _sub_csr(ring_offsets, which)                # only the re-sorted rings are checked again
        ok_sub, reason_sub = rings_simple(sub_off, r["xy"][rows])
        out["reason_after"] = reason_before.clone()
        out["reason_after"][which] = reason_sub
        status[which] = torch.where(ok_sub, STATUS_REPAIRED, STATUS_INVALID).to(torch.int8)
        n_still = int((~ok_sub).sum())
    out["counters"] = torch.tensor([n_invalid, n_invalid - n_still, n_still], dtype=torch.int64, device=dev)
    if n_still and on_failure == "raise":
        p = int((status == STATUS_INVALID).nonzero()[0])
        code, i, j = out["reason_after"][p].tolist()
        why = "fewer than 3 distinct vertices" if code == L.RING_TOO_FEW else f"edges {i} and {j} touch"
        raise ValueError(f"{who}: polygon {p} is still invalid after the re-sort ({why}); {n_still} of {n_polygons} are, and the "
                         f"reference's buffer(0) fallback is not built -- pass on_failure='keep' or 'drop'")
    if on_failure == "drop":
        kept = (status != STATUS_INVALID).nonzero().reshape(-1)
        if n_still:
            out["ring_offsets"], rows = _sub_csr(ring_offsets, kept)
            out["xy"], out["vertex_index"] = out["xy"][rows], out["vertex_index"][rows]
        out["kept"] = kept
    return out
