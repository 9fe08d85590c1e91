"""Boundary polygons from label images on the device: the intake CosMx needs, whose boundaries are label images and not
vertex lists.  The reference turns them into polygons on the CPU, one label at a time (``masks_to_contours``,
``src/segger/io/utils.py:8-41``, driven by ``src/segger/io/cosmx.py:79-107``): a ``regionprops`` crop, ``cv2.findContours(...,
RETR_LIST, CHAIN_APPROX_SIMPLE)``, the contour with the most vertices, dropped with <= 2.  :func:`label_contours` does the
same for every label of an image in one call (csrc/contours.hip) and returns the project's ring CSR, which goes into
``polygon_props``, ``morphology_features`` and ``points_in_polygons`` as it is.

The result is defined exactly (include/segger_amd.h) and checked against a sequential Suzuki-Abe oracle
written from that definition plus independent properties (raster round trip, Pick's area).  UNPINNED: neither ``cv2`` nor
``skimage`` could be run, so cv2's start vertex, orientation and order among borders of equal length are supposed, not
checked; downstream code accepts any start and either orientation.

The step the reference takes next, ``simplify(tolerance)`` followed by ``is_valid``, is :mod:`segger_amd.simplify`
(``simplify_rings``, ``contour_tolerance``, ``rings_simple``); the re-sort of ``fix_invalid_geometry`` is
:mod:`segger_amd.repair`.  NOT BUILT: TIFF reading, the ``buffer(0)`` repair of ``fix_invalid_geometry``, the id strings,
FOV stitching."""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L

__all__ = ["label_contours", "COUNTER_NAMES"]

COUNTER_NAMES = ("n_present", "n_kept", "n_vertices", "n_dropped", "n_borders", "longest_ring", "n_ties", "n_bad_label", "overflow",
                 "n_global")
MAX_PIXELS = (1 << 31) - 1


def _pair(who: str, name: str, v) -> Sequence[float]:
    try:
        a, b = (float(t) for t in v)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} is a pair of finite numbers, got {v!r}") from None
    if not (abs(a) < float("inf") and abs(b) < float("inf")):
        raise ValueError(f"{who}: {name} is a pair of finite numbers, got {v!r}")
    return a, b


def _code_words(who: str, valid_codes: Iterable[int]):
    words = [0, 0, 0, 0]
    try:
        codes = [c for c in valid_codes]
    except TypeError:
        raise ValueError(f"{who}: valid_codes is a collection of ints in 0 .. 255, got {valid_codes!r}") from None
    for c in codes:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 255:
            raise ValueError(f"{who}: valid_codes is a collection of ints in 0 .. 255, got {c!r}")
        words[c >> 6] |= 1 << (c & 63)
    return words


def _empty(dev, counters: Tensor) -> Dict[str, Tensor]:
    return {"ring_offsets": torch.zeros(1, dtype=torch.int64, device=dev), "xy": torch.empty(0, 2, dtype=torch.float64, device=dev),
            "label_ids": torch.empty(0, dtype=torch.int32, device=dev), "n_pixels": torch.empty(0, dtype=torch.int64, device=dev),
            "counters": counters}


def label_contours(labels: Tensor, compartment: Optional[Tensor] = None, valid_codes: Optional[Iterable[int]] = None, *,
                   scale=(1.0, 1.0), translation=(0.0, 0.0), _lds_max_bits: Optional[int] = None) -> Dict[str, Tensor]:
    """One polygon per label of a label image: the border of the label with the most vertices.

    ``labels`` is ``[H, W]`` int32 on the device, row = y, column = x, 0 = background, ids >= 0 and at most
    ``SEGGER_CONTOUR_MAX_LABEL`` = 2^24 (they size five int32 tables; sparse ids are fine), ``H * W < 2^31``.  With
    ``compartment`` (``[H, W]`` uint8) and ``valid_codes`` (ints in 0 .. 255) a pixel counts as its label only if its
    compartment code is among the codes -- ``np.where(np.isin(compartment, codes), labels, 0)`` fused into the read.  Both
    or neither.  Which codes mean "nucleus" or "membrane" is the caller's knowledge: pass them.

    Returns ``ring_offsets`` ``[P + 1]`` int64, ``xy`` ``[V, 2]`` float64, ``label_ids`` ``[P]`` int32 ascending, ``n_pixels``
    ``[P]`` int64 (the masked pixel count of each kept label) and ``counters`` (int64, :data:`COUNTER_NAMES`: labels
    present, kept, vertices, labels dropped for <= 2 points, borders traced, the longest ring, ties broken, ...).  A vertex
    is a pixel's integer ``(x, y)``, exact in float64, then ``xy * scale + translation`` (the reference's
    ``scale=(1, -1)`` and FOV position; one multiplication and one addition, not fused).  Rings are open.

    What a ring is: the foreground of a label is its pixels after the mask; its borders are those of Suzuki-Abe border
    following with 8-connected foreground, outer and hole borders of every component; the scan is x-major, as the
    reference's transposed crop makes cv2's; ``CHAIN_APPROX_SIMPLE`` keeps a chain point iff the step into it differs from
    the step out of it.  The border with the most kept points wins (a hole border can); equal counts: the one whose
    canonical start -- its first pixel in the scan -- comes first (UNPINNED, as is the start itself: cv2 was not run).  A
    label whose winner has <= 2 points is dropped.  A ring longer than ``SEGGER_MORPH_MAX_VERTS`` is still returned; the
    downstream units refuse it as documented there.  The same bytes from run to run.

    ``_lds_max_bits`` (tests and timing only) lowers the crop size up to which a label is traced in LDS; 0 sends every
    label over the image in global memory.  Two waits for the device (the largest label; the counters), a third call when
    the first guess of the vertex capacity was too small.

    Raises ``ValueError`` for wrong dtypes or shapes, ``compartment`` without ``valid_codes`` or the reverse, negative
    labels or bounds exceeded, and ``SeggerAmdError`` for CPU tensors (there is no CPU fallback), before anything is
    launched."""
    who = "label_contours"
    if not isinstance(labels, Tensor) or labels.dim() != 2 or labels.dtype != torch.int32:
        raise ValueError(f"{who}: labels is an int32 [H, W] tensor")
    if (compartment is None) != (valid_codes is None):
        raise ValueError(f"{who}: compartment and valid_codes come together or not at all")
    words = [0, 0, 0, 0]
    if compartment is not None:
        if not isinstance(compartment, Tensor) or compartment.dtype != torch.uint8 or compartment.dim() != 2:
            raise ValueError(f"{who}: compartment is a uint8 [H, W] tensor")
        if compartment.shape != labels.shape:
            raise ValueError(f"{who}: compartment {tuple(compartment.shape)} and labels {tuple(labels.shape)} differ in shape")
        if compartment.device != labels.device:
            raise ValueError(f"{who}: compartment and labels are on different devices")
        words = _code_words(who, valid_codes)
    sx, sy = _pair(who, "scale", scale)
    tx, ty = _pair(who, "translation", translation)
    if _lds_max_bits is None:
        _lds_max_bits = L.CONTOUR_LDS_BITS
    if isinstance(_lds_max_bits, bool) or not isinstance(_lds_max_bits, int) or not 0 <= _lds_max_bits <= L.CONTOUR_LDS_BITS:
        raise ValueError(f"{who}: _lds_max_bits must be an int in 0 .. {L.CONTOUR_LDS_BITS}, got {_lds_max_bits!r}")
    H, W = int(labels.shape[0]), int(labels.shape[1])
    if H * W > MAX_PIXELS:
        raise ValueError(f"{who}: H * W = {H * W} is 2^31 or more (pixel indices are 32-bit)")
    L.need_device(who, labels, compartment, hint="tests/contour_cases.py has the CPU oracle")
    dev = labels.device
    counters = torch.zeros(L.CONTOUR_COUNTERS, dtype=torch.int64, device=dev)
    if H * W == 0:
        return _empty(dev, counters)
    img = labels.detach().contiguous()
    comp = None if compartment is None else compartment.detach().contiguous()
    lo, hi = (int(v) for v in torch.aminmax(img))                    # a wait for the device
    if lo < 0:
        raise ValueError(f"{who}: labels must be >= 0, the smallest is {lo}")
    if hi > L.CONTOUR_MAX_LABEL:
        raise ValueError(f"{who}: the largest label {hi} exceeds SEGGER_CONTOUR_MAX_LABEL = {L.CONTOUR_MAX_LABEL} "
                         f"(tables are sized by it); relabel the image")
    if hi == 0:
        return _empty(dev, counters)
    cap = max(min(hi, H * W), 1)
    ring_offsets = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    label_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    n_pixels = torch.empty(cap, dtype=torch.int64, device=dev)
    ws, ws_bytes = L.workspace("segger_label_contours_workspace_bytes", dev, H, W, hi)
    capacity = max(H * W // 8, 4096)                                 # a guess; the counters say what was needed
    while True:
        out = torch.empty(capacity, 2, dtype=torch.float64, device=dev)
        L.call("segger_label_contours", dev, img.data_ptr(), L.ptr(comp), words[0], words[1], words[2], words[3], H, W, hi, sx, sy,
               tx, ty, ring_offsets.data_ptr(), out.data_ptr(), capacity, label_ids.data_ptr(), n_pixels.data_ptr(),
               counters.data_ptr(), ws.data_ptr(), ws_bytes, _lds_max_bits)
        c = dict(zip(COUNTER_NAMES, counters.tolist()))              # the wait for the device
        if not c["overflow"]:
            break
        capacity = c["n_vertices"]                                   # the same rings again, this time with room
    del ws
    assert c["n_bad_label"] == 0, c                                  # aminmax said so
    K, V = c["n_kept"], c["n_vertices"]
    verts = out[:V]
    if 4 * V < capacity:                                             # do not keep the guess alive behind a small view
        verts = verts.clone()
    return {"ring_offsets": ring_offsets[:K + 1], "xy": verts, "label_ids": label_ids[:K], "n_pixels": n_pixels[:K],
            "counters": counters}
