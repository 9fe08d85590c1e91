"""Writes tests/golden/boundaries_small.npz: a small segmentation (``xy``, ``cell``, ``n_cells``) and, for every cell
Qhull accepts, what ``scipy.spatial.ConvexHull`` returns for it -- the hull's vertex indices into ``xy`` (a CSR over the
cells in ``scipy_cell_ids``) and its area.  tests/test_gpu_boundaries.py requires the device's rings to have exactly these
vertex sets and areas.

PINNED TO SCIPY ONLY.  The reference's own ``cell_boundary`` / ``_chaikin`` (src/segger/export/boundary.py) need geopandas,
shapely and polars at import; none of them could be imported where this file was written, so no output of the reference
is recorded here.  The smoothing is checked against numpy's iteration of the reference's formula instead
(tests/boundaries_cases.py: chaikin).

Run from the repository root:  python tests/golden/make_boundaries_golden.py
"""
import os
import sys

import numpy as np
from scipy.spatial import ConvexHull, QhullError

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import boundaries_cases as bc  # noqa: E402


def main() -> None:
    for name in ("geopandas", "shapely", "polars"):
        try:
            __import__(name)
            print(f"note: {name} imports here; the reference's cell_boundary could be recorded too")
        except ImportError:
            pass
    cells = {c: p for c, p in bc.scene_cells().items() if len(p) <= 100}
    xy = np.concatenate(list(cells.values()))
    ids = np.concatenate([np.full(len(p), c, dtype=np.int32) for c, p in cells.items()])
    perm = np.random.default_rng(0).permutation(len(ids))
    xy, ids = np.ascontiguousarray(xy[perm]), ids[perm]
    kept, verts, areas = [], [], []
    for c in sorted(cells):
        rows = np.flatnonzero(ids == c)
        try:
            qh = ConvexHull(xy[rows])
        except (QhullError, ValueError):                             # collinear, duplicate or too few points
            continue
        kept.append(c)
        verts.append(rows[qh.vertices])
        areas.append(qh.volume)                                      # in two dimensions Qhull's "volume" is the area
    offsets = np.zeros(len(kept) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(v) for v in verts])
    path = os.path.join(HERE, "boundaries_small.npz")
    np.savez_compressed(path, xy=xy, cell=ids, n_cells=np.int64(bc.N_CELLS), scipy_cell_ids=np.array(kept, dtype=np.int32),
                        scipy_hull_offsets=offsets, scipy_hull_vertices=np.concatenate(verts).astype(np.int64),
                        scipy_hull_area=np.array(areas, dtype=np.float64))
    print(path, os.path.getsize(path), "bytes;", len(kept), "cells with a hull of", len(cells))


if __name__ == "__main__":
    main()
