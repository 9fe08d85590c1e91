#!/usr/bin/env python
"""Writes tests/golden/morphology_small.npz: the non-degenerate named rings of tests/morphology_cases.py (the ring of
SEGGER_MORPH_MAX_VERTS vertices left out) as one CSR, with what ``scipy.spatial.ConvexHull`` says about each of them --
its hull area (``.volume`` in 2-D) and its hull vertices (``.vertices``, as a CSR of indices into the ring) -- so that a
machine without scipy can replay scipy's numbers.  Data only.  Run from the repository root:

    python tests/golden/make_morphology_golden.py
"""
import os
import sys

import numpy as np
from scipy.spatial import ConvexHull

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import morphology_cases as mc  # noqa: E402


def main() -> None:
    picked = [(name, ring) for name, ring in mc.cases() if name in mc.NON_DEGENERATE and not name.startswith("star_max")]
    offsets, xy = mc.to_csr([ring for _, ring in picked])
    areas, vertices = [], []
    for _, ring in picked:
        hull = ConvexHull(mc.open_ring(ring))
        areas.append(hull.volume)
        vertices.append(np.sort(hull.vertices).astype(np.int64))
    hull_offsets = np.zeros(len(picked) + 1, dtype=np.int64)
    hull_offsets[1:] = np.cumsum([len(v) for v in vertices])
    out = os.path.join(HERE, "morphology_small.npz")
    np.savez_compressed(out, names=np.array([name for name, _ in picked]), ring_offsets=offsets, xy=xy,
                        scipy_hull_area=np.array(areas), scipy_hull_offsets=hull_offsets,
                        scipy_hull_vertices=np.concatenate(vertices))
    print(out, os.path.getsize(out), "bytes,", len(picked), "rings")


if __name__ == "__main__":
    main()
