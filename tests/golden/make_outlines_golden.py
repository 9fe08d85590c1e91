"""Writes tests/golden/outlines_small.npz from a RUN of the reference's ``_CellOutline`` (src/segger/export/boundary.py).

    python tests/golden/make_outlines_golden.py /path/to/reference/src/segger/export/boundary.py

``_CellOutline.__init__`` and ``refine`` need only numpy and scipy; the module's other imports (geopandas, pandas, polars,
shapely, tqdm) may be absent, so empty stand-in modules are put into ``sys.modules`` for those that cannot be imported.
``polygon()`` needs shapely and is NOT run: what is recorded per cell and connectivity is ``d_max`` and the edges that
``refine`` leaves with fewer than two triangles (``len(tri) < 2``), as pairs of indices into the cell's points in
``tri.points`` order.  tests/test_outlines_oracle.py requires the oracle's ring to be the closed cycle of largest area
among those edges, which pins the pruning to the reference; only ``polygonize`` stays restated.

The cells are the small ones of tests/outline_cases.py (every cell of ``cells()`` with at least 3 distinct points that are
not collinear -- qhull raises for the others, and the reference returns None before it gets there).  Only data is written.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import outline_cases as oc  # noqa: E402


def load_reference(path: str):
    for name in ("geopandas", "pandas", "polars", "shapely", "shapely.geometry", "shapely.ops", "tqdm"):
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            for attr in ("LineString", "MultiPoint", "Polygon", "polygonize", "tqdm", "DataFrame", "GeoDataFrame"):
                setattr(mod, attr, None)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_boundary", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(path: str) -> None:
    ref = load_reference(path)
    out = {"connectivities": np.array(oc.CONNECTIVITIES)}
    ids = []
    for c, pts in sorted(oc.cells().items()):
        if oc.State(pts).simplices is None:
            continue
        ids.append(c)
        out[f"points_{c}"] = np.asarray(pts, dtype=np.float64)
        for k, conn in enumerate(oc.CONNECTIVITIES):
            o = ref._CellOutline(np.asarray(pts, dtype=np.float64)).refine(conn)
            rim = sorted((int(a), int(b)) for (a, b), info in o.edges.items() if len(info["tri"]) < 2)
            out[f"rim_{c}_{k}"] = np.array(rim, dtype=np.int64).reshape(-1, 2)
            out[f"d_max_{c}_{k}"] = np.float64(o.d_max)
    out["cell_ids"] = np.array(ids, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "outlines_small.npz"), **out)
    print("wrote", len(ids), "cells")


if __name__ == "__main__":
    main(sys.argv[1])
