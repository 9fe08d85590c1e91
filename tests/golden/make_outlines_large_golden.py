"""Writes tests/golden/outlines_large.npz: the canonical oracle's ring, area and triangle count for the two cells of
tests/outline_large_cases.py whose oracle is too slow in Python for a test (11 500 and 65 537 points: about 15 s together).  The points are not stored:
the test regenerates them from the seeds in the case module.  ``check_large`` asserts the conditions of exactness on the way.

    python tests/golden/make_outlines_large_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import outline_large_cases as lc  # noqa: E402


def main():
    out = {}
    for name in lc.GOLDEN_CASES:
        pts = getattr(lc, name + "_cell")()
        ring, area, triangles = lc.check_large(pts, 2.0)
        out[name + "_ring"], out[name + "_area"], out[name + "_triangles"] = ring, np.float64(area), np.int64(triangles)
        out[name + "_points"] = np.int64(len(pts))
        print(name, len(pts), "points", triangles, "triangles", len(ring), "ring vertices, area", area)
    np.savez_compressed(os.path.join(HERE, "outlines_large.npz"), **out)


if __name__ == "__main__":
    main()
