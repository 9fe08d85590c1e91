"""segger_amd.label_contours on the MI355X against the sequential Suzuki-Abe oracle of tests/contour_cases.py: every returned
tensor equal, on the default route (bit mask in LDS) and again with every label forced over the image in global memory.
The kernel's own boundaries, each with a case below and above it (contour_cases.edge_cases): 64 candidates per drain of the
trace kernel's queue (63 / 64 / 65 and 127 / 128 / 129), the LDS route's 32768 padded bits (128 x 256 and 128 x 257), the
64-pixel staging chunk (64 and 65 columns) and the 32-bit mask word (32 and 33 columns), the offsets kernel's 1024 labels
per trip (1023 / 1024 / 1025), image widths that are no multiple of the wave."""
import numpy as np
import pytest
import torch

import contour_cases as cc
from segger_amd import _lib, label_contours, points_in_polygons, polygon_props
from segger_amd.contours import COUNTER_NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("ring_offsets", "xy", "label_ids", "n_pixels")
ROUTES = (None, 0)
EDGE = cc.edge_cases()


def run(img, comp=None, codes=None, **kw):
    out = label_contours(torch.as_tensor(img, device=DEV), None if comp is None else torch.as_tensor(comp, device=DEV), codes, **kw)
    assert out["ring_offsets"].dtype == torch.int64 and out["xy"].dtype == torch.float64 and out["xy"].shape[1:] == (2,)
    assert out["label_ids"].dtype == torch.int32 and out["n_pixels"].dtype == torch.int64
    got = {k: out[k].cpu().numpy() for k in KEYS}
    got["counters"] = dict(zip(COUNTER_NAMES, out["counters"].tolist()))
    return got


def check(img, comp=None, codes=None, want=None, **kw):
    """every tensor and every counter equal to the oracle's, on both routes -> the default route's result"""
    want = cc.expected(img, comp, codes, **kw) if want is None else want
    first = None
    for bits in ROUTES:
        got = run(img, comp, codes, _lds_max_bits=bits, **kw)
        for k in KEYS:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, bits)
        for k, v in want["counters"].items():
            assert got["counters"][k] == v, (k, bits, got["counters"])
        if bits == 0:
            assert got["counters"]["n_global"] == want["counters"]["n_present"]
        first = first or got
    return first


def test_hand_cases_in_one_image():
    img, rings = cc.hand_image()
    got = check(img)
    for k, lab in enumerate(got["label_ids"].tolist()):
        a, b = got["ring_offsets"][k:k + 2]
        assert [tuple(p) for p in got["xy"][a:b].tolist()] == [tuple(map(float, p)) for p in rings[lab]], lab
    assert got["label_ids"].tolist() == [1, 2, 3, 5] and got["counters"]["n_global"] == 0


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_cases(name):
    got = check(EDGE[name])
    if name == "lds_route_boundaries":
        assert got["counters"]["n_global"] == 1                      # the 128 x 257 crop alone
    if name == "sparse_ids":
        assert got["label_ids"].tolist() == [1, 7, 65537]


def test_a_ring_above_the_morphology_cap_is_emitted_and_refused_downstream():
    img = cc.long_ring()
    got = check(img)
    assert got["counters"]["longest_ring"] > _lib.MORPH_MAX_VERTS
    out = label_contours(torch.as_tensor(img, device=DEV))
    with pytest.raises(ValueError, match="SEGGER_MORPH_MAX_VERTS"):
        polygon_props(out["ring_offsets"], out["xy"])


def test_compartment_mask():
    img, _ = cc.hand_image()
    comp = np.full(img.shape, 2, np.uint8)
    comp[img == 2] = 0                                               # label 2 is masked away entirely
    comp[:, 27] = 200                                                # cuts the plus in two
    comp[0, 0] = 255
    codes = (2, 64, 255)
    got = check(img, comp, codes)
    pre = run(np.where(np.isin(comp, codes), img, 0).astype(np.int32))
    assert all(np.array_equal(got[k], pre[k]) for k in KEYS)
    assert 2 not in got["label_ids"].tolist() and got["counters"]["n_present"] == 6


def test_affine_is_applied_in_float64_on_the_write():
    img, _ = cc.hand_image()
    scale, trans = (1.0, -1.0), (1234.5678, 0.1)
    got = check(img, scale=scale, translation=trans)
    plain = cc.expected(img)["xy"]
    assert got["xy"].tobytes() == (plain * np.asarray(scale) + np.asarray(trans)).tobytes()


@pytest.fixture(scope="module", params=["small", "medium"])
def scene(request):
    img = cc.voronoi_small() if request.param == "small" else cc.voronoi_medium()
    want = cc.expected(img)
    return img, want, cc.admitted(img, want["by_label"])


def test_voronoi_scene_equals_the_oracle_and_flows_downstream(scene):
    img, want, ok = scene
    check(img, want=want)
    assert len(ok) >= 0.9 * len(want["by_label"])
    out = label_contours(torch.as_tensor(img, device=DEV))           # stays on the device from here on
    ids = out["label_ids"].tolist()
    area = polygon_props(out["ring_offsets"], out["xy"])["area"].cpu().numpy()
    pts, owner = [], []
    for lab in ok:
        ring = want["by_label"][lab]["ring"]
        closed, strict = cc.raster(ring)
        B = cc.boundary_lattice_points(ring)
        assert area[ids.index(lab)] == len(strict) + B / 2 - 1, lab  # Pick; exact in fp64 at these sizes
        pts += sorted(strict)
        owner += [ids.index(lab)] * len(strict)
    pairs = points_in_polygons(torch.tensor(pts, dtype=torch.float64, device=DEV), out["ring_offsets"], out["xy"]).cpu().numpy()
    admitted = np.isin(pairs[1], [ids.index(lab) for lab in ok])
    assert np.array_equal(pairs[:, admitted], np.stack([np.arange(len(pts)), np.asarray(owner)]))


def test_two_runs_give_equal_bytes_and_a_frame_only_shifts():
    img = cc.voronoi_small()
    a, b = run(img), run(img)
    assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS)
    framed = np.zeros((img.shape[0] + 10, img.shape[1] + 10), np.int32)
    framed[5:-5, 5:-5] = img
    c = run(framed)
    assert all(np.array_equal(a[k], c[k]) for k in ("ring_offsets", "label_ids", "n_pixels"))
    assert (c["xy"] - 5.0).tobytes() == a["xy"].tobytes()


def test_capacity_one_short_reports_overflow_and_writes_nothing_past_the_buffer():
    img, _ = cc.hand_image()
    want = cc.expected(img)
    H, W = img.shape
    V, hi = int(want["ring_offsets"][-1]), int(img.max())
    lab = torch.as_tensor(img, device=DEV)
    for capacity in (V - 1, V):
        guard = 64
        out = torch.full((capacity + guard, 2), -7.0, dtype=torch.float64, device=DEV)
        offs = torch.zeros(hi + 1, dtype=torch.int64, device=DEV)
        ids = torch.zeros(hi, dtype=torch.int32, device=DEV)
        npx = torch.zeros(hi, dtype=torch.int64, device=DEV)
        counters = torch.zeros(_lib.CONTOUR_COUNTERS, dtype=torch.int64, device=DEV)
        ws, ws_bytes = _lib.workspace("segger_label_contours_workspace_bytes", lab.device, H, W, hi)
        _lib.call("segger_label_contours", lab.device, lab.data_ptr(), None, 0, 0, 0, 0, H, W, hi, 1.0, 1.0, 0.0, 0.0, offs.data_ptr(),
                  out.data_ptr(), capacity, ids.data_ptr(), npx.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes,
                  _lib.CONTOUR_LDS_BITS)
        c = dict(zip(COUNTER_NAMES, counters.tolist()))
        assert c["overflow"] == (capacity < V) and c["n_vertices"] == V and c["n_kept"] == len(want["label_ids"])
        assert np.array_equal(offs[:c["n_kept"] + 1].cpu().numpy(), want["ring_offsets"])
        assert np.array_equal(out[:capacity].cpu().numpy(), want["xy"][:capacity])
        assert bool((out[capacity:] == -7.0).all())                  # the guard region


def test_all_background_and_wrapper_bounds():
    for img in (np.zeros((5, 7), np.int32), np.zeros((0, 4), np.int32)):
        out = label_contours(torch.as_tensor(img, device=DEV))
        assert out["ring_offsets"].tolist() == [0] and out["xy"].shape == (0, 2) and out["label_ids"].numel() == 0
        assert out["n_pixels"].numel() == 0 and out["counters"].tolist() == [0] * _lib.CONTOUR_COUNTERS
    comp = np.zeros((5, 7), np.uint8)
    img = np.ones((5, 7), np.int32)
    assert run(img, comp, (1,))["label_ids"].size == 0               # everything masked away: P == 0
    bad = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
    bad[1, 1] = -1
    with pytest.raises(ValueError, match=">= 0"):
        label_contours(bad)
    bad[1, 1] = (1 << 24) + 1
    with pytest.raises(ValueError, match="SEGGER_CONTOUR_MAX_LABEL"):
        label_contours(bad)
