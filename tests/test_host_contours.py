"""Label contours without a GPU: the oracle of tests/contour_cases.py against rings written out by hand and against
independent geometric properties (raster round trip, Pick's area) on a seeded Voronoi scene; the C-ABI surface of
segger_label_contours (symbols, signatures, ABI version 32, the documented terms of the workspace size, rejections with
SEGGER_EINVAL and a message on fake pointers that are never dereferenced, an empty input returning 0 without a device); and
the refusals of the Python wrapper, raised before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import contour_cases as cc
from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i32, i64, u64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
PTRS = ("labels", "compartment", "ring_offsets", "xy_out", "label_ids", "n_pixels", "counters", "workspace")


# ---------------------------------------------------------------- the oracle ---
@pytest.mark.parametrize("name", cc.HAND_ORDER)
def test_oracle_gives_the_ring_worked_by_hand(name):
    rows, ring = cc.HAND[name]
    img = np.zeros((len(rows) + 2, len(rows[0]) + 3), np.int32)     # a frame, H != W
    cc.place(img, cc.art(rows), 4, 2, 1)
    got = cc.label_rings(img)[4]["ring"]
    assert got == (None if ring is None else [(x + 2, y + 1) for x, y in ring])
    assert cc.label_rings(img)[4]["n_pixels"] == len(cc.art(rows))


def test_oracle_hand_details():
    res = cc.label_rings(cc.hand_image()[0])
    by = dict(zip(cc.HAND_ORDER, (res[k + 1] for k in range(len(cc.HAND_ORDER)))))
    assert by["ring3"]["n_borders"] == 2 and by["ring3"]["tie"]     # outer and hole border, 4 points each
    assert all(by[n]["n_borders"] == 1 and not by[n]["tie"] for n in cc.HAND_ORDER if n != "ring3")
    assert len(by["line5"]["chain"]) == 8                            # the pixels of a spur appear twice in the chain
    single = np.zeros((3, 3), np.int32)
    single[1, 1] = 1
    e = cc.expected(single)
    assert e["counters"]["n_present"] == 1 and e["counters"]["n_dropped"] == 1 and e["counters"]["n_borders"] == 1
    img, want = cc.hand_image()
    e = cc.expected(img)
    assert e["label_ids"].tolist() == [k for k in sorted(want) if want[k] is not None]
    assert e["counters"]["n_ties"] == 1 and e["counters"]["longest_ring"] == 4 and e["counters"]["n_dropped"] == 3


def test_oracle_edge_cases_have_what_their_names_say():
    c = cc.edge_cases()
    r = cc.label_rings(c["hole_outnumbers_outer"])[4]
    assert r["n_borders"] == 2 and len(r["ring"]) > 4
    r = cc.label_rings(c["two_components"])[1]
    assert r["n_borders"] == 2 and len(r["ring"]) == 6
    assert len(cc.label_rings(c["spiral_64"])[1]["chain"]) > 64
    assert len(cc.label_rings(c["spiral_4096"])[1]["chain"]) > 4096
    assert cc.label_rings(c["fills_the_image"])[2]["ring"] == [(0, 0), (4, 0), (4, 6), (0, 6)]
    q = c["candidate_queue_boundaries"]
    assert [int(((q == k + 1) & (np.roll(q, 1, 0) != k + 1)).sum()) for k in range(6)] == [63, 64, 65, 127, 128, 129]
    assert len(cc.label_rings(cc.long_ring())[9]["ring"]) > cc.MORPH_MAX_VERTS


def test_oracle_has_the_independent_properties_on_a_voronoi_scene():
    img = cc.voronoi_small()
    res = cc.label_rings(img)
    ok = cc.admitted(img, res)
    assert len(res) >= 30 and len(res) - len(ok) <= 0.10 * len(res), (len(res), len(ok))
    for lab in ok:
        ring = res[lab]["ring"]
        inside, strict = cc.raster(ring)
        ys, xs = np.nonzero(img == lab)
        assert len(strict) == len(inside) - cc.boundary_lattice_points(ring), lab
        assert inside == set(zip(xs.tolist(), ys.tolist())), lab     # the raster round trip
        B = cc.boundary_lattice_points(ring)
        I = len(inside) - B
        assert cc.shoelace2(ring) == 2 * I + B - 2, lab              # Pick: A = I + B / 2 - 1


def test_oracle_mask_and_affine():
    img, _ = cc.hand_image()
    comp = np.full(img.shape, 2, np.uint8)
    comp[img == 2] = 0
    comp[:, 27] = 1                                                  # cuts the plus in two
    a, b = cc.expected(img, comp, (2, 3)), cc.expected(np.where(np.isin(comp, (2, 3)), img, 0))
    assert all(np.array_equal(a[k], b[k]) for k in ("ring_offsets", "xy", "label_ids", "n_pixels"))
    assert 2 not in a["label_ids"]
    t = cc.expected(img, scale=(1.0, -1.0), translation=(100.5, 7.25))
    assert np.array_equal(t["xy"], cc.expected(img)["xy"] * np.array([1.0, -1.0]) + np.array([100.5, 7.25]))


# ---------------------------------------------------------------- the C ABI ---
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, H=10, W=12, max_label=5, valid=(0, 0, 0, 0), scale=(1.0, 1.0), trans=(0.0, 0.0), capacity=100, ws_bytes=1 << 24,
         lds_max=32768, **p):
    a = {name: FAKE for name in PTRS}
    a.update(p)
    return lib.segger_label_contours(a["labels"], a["compartment"], valid[0], valid[1], valid[2], valid[3], H, W, max_label, scale[0],
                                     scale[1], trans[0], trans[1], a["ring_offsets"], a["xy_out"], capacity, a["label_ids"],
                                     a["n_pixels"], a["counters"], a["workspace"], ws_bytes, lds_max, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_label_contours_workspace_bytes": (C.c_int64, [i64, i64, i64]),
            "segger_label_contours": (C.c_int, [vp, vp, u64, u64, u64, u64, i64, i64, i64, f64, f64, f64, f64, vp, vp, i64, vp, vp, vp,
                                                vp, i64, i32, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION                  # purely additive
    assert (_lib.CONTOUR_MAX_LABEL, _lib.CONTOUR_LDS_BITS, _lib.CONTOUR_COUNTERS) == (1 << 24, 32768, 10)
    import segger_amd
    from segger_amd import contours
    assert segger_amd.label_contours is contours.label_contours and len(contours.COUNTER_NAMES) == _lib.CONTOUR_COUNTERS


def test_workspace_size_has_the_documented_terms(lib):
    def up(x):
        return (x + 255) // 256 * 256
    size = lib.segger_label_contours_workspace_bytes
    for H, W, m in ((1, 1, 1), (10, 12, 5), (96, 96, 40), (7, 9, 65537), (4096, 4096, 20000), (3, 3, 1 << 24)):
        c = max(min(m, H * W), 1)
        fixed = 5 * up(4 * (m + 1)) + 6 * up(4 * c)
        got = size(H, W, m)
        assert fixed < got <= fixed + up(4 * (m + 1)) + (1 << 20), (H, W, m)   # the rest is the compaction's storage
    assert size(0, 0, 0) > 0
    for H, W, m in ((-1, 1, 1), (1, -1, 1), (1 << 16, 1 << 15, 1), (1, 1 << 31, 1), (4, 4, -1), (4, 4, (1 << 24) + 1)):
        assert size(H, W, m) == EINVAL, (H, W, m)
    assert size(1 << 16, 1 << 15, 1) == EINVAL and b"2^31" in lib.segger_last_error()
    assert size(4, 4, (1 << 24) + 1) == EINVAL and b"max_label" in lib.segger_last_error()


def test_rejections(lib):
    err = lib.segger_last_error
    assert call(lib, H=-1) == EINVAL and b"negative height" in err()
    assert call(lib, H=1 << 16, W=1 << 15) == EINVAL and b"2^31" in err()
    for m in (-1, (1 << 24) + 1):
        assert call(lib, max_label=m) == EINVAL and b"max_label" in err(), m
    for b in (-1, 32769):
        assert call(lib, lds_max=b) == EINVAL and b"lds_max_bits" in err(), b
    for bad in (float("inf"), float("nan")):
        assert call(lib, scale=(bad, 1.0)) == EINVAL and b"finite" in err()
        assert call(lib, trans=(0.0, bad)) == EINVAL and b"finite" in err()
    assert call(lib, ws_bytes=-1) == EINVAL and b"negative" in err()
    assert call(lib, capacity=-1) == EINVAL and b"negative" in err()
    for name in PTRS:
        if name not in ("compartment", "xy_out"):
            assert call(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
    assert call(lib, xy_out=None) == EINVAL and b"xy_out" in err()
    assert call(lib, compartment=None, ws_bytes=0) == EINVAL and b"workspace" in err()   # may be NULL: the next check fires
    assert call(lib, xy_out=FAKE + 8) == EINVAL and b"16-byte aligned" in err()
    for name in ("ring_offsets", "n_pixels", "counters"):
        assert call(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("labels", "label_ids"):
        assert call(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in err(), name
    assert call(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
    need = lib.segger_label_contours_workspace_bytes(10, 12, 5)
    assert call(lib, ws_bytes=need - 1) == EINVAL and str(need).encode() in err()


def test_empty_input_returns_ok_without_a_device(lib):
    none = dict(labels=None, compartment=None, xy_out=None, label_ids=None, n_pixels=None, workspace=None)
    assert call(lib, H=0, W=7, capacity=0, ws_bytes=0, **none) == 0
    assert call(lib, H=5, W=0, capacity=0, ws_bytes=0, **none) == 0
    assert call(lib, max_label=0, capacity=0, ws_bytes=0, **none) == 0       # nothing but background can be in it
    assert call(lib, H=0, counters=None) == EINVAL


# ---------------------------------------------------------------- the wrapper ---
def test_python_side_refusals():
    from segger_amd import label_contours
    lab = torch.zeros(4, 5, dtype=torch.int32)
    comp = torch.zeros(4, 5, dtype=torch.uint8)
    for bad in (lab.long(), lab.float(), lab[0], lab[None], lab.numpy(), None):
        with pytest.raises(ValueError, match="labels"):
            label_contours(bad)
    with pytest.raises(ValueError, match="come together"):
        label_contours(lab, comp)
    with pytest.raises(ValueError, match="come together"):
        label_contours(lab, valid_codes=(1,))
    for bad in (comp.int(), comp[0], comp.bool()):
        with pytest.raises(ValueError, match="compartment"):
            label_contours(lab, bad, (1,))
    with pytest.raises(ValueError, match="differ in shape"):
        label_contours(lab, torch.zeros(5, 4, dtype=torch.uint8), (1,))
    for bad in ((256,), (-1,), (1.0,), (True,), 3):
        with pytest.raises(ValueError, match="valid_codes"):
            label_contours(lab, comp, bad)
    for bad in ((1.0,), (1.0, float("inf")), "ab", 2.0):
        with pytest.raises(ValueError, match="scale"):
            label_contours(lab, scale=bad)
        with pytest.raises(ValueError, match="translation"):
            label_contours(lab, translation=bad)
    for bad in (-1, 32769, 1.0, True, "0"):
        with pytest.raises(ValueError, match="_lds_max_bits"):
            label_contours(lab, _lds_max_bits=bad)
    with pytest.raises(ValueError, match="2\\^31"):                  # a view: no memory behind it
        label_contours(torch.zeros(1, 1, dtype=torch.int32).expand(1 << 16, 1 << 15))
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):    # as the rest of the product: no CPU fallback
        label_contours(lab)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        label_contours(lab, comp, (1, 2))
