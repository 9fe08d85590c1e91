"""segger_amd.rasterize_rings on the MI355X against the numpy oracle of tests/rasterize_cases.py (the join's float64
predicate over the pixel centres, pinned to the exact-rational one by tests/test_rasterize_cases.py): every tensor and
every pinned counter EQUAL, under both predicates and both overlap rules, with the default block, with the shortcut off
(``_block=1``) and with every ring forced through the LDS tier.  ``n_blocks_filled`` is the device's own diagnostic (it
depends on the block side): it is 0 with the shortcut off and positive where a large ring has an interior.

The kernel's own boundaries: rings of 3 / 64 / 65 / 4096 vertices (the register tier ends at 64, the LDS tier at 4096),
pixel ranges 1 / 63 / 64 / 65 wide (a wave takes 64 pixels or block centres a step) and block - 1 / block / block + 1 wide."""
import numpy as np
import pytest
import torch

import rasterize_cases as rc
from segger_amd import label_contours, points_in_polygons, rasterize_rings
from segger_amd.rasterize import COUNTER_NAMES, DEFAULT_BLOCK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = rc.cases(DEFAULT_BLOCK)
GEOMETRIES = (dict(), dict(_block=1), dict(_route="large"), dict(_block=4, _route="large"), dict(_block=32))


def to_device(rings):
    offs, xy = rc.mc.to_csr(rings)
    return torch.as_tensor(offs, device=DEV), torch.as_tensor(xy, device=DEV)


def run(rings, shape, labels=None, **kw):
    offs, xy = to_device(rings)
    out = rasterize_rings(offs, xy, shape, labels=None if labels is None else torch.as_tensor(labels, dtype=torch.int32, device=DEV), **kw)
    assert out["image"].dtype == torch.int32 and tuple(out["image"].shape) == tuple(shape)
    assert out["n_covered"].dtype == out["n_won"].dtype == out["counters"].dtype == torch.int64
    got = {k: out[k].cpu().numpy() for k in ("image", "n_covered", "n_won")}
    got["counters"] = dict(zip(COUNTER_NAMES, out["counters"].tolist()))
    return got


def assert_equal(got, want, what):
    for k in ("image", "n_covered", "n_won"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, what)
    for k, v in want["counters"].items():
        assert got["counters"][k] == v, (k, what, got["counters"])


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_equals_the_oracle_under_every_option_and_geometry(name):
    c = next(c for c in CASES if c["name"] == name)
    n_real = sum(len(rc.mc.open_ring(r)) >= 3 for r in c["rings"])
    for predicate in rc.PREDICATES:
        for overlap in rc.OVERLAPS:
            want = rc.expected(c, predicate, overlap, block=DEFAULT_BLOCK)
            for geometry in GEOMETRIES:
                got = run(c["rings"], c["shape"], c["labels"], scale=c["scale"], translation=c["translation"], predicate=predicate,
                          overlap=overlap, **geometry)
                forced = geometry.get("_route") == "large"              # then every ring of 3 or more vertices runs in LDS
                assert_equal(got, dict(want, counters=dict(want["counters"], n_large_tier=n_real)) if forced else want,
                             (predicate, overlap, geometry))
                if geometry.get("_block") == 1:
                    assert got["counters"]["n_blocks_filled"] == 0


@pytest.mark.parametrize("predicate", rc.PREDICATES)
def test_hand_worked_square_and_triangle(predicate):
    got = run([rc.HAND_SQUARE, rc.HAND_TRIANGLE], (8, 8), predicate=predicate)
    assert np.array_equal(got["image"], rc.hand_image(predicate))    # on-ring pixels differ between the two


def test_a_large_ring_is_mostly_filled_by_blocks():
    ring = [rc._rect(10.5, 10.5, 200.5, 150.5)]
    want = rc.resolve(rc.masks_f64(ring, (160, 256)), ring, (160, 256), (1.0, 1.0), (0.0, 0.0), None, "intersects", "lowest")
    for block in (4, 8, 16):
        got = run(ring, (160, 256), _block=block)
        assert_equal(got, want, block)
        inner = ((190 - 2 * block) // block - 1) * ((140 - 2 * block) // block - 1)           # aligned blocks a block away from every edge
        assert inner <= got["counters"]["n_blocks_filled"] <= (190 // block + 2) * (140 // block + 2), (block, got["counters"])


def test_blocks_fill_inside_a_4096_vertex_ring_the_same_from_run_to_run():
    """the shortcut fires on the LDS tier too: the star's radius is at least 16 pixels, so whole 8 x 8 blocks lie inside"""
    ring = [rc.mc.star_ring(4096, 11, 40.0) + [48.0, 48.0]]
    want = rc.resolve(rc.masks_f64(ring, (96, 96)), ring, (96, 96), (1.0, 1.0), (0.0, 0.0), None, "intersects", "lowest")
    runs = [run(ring, (96, 96)), run(ring, (96, 96)), run(ring, (96, 96), _route="large")]
    for got in runs:
        assert_equal(got, want, "ring4096 at radius 40")
    filled = [got["counters"]["n_blocks_filled"] for got in runs]
    assert filled[0] > 0 and filled[0] == filled[1] == filled[2], filled
    assert 64 * filled[0] <= want["counters"]["n_pixels_set"]


# ---------------------------------------------------------------- the 128 x 128 Voronoi scene ---
@pytest.fixture(scope="module")
def scene():
    img, want, ok = rc.scene()
    rings, labels = rc.rings_of(want)
    masks = rc.masks_f64(rings, img.shape)
    return img, want, ok, rings, labels, masks


def test_scene_bytes_do_not_depend_on_geometry_or_run_and_equal_the_oracle(scene):
    img, _, _, rings, labels, masks = scene
    for overlap in rc.OVERLAPS:
        want = rc.resolve(masks, rings, img.shape, (1.0, 1.0), (0.0, 0.0), labels, "intersects", overlap)
        first = run(rings, img.shape, labels, overlap=overlap)
        assert_equal(first, want, overlap)
        for geometry in (dict(), dict(_block=1), dict(_route="large")):
            again = run(rings, img.shape, labels, overlap=overlap, **geometry)
            for k in ("image", "n_covered", "n_won"):
                assert again[k].tobytes() == first[k].tobytes(), (k, geometry)
            assert [again["counters"][k] for k in COUNTER_NAMES[:5]] == [first["counters"][k] for k in COUNTER_NAMES[:5]]
            if "_block" not in geometry:                             # the shortcut fires, and the same way on either route and run
                assert again["counters"]["n_blocks_filled"] == first["counters"]["n_blocks_filled"] > 0, (geometry, again["counters"])


@pytest.mark.parametrize("predicate", rc.PREDICATES)
def test_scene_equals_the_composition_a_user_would_write(scene, predicate):
    """points_in_polygons over the full pixel-centre grid on the device, overlaps resolved by a sort in torch"""
    img, _, _, rings, labels, _ = scene
    H, W = img.shape
    offs, xy = to_device(rings)
    got = rasterize_rings(offs, xy, (H, W), labels=torch.as_tensor(labels, device=DEV), predicate=predicate)
    cols = torch.arange(W, dtype=torch.float64, device=DEV) * 1.0 + 0.0
    rows = torch.arange(H, dtype=torch.float64, device=DEV) * 1.0 + 0.0
    pts = torch.stack([cols.repeat(H), rows.repeat_interleave(W)], dim=1)
    pairs = points_in_polygons(pts, offs, xy, None, predicate)       # sorted by (point, polygon)
    first = torch.ones(pairs.shape[1], dtype=torch.bool, device=DEV)
    first[1:] = pairs[0, 1:] != pairs[0, :-1]                        # the lowest polygon of every pixel
    image = torch.zeros(H * W, dtype=torch.int32, device=DEV)
    image[pairs[0, first]] = torch.as_tensor(labels, device=DEV)[pairs[1, first]]
    assert torch.equal(got["image"], image.view(H, W))
    assert torch.equal(got["n_covered"], torch.bincount(pairs[1], minlength=len(rings)))
    assert int(got["counters"][0]) == int(first.sum()) and int(got["counters"][1]) == int((~first).sum())


def test_shuffled_polygons_with_their_labels(scene):
    """the scene's rings and six large stars across them, shuffled, ``labels`` carrying the original ids: overlaps are decided
    by polygon index, so the shuffle changes the image only where polygons overlap"""
    img, _, _, rings, labels, masks = scene
    stars = [rc.mc.star_ring(13 + 20 * k, 40 + k, 24.0) + [20.0 + 18.0 * k, 30.0 + 14.0 * k] for k in range(6)]
    rings, masks = rings + stars, masks + rc.masks_f64(stars, img.shape)
    labels = np.concatenate([labels, np.arange(1000, 1006, dtype=np.int32)])
    perm = np.random.default_rng(5).permutation(len(rings))
    s_rings, s_labels, s_masks = [rings[k] for k in perm], labels[perm], [masks[k] for k in perm]
    want = rc.resolve(s_masks, s_rings, img.shape, (1.0, 1.0), (0.0, 0.0), s_labels, "intersects", "lowest")
    got = run(s_rings, img.shape, s_labels)
    assert_equal(got, want, "shuffled")
    assert got["counters"]["n_overlaps"] > 1000
    plain = run(rings, img.shape, labels)
    assert_equal(plain, rc.resolve(masks, rings, img.shape, (1.0, 1.0), (0.0, 0.0), labels, "intersects", "lowest"), "plain")
    assert np.array_equal(got["n_covered"], plain["n_covered"][perm])
    total = np.zeros(img.size, np.int64)
    for m in masks:
        total[m["intersects"]] += 1
    alone = (total <= 1).reshape(img.shape)                          # the n_covered totals show no overlap here
    assert np.array_equal(got["image"][alone], plain["image"][alone]) and not np.array_equal(got["image"], plain["image"])


def test_device_round_trip_on_the_admitted_labels(scene):
    """label_contours(img) -> rasterize_rings -> img, on the labels contour_cases.admitted admits"""
    img, want, ok, _, _, _ = scene
    assert len(ok) >= 0.5 * len(want["by_label"])
    out = label_contours(torch.as_tensor(img, device=DEV))
    keep = torch.isin(out["label_ids"], torch.as_tensor(ok, dtype=torch.int32, device=DEV)).nonzero().view(-1)
    offs, xy = out["ring_offsets"], out["xy"]
    lengths = (offs[1:] - offs[:-1])[keep]
    sub = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=DEV)
    sub[1:] = torch.cumsum(lengths, 0)
    ring_of = torch.repeat_interleave(torch.arange(keep.numel(), device=DEV), lengths)
    rows = torch.arange(int(sub[-1]), device=DEV) - sub[ring_of] + offs[:-1][keep][ring_of]
    back = rasterize_rings(sub, xy[rows], img.shape, labels=out["label_ids"][keep])
    assert np.array_equal(back["image"].cpu().numpy(), np.where(np.isin(img, ok), img, 0))
    assert torch.equal(back["n_covered"], out["n_pixels"][keep]) and int(back["counters"][1]) == 0


def test_device_found_errors_are_raised_after_the_call():
    offs, xy = to_device([rc.HAND_SQUARE])
    with pytest.raises(ValueError, match="labels must be >= 1"):
        rasterize_rings(offs, xy, (8, 8), labels=torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="non-finite"):
        rasterize_rings(offs, torch.full_like(xy, float("nan")), (8, 8))
    with pytest.raises(ValueError, match="ring_offsets of polygon 0"):
        rasterize_rings(torch.tensor([0, 9], device=DEV), xy, (8, 8))
    empty = rasterize_rings(torch.zeros(1, dtype=torch.int64, device=DEV), xy[:0], (5, 7))
    assert tuple(empty["image"].shape) == (5, 7) and int(empty["image"].abs().sum()) == 0 and empty["counters"].tolist() == [0] * 7
