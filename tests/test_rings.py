"""segger_amd.rings on the CPU: ``ring_csr`` speaks in its caller's name, counts a ring's vertices the way the kernels do
(a closing duplicate of the first vertex is not one) and hands back what the device code reads; ``raise_ring_errors`` names
the first polygon with bad offsets.  Nothing here needs a device."""
import pytest
import torch

from segger_amd import _lib, rings

WHO = "xyz"
CAP = _lib.MORPH_MAX_VERTS


def good():
    return torch.tensor([0, 4]), torch.rand(4, 2, dtype=torch.float64)


@pytest.mark.parametrize("what, offsets, xy", [
    ("offsets are a list", [0, 4], good()[1]),
    ("xy is a list", good()[0], [[0.0, 0.0]] * 4),
    ("2-D offsets", torch.zeros(2, 2, dtype=torch.int64), good()[1]),
    ("no offsets", torch.zeros(0, dtype=torch.int64), good()[1]),
    ("float offsets", torch.tensor([0.0, 4.0]), good()[1]),
    ("xy [V, 3]", good()[0], torch.rand(4, 3)),
    ("xy [V]", good()[0], torch.rand(8)),
    ("integer xy", good()[0], torch.zeros(4, 2, dtype=torch.int64)),
    ("mixed devices", good()[0].to("meta"), good()[1]),
])
def test_every_rejection_is_in_the_callers_name(what, offsets, xy):
    with pytest.raises(ValueError, match=rf"^{WHO}: .*(ring_offsets|xy)"):
        rings.ring_csr(WHO, offsets, xy)


def test_the_cap_counts_open_vertices():
    ring = torch.rand(CAP + 1, 2, dtype=torch.float64)
    ring[-1] = ring[0] + 1.0                                         # CAP + 1 distinct entries
    head = torch.rand(3, 2, dtype=torch.float64)
    offsets = torch.tensor([0, 3, 3 + CAP + 1])
    with pytest.raises(ValueError, match=rf"^{WHO}: polygon 1 has {CAP + 1} vertices, more than SEGGER_MORPH_MAX_VERTS = {CAP}$"):
        rings.ring_csr(WHO, offsets, torch.cat([head, ring]))
    closed = ring.clone()
    closed[-1] = closed[0]                                           # CAP vertices and their closing duplicate
    o, v, n_polygons, n_vertices = rings.ring_csr(WHO, offsets, torch.cat([head, closed]))
    assert (n_polygons, n_vertices) == (2, 3 + CAP + 1)
    with pytest.raises(ValueError, match=rf"^{WHO}: polygon 0 has {CAP + 2} vertices"):      # closed, and still one too many
        rings.ring_csr(WHO, torch.tensor([0, CAP + 2]), torch.cat([closed[:1], closed]))
    assert rings.ring_csr(WHO, torch.tensor([0, CAP]), ring[:CAP])[2] == 1                   # open, at the cap


def test_the_csr_comes_back_as_the_device_code_reads_it():
    offsets = torch.tensor([0, 3, 3, 7], dtype=torch.int32)
    xy = torch.rand(2, 7, dtype=torch.float32).t()                   # [7, 2], not contiguous
    assert not xy.is_contiguous()
    o, v, n_polygons, n_vertices = rings.ring_csr(WHO, offsets, xy)
    assert o.dtype == torch.int64 and o.is_contiguous() and o.tolist() == [0, 3, 3, 7]
    assert v.dtype == torch.float64 and v.is_contiguous() and torch.equal(v, xy.double())
    assert (n_polygons, n_vertices) == (3, 7)
    o, v, n_polygons, n_vertices = rings.ring_csr(WHO, torch.zeros(1, dtype=torch.int64), xy[:0])
    assert (n_polygons, n_vertices) == (0, 0) and v.shape == (0, 2)


def test_error_words():
    offsets = torch.tensor([0, 4, 3, 12])
    rings.raise_ring_errors(WHO, 0, offsets, 10)
    with pytest.raises(ValueError, match=rf"^{WHO}: ring_offsets of polygon 1 are negative, descending or beyond the 10 vertices$"):
        rings.raise_ring_errors(WHO, _lib.PJOIN_ERR_OFFSETS, offsets, 10)
    with pytest.raises(ValueError, match=rf"^{WHO}: ring_offsets of polygon 2 are"):
        rings.raise_ring_errors(WHO, _lib.MORPH_ERR_OFFSETS | _lib.MORPH_ERR_CAP, torch.tensor([0, 4, 4, 12]), 10)
    for word in (_lib.MORPH_ERR_CAP, _lib.PJOIN_ERR_BUFFER, _lib.PJOIN_ERR_FILL | _lib.PJOIN_ERR_BUFFER):
        with pytest.raises(ValueError, match=rf"^{WHO}: the device reported error word {word}$"):
            rings.raise_ring_errors(WHO, word, offsets, 10)
    assert _lib.MORPH_ERR_OFFSETS == _lib.PJOIN_ERR_OFFSETS and _lib.MORPH_ERR_CAP == _lib.PJOIN_ERR_CAP


def test_the_modules_share_one_definition():
    import segger_amd
    from segger_amd import geometry, morphology
    assert morphology.rings_from_padded is rings.rings_from_padded is segger_amd.rings_from_padded
    assert geometry.ring_csr is rings.ring_csr is morphology.ring_csr
    assert not hasattr(morphology, "_rings")
