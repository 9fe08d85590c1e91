"""C-ABI surface of the streaming-assignment entry points (CPU): bad arguments are rejected on the host with
SEGGER_EINVAL and a message -- nothing is launched -- and an empty update is a no-op."""
import pytest

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 8-byte aligned address: never dereferenced, every call below is rejected


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def update(lib, n=100, n_tx=1000, tx=FAKE, seg=FAKE, sim=FAKE, gene=FAKE, mask=None, key=FAKE, cell=FAKE, gene_out=FAKE,
           counters=FAKE):
    return lib.segger_assign_update(tx, seg, sim, gene, mask, n, key, cell, gene_out, counters, n_tx, None)


def finalize(lib, n_tx=1000, key=FAKE, sim=FAKE, seen=FAKE):
    return lib.segger_assign_finalize(key, n_tx, sim, seen, None)


def test_abi_version(lib):
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION


def test_update_rejects_bad_arguments(lib):
    assert update(lib, n=-1) == EINVAL and b"negative" in lib.segger_last_error()
    assert update(lib, n=1 << 32) == EINVAL and b"2^32" in lib.segger_last_error()
    assert update(lib, n_tx=0) == EINVAL and b"n_tx" in lib.segger_last_error()
    assert update(lib, n_tx=-5) == EINVAL and b"n_tx" in lib.segger_last_error()
    assert update(lib, n_tx=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    for name in ("tx", "seg", "sim", "gene", "key", "cell", "gene_out", "counters"):
        assert update(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    for name in ("tx", "seg", "key", "counters"):
        assert update(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in lib.segger_last_error(), name
    for name in ("sim", "gene", "cell", "gene_out"):
        assert update(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in lib.segger_last_error(), name


def test_empty_update_launches_nothing(lib):
    assert update(lib, n=0) == 0
    assert update(lib, n=0, tx=None, seg=None, sim=None, gene=None, key=None, cell=None, gene_out=None, counters=None) == 0
    assert update(lib, n=0, n_tx=0) == EINVAL                        # the sizes are still checked


def test_finalize_rejects_bad_arguments(lib):
    assert finalize(lib, n_tx=0) == EINVAL and b"n_tx" in lib.segger_last_error()
    assert finalize(lib, n_tx=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    for name in ("key", "sim", "seen"):
        assert finalize(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    assert finalize(lib, key=FAKE + 4) == EINVAL and b"8-byte aligned" in lib.segger_last_error()
    assert finalize(lib, sim=FAKE + 2) == EINVAL and b"4-byte aligned" in lib.segger_last_error()


def test_accumulator_rejects_on_the_host():
    from segger_amd import postprocess as pp
    for n in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            pp.SegmentationAccumulator(n, "cuda")
    with pytest.raises(_lib.SeggerAmdError):
        pp.SegmentationAccumulator(10, "cpu")                        # no CPU fallback: best_assignment is the CPU form
