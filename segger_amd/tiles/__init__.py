"""Device-resident tile batcher: what feeds the hot path.

Restates the reference's ``data/tiling.py``, ``data/partition/`` and ``data/tile_dataset.py`` with tensors that can live
in HBM for the whole run; by subject: tiling (``SquareTiling``, ``QuadTreeTiling``), segments (rows grouped into contiguous
segments: the one store behind partition tiles, shards and prediction bins), partition (``TilePartition``), packing (the bin
packers and ``TileBatchSampler``), predict (``PredictTiles`` and its binned forms).  Each module names what it restates.

The reference slices on the host inside DataLoader workers and ships every batch over PCIe; here the
partitioned graph stays on the device and a batch is assembled by index arithmetic on device tensors
(``TilePartition.batch``), so 8 ranks are not limited by Python ``__getitem__`` + collate.
Everything is plain torch (works on CPU tensors too, which is how the unit tests run it); the quadtree has a plain-torch
path with the same exact-integer contract next to its kernels.
"""
from ..hetero import EdgeType, HeteroBatch
from .tiling import QuadTreeTiling, SquareTiling
from .segments import Segments
from .partition import NODE_SKIP, TilePartition, partition_by_tiling
from .packing import TileBatchSampler, _indexed, best_fit_decreasing, first_fit_decreasing_bucketed, harmonic_k
from .predict import PredictQuadTreeIndex, PredictTileIndex, PredictTiles, _BinnedPredictTiles
