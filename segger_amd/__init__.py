"""segger_amd: MI355X-native hot path of dpeerlab/segger.

Heterogeneous transcript<->boundary GATv2 message passing and the
transcript->cell edge-scoring heads, as hand-written gfx950 HIP kernels behind a
C ABI (``include/segger_amd.h`` -> ``segger_amd/libsegger_amd.so``), with
host-side mirrors of the reference's ``ISTEncoder`` and ``LitISTEncoder``.
"""
from .hetero import HeteroBatch, collate, TX_TX, TX_BD, TX_NB_BD  # noqa: F401
from .ist_encoder import ISTEncoder, SkipGAT, Positional2dEmbedder, GATv2Conv  # noqa: F401
from .lightning_model import LitISTEncoder  # noqa: F401
from .postprocess import SegmentationAccumulator, expression_matrix, expression_to_scipy, gene_thresholds  # noqa: F401
from .features import expression_features, sparse_gram, sparse_project, cluster_cosine_similarity, anndata_features  # noqa: F401
from . import phenograph  # noqa: F401  (the module: its function of the same name stays segger_amd.phenograph.phenograph)
from .phenograph import knn_bruteforce, jaccard_graph, louvain  # noqa: F401
from . import validation  # noqa: F401
from .validation import neighbor_frequencies, reference_table, contamination_posterior, calculate_contamination, contamination_flow  # noqa: F401
from . import morphology  # noqa: F401
from .morphology import polygon_props, morphology_features, rings_from_padded  # noqa: F401
from . import geometry  # noqa: F401
from .geometry import points_in_polygons  # noqa: F401
from .neighbors import prediction_graph_shape, prediction_graph_nearest  # noqa: F401
from . import nearest  # noqa: F401
from .nearest import nearest_boundaries, signed_distance  # noqa: F401
from . import boundaries  # noqa: F401
from .boundaries import cell_boundaries, segmentation_boundaries  # noqa: F401
from .boundaries import cell_outlines, segmentation_outlines  # noqa: F401
from . import contours  # noqa: F401
from .contours import label_contours  # noqa: F401
from . import simplify  # noqa: F401
from .simplify import contour_tolerance, rings_simple, simplify_rings  # noqa: F401
from . import repair  # noqa: F401
from .repair import repair_rings, resort_rings  # noqa: F401
from . import overlap  # noqa: F401
from .overlap import match_polygons, polygon_overlaps, polygons_in_polygons  # noqa: F401
from . import fragments  # noqa: F401
from .fragments import FragmentAccumulator, fragment_cells, connected_components, unassigned_mask, merge_fragments  # noqa: F401
from . import buffered_counts  # noqa: F401  (the module, as phenograph: its function of the same name stays segger_amd.buffered_counts.buffered_counts)
from .buffered_counts import buffered_counts_regions, buffered_counts_to_scipy, filter_boundaries  # noqa: F401
from . import rasterize  # noqa: F401
from .rasterize import rasterize_rings  # noqa: F401

__version__ = "0.1.0"
