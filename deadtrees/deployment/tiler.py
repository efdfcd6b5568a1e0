"""reference deadtrees/deployment/tiler.py -> deadtrees_amd.deployment.tiler"""
from deadtrees_amd.deployment.tiler import TileInfo, Tiler, divisible_without_remainder, inspect_tile  # noqa: F401
from deadtrees_amd.deployment.tiler import blend_ramp, window_grid  # noqa: F401  (overlap-stitch geometry)
from deadtrees_amd.deployment.tiler import tta_views  # noqa: F401  (test-time augmentation views)
from deadtrees_amd.deployment.tiler import PatchConfig, PatchTable  # noqa: F401  (dead-tree patches of a map)
from deadtrees_amd.deployment.tiler import (outlines_geojson, polygonize, polygonize_host,  # noqa: F401  (their outlines)
                                            write_outlines_geojson)
from deadtrees_amd.deployment.tiler import (PatchMatch, PatchOverlaps, PatchTracks, overlap_pairs_host,  # noqa: F401
                                            patch_overlaps)  # (overlaps of two maps' patches)
from deadtrees_amd.deployment.tiler import (PatchDistances, PatchGaps, ProximityConfig, patch_distances,  # noqa: F401
                                            patch_gaps, patch_proximity_host)  # (nearest-patch distances)
from deadtrees_amd.deployment.tiler import (AttributeConfig, PatchAttributes, patch_attributes,  # noqa: F401
                                            patch_attributes_host)  # (band statistics, indices and confidence per patch)
from deadtrees_amd.deployment.tiler import (CoverGrid, GridConfig, cover_grid, cover_grid_host,  # noqa: F401
                                            write_cover_csv)  # (area-weighted class and zone counts per grid cell)
