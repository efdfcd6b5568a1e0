"""``Tiler`` — the reference's whole-tile splitter/merger (deadtrees/deployment/tiler.py:22-170) with the same
constructor, ``load_file`` / ``get_batches`` / ``put_batches`` / ``write_file`` contract, plus an array-level entry
(``load_array``) and a rank-sharded tile-queue driver (``infer_tile``) for the MI355X path.

Contract kept from the reference (scripts/inference.py:80-115 runs against it unchanged):

* ``Tiler(infile=None, tile_shape=(2048, 2048), subtile_shape=(256, 256))``; non-square sub-tiles -> ``ValueError``;
* the source raster is zero-padded to ``tile_shape`` (tiler.py:108-114) and cut into NON-overlapping sub-tiles with
  ``make_blocks_vectorized`` (utils/data_handling.py:9-19) — there is no overlap stitching in the reference;
* ``get_batches() -> ndarray [n_used, C, d, d]``: only the sub-tiles that intersect the valid raster
  (``_subtiles_to_use``, tiler.py:121-134) — all-padding sub-tiles never reach the network;
* ``put_batches(ndarray [n_used, d, d])``: the skipped sub-tiles are zero-filled, blocks are merged with
  ``unmake_blocks_vectorized`` (data_handling.py:22-34) into the padded ``_outdata`` and cropped to the raster size.

GeoTIFF I/O goes through rioxarray exactly like the reference when that package is importable; it is absent from
this image, so ``load_file`` / ``write_file`` raise an ``ImportError`` that says so, and ``load_array`` /
``result`` are the array-level way in and out (what the tests and the bench use).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from pathlib import Path
from typing import List, Mapping, Optional, Tuple, Union

import numpy as np
import torch

from .analysis import MapAnalysis, run_device, run_host
from .attributes import AttributeConfig, PatchAttributes, patch_attributes, patch_attributes_host  # noqa: F401
from .cover import (CoverGrid, GridConfig, check_grid, cover_grid, cover_grid_host,  # noqa: F401
                    write_cover_csv)  # (the ``grid`` argument of infer_tile)
from .crowns import CrownConfig, CrownSplit, split_patches, split_patches_host  # noqa: F401
from .outlines import outlines_geojson, polygonize, polygonize_host, write_outlines_geojson  # noqa: F401
from .overlaps import (PatchMatch, PatchOverlaps, PatchTracks, overlap_pairs_host, patch_overlaps)  # noqa: F401
from .proximity import (PatchDistances, PatchGaps, ProximityConfig, patch_distances, patch_gaps,  # noqa: F401
                        patch_proximity_host)
from .patches import PatchConfig, PatchTable  # noqa: F401  (the ``patches`` argument of infer_tile)
from ..loss.curves import Decision, check_decision  # noqa: F401  (the ``decision`` argument of infer_tile)


def divisible_without_remainder(a, b):
    if b == 0:
        return False
    return True if a % b == 0 else False


def make_blocks_vectorized(x: np.ndarray, d: int) -> np.ndarray:
    """[C,M,N] -> [(M/d)*(N/d), C, d, d] (row-major over blocks) — utils/data_handling.py:9-19"""
    p, m, n = x.shape
    return x.reshape(p, m // d, d, n // d, d).transpose(1, 3, 0, 2, 4).reshape(-1, p, d, d)


def unmake_blocks_vectorized(x, d: int, m: int, n: int) -> np.ndarray:
    """blocks [k,d,d] (or a sequence of such batches) -> [m,n] — utils/data_handling.py:22-34"""
    return np.concatenate(x).reshape(m // d, n // d, d, d).transpose(0, 2, 1, 3).reshape(m, n)


# ---------------------------------------------------------------------- overlap-stitch geometry (no GPU needed)
# One definition, restated by csrc/stitch.hip: d = window edge, overlap o even with 0 <= o <= d/2, stride s = d - o; an
# axis of length L carries n(L) = max(1, ceil((L - o) / s)) windows; window k = i * nx + j starts at (i * s, j * s).
def _check_overlap(d: int, overlap: int) -> None:
    if d <= 0:
        raise ValueError(f"window edge must be positive, got {d}")
    if overlap < 0 or overlap % 2:
        raise ValueError(f"overlap must be even and >= 0, got {overlap}")
    if 2 * overlap > d:
        raise ValueError(f"overlap must be <= d/2 = {d // 2}, got {overlap}")


def window_grid(h: int, w: int, d: int, overlap: int = 0) -> Tuple[int, int, int]:
    """(ny, nx, stride) of the d x d windows that cover an h x w raster with ``overlap`` pixels shared between neighbours;
    overlap 0 is the block grid (ceil(h/d), ceil(w/d), d)"""
    _check_overlap(d, overlap)
    s = d - overlap
    return max(1, -(-(h - overlap) // s)), max(1, -(-(w - overlap) // s)), s


def blend_ramp(d: int, overlap: int) -> np.ndarray:
    """fp64 [d] blend weights along one axis of a window: r(t) = min(1, (t+1)/(o+1), (d-t)/(o+1)); a window pixel (y, x)
    weighs r(y) * r(x), and the ramps of two neighbouring windows sum to 1 across their overlap"""
    _check_overlap(d, overlap)
    t = np.arange(d, dtype=np.float64)
    return np.minimum(1.0, np.minimum((t + 1.0) / (overlap + 1.0), (d - t) / (overlap + 1.0)))


def window_keep(i: int, n: int, d: int, overlap: int) -> Tuple[int, int]:
    """crop mode: the raster rows (columns alike) [lo, hi) that window ``i`` of ``n`` keeps — interior edges give up
    overlap/2 pixels; the kept ranges tile [0, (n-1) * stride + d) exactly once"""
    s = d - overlap
    return i * s + (overlap // 2 if i > 0 else 0), i * s + d - (overlap // 2 if i < n - 1 else 0)


# ---------------------------------------------------------------------- test-time augmentation views (no GPU needed)
# A view is (flip, rot): flip 0 none / 1 horizontal / 2 vertical, rot = k of np.rot90; view = rot90^k(flip(window)) — the
# convention of the training augmentation (csrc/views.h).  A vertical flip is a horizontal one turned by 180 degrees, so
# (2, k) is stored as (1, (k + 2) % 4): the eight distinct views are flip in {0, 1} x rot in 0..3.
_TTA_SETS = {
    "flips": ((0, 0), (1, 0), (2, 0), (0, 2)),          # identity, horizontal, vertical, both
    "d4": tuple((f, k) for f in (0, 1) for k in range(4)),
}


def tta_views(spec=None) -> Tuple[Tuple[int, int], ...]:
    """the views of a test-time-augmentation request as canonical ``(flip, rot)`` pairs: ``None`` -> the identity alone,
    ``"flips"`` -> identity / horizontal / vertical / both, ``"d4"`` -> all eight, or an explicit sequence of pairs.
    ``ValueError`` for an unknown name, an empty list, values outside flip 0..2 / rot 0..3, and views that coincide"""
    if spec is None:
        return ((0, 0),)
    if isinstance(spec, str):
        if spec not in _TTA_SETS:
            raise ValueError(f"tta {spec!r}: use None, 'flips', 'd4' or a sequence of (flip, rot) pairs")
        spec = _TTA_SETS[spec]
    views = []
    for item in spec:
        try:
            flip, rot = item
        except (TypeError, ValueError):
            raise ValueError(f"tta view {item!r}: expected a (flip, rot) pair") from None
        if flip not in (0, 1, 2) or rot not in (0, 1, 2, 3):
            raise ValueError(f"tta view {item!r}: flip must be in 0..2 and rot in 0..3")
        views.append((1, (int(rot) + 2) % 4) if flip == 2 else (int(flip), int(rot)))
    if not views:
        raise ValueError("tta: no views given")
    if len(set(views)) != len(views):
        raise ValueError(f"tta: duplicate views after canonicalisation: {views}")
    return tuple(views)


@dataclass
class TileInfo:
    size: Tuple[int, int]
    subtiles: Tuple[int, int]


def _rioxarray():
    try:
        import rioxarray  # type: ignore
        return rioxarray
    except Exception as e:  # noqa: BLE001
        raise ImportError("GeoTIFF I/O needs the `rioxarray` package (reference deployment/tiler.py:15), which is not "
                          "installed here: use Tiler.load_array(array) / Tiler.result for in-memory rasters") from e


def inspect_tile(infile, tile_shape: Tuple[int, int] = (8192, 8192),
                 subtile_shape: Tuple[int, int] = (512, 512)) -> TileInfo:
    """reference tiler.py:34-56; ``infile``: a path (rioxarray), or anything with ``.shape`` [(C,)H,W]"""
    if hasattr(infile, "shape"):
        shape = tuple(int(v) for v in infile.shape[-2:])
    else:
        with _rioxarray().open_rasterio(infile).sel(band=1, drop=True) as da:
            shape = tuple(da.shape)
    if not divisible_without_remainder(tile_shape[0], subtile_shape[0]):
        raise ValueError(f"Shapes unaligned (v): {tile_shape[0], subtile_shape[0]}")
    if not divisible_without_remainder(tile_shape[1], subtile_shape[1]):
        raise ValueError(f"Shapes unaligned (h): {tile_shape[1], subtile_shape[1]}")
    subtiles = (math.ceil(shape[0] / subtile_shape[0]), math.ceil(shape[1] / subtile_shape[1]))
    return TileInfo(size=shape, subtiles=subtiles)


class Tiler:
    def __init__(self, infile: Optional[Union[str, Path]] = None, tile_shape: Optional[Tuple[int, int]] = (2048, 2048),
                 subtile_shape: Optional[Tuple[int, int]] = (256, 256)) -> None:
        self._infile = infile
        self._tile_shape = tuple(tile_shape)
        self._subtile_shape = tuple(subtile_shape)
        if subtile_shape[0] != subtile_shape[1]:
            raise ValueError("Subtile required to have matching x/y dims")
        self._source = None
        self._target = None
        self._indata: Optional[np.ndarray] = None
        self._outdata: Optional[np.ndarray] = None
        self._batch_shape = None
        self._subtiles_to_use: Optional[np.ndarray] = None
        self._tile_info: Optional[TileInfo] = None

    # ------------------------------------------------------------------ sources
    def _set_shapes(self, tile_shape, subtile_shape):
        self._tile_shape = tuple(tile_shape) if tile_shape else self._tile_shape
        if subtile_shape:
            if subtile_shape[0] != subtile_shape[1]:
                raise ValueError("Subtile required to have matching x/y dims")
        self._subtile_shape = tuple(subtile_shape) if subtile_shape else self._subtile_shape

    def _stage(self, sv: np.ndarray):
        """pad to the tile shape, allocate the output plane, mark the sub-tiles that hold data (tiler.py:106-134)"""
        if sv.shape[1] > self._tile_shape[0] or sv.shape[2] > self._tile_shape[1]:
            raise ValueError(f"raster {sv.shape[1:]} larger than the tile shape {self._tile_shape}")
        if tuple(self._tile_shape) != tuple(self._tile_info.size):
            self._indata = np.zeros((sv.shape[0], *self._tile_shape), dtype=sv.dtype)
            self._indata[:, 0:sv.shape[1], 0:sv.shape[2]] = sv
        else:
            self._indata = sv
        self._outdata = np.zeros(self._tile_shape, dtype="uint8")
        mask = np.zeros((self._tile_shape[0] // self._subtile_shape[0], self._tile_shape[1] // self._subtile_shape[1]),
                        dtype=bool)
        mask[0:self._tile_info.subtiles[0], 0:self._tile_info.subtiles[1]] = 1
        self._subtiles_to_use = mask.ravel()
        self._batch_shape = None

    def load_file(self, infile: Union[str, Path], tile_shape: Optional[Tuple[int, int]] = None,
                  subtile_shape: Optional[Tuple[int, int]] = None) -> None:
        """reference tiler.py:82-134 (needs rioxarray)"""
        rio = _rioxarray()
        self._infile = infile
        self._set_shapes(tile_shape, subtile_shape)
        self._tile_info = inspect_tile(self._infile, self._tile_shape, self._subtile_shape)
        self._source = rio.open_rasterio(self._infile, chunks={"band": 4, "x": 256, "y": 256})
        self._target = self._source.sel(band=1, drop=True).astype("uint8").copy(deep=True)
        self._stage(self._source.values)

    def load_array(self, arr_chw: np.ndarray, tile_shape: Optional[Tuple[int, int]] = None,
                   subtile_shape: Optional[Tuple[int, int]] = None) -> None:
        """the in-memory twin of ``load_file``: a [C,H,W] raster (what ``rioxarray.open_rasterio(f).values`` holds)"""
        arr_chw = np.asarray(arr_chw)
        if arr_chw.ndim != 3:
            raise ValueError(f"expected a [C,H,W] raster, got shape {arr_chw.shape}")
        self._infile = None
        self._set_shapes(tile_shape, subtile_shape)
        self._tile_info = inspect_tile(arr_chw, self._tile_shape, self._subtile_shape)
        self._source, self._target = arr_chw, None
        self._stage(arr_chw)

    # ------------------------------------------------------------------ batches
    def get_batches(self) -> np.ndarray:
        if self._indata is None:
            raise RuntimeError("Tiler: load_file / load_array first")
        subtiles = make_blocks_vectorized(self._indata, self._subtile_shape[0])
        self._batch_shape = self._batch_shape or subtiles.shape
        return subtiles[self._subtiles_to_use]

    def put_batches(self, batches: np.ndarray) -> None:
        batches = np.asarray(batches)
        n_used = int(self._subtiles_to_use.sum())
        d = self._subtile_shape[0]
        if batches.shape[0] != n_used or tuple(batches.shape[1:]) != (d, d):
            raise ValueError(f"expected {n_used} sub-tile maps of {d}x{d}, got {batches.shape}")
        expanded = np.zeros((self._subtiles_to_use.size, d, d), dtype=batches.dtype)   # skipped sub-tiles stay zero
        expanded[self._subtiles_to_use] = batches
        self._outdata = unmake_blocks_vectorized(expanded, d, self._tile_shape[0], self._tile_shape[1])
        if self._target is not None:   # geo-registered copy of the valid part (tiler.py:166-170)
            self._target = self._target.load()
            self._target.loc[:] = self._outdata[0:self._tile_info.size[0], 0:self._tile_info.size[1]]

    @property
    def result(self) -> np.ndarray:
        """the merged class map cropped to the raster size (what ``write_file`` stores)"""
        return self._outdata[0:self._tile_info.size[0], 0:self._tile_info.size[1]]

    def stats(self, zones=None, classes: int = 3, n_zones: Optional[int] = None, patches=None, outlines=None,
              against=None, against_patches=None, distances=None, gaps=None, attributes=None, crowns=None,
              against_crowns=None, grid=None):
        """``RasterStats`` of ``result``: what ``infer_tile(..., stats=True)`` returns, for a caller of the reference's own
        ``get_batches`` / ``put_batches`` loop, computed on the host (``analysis.run_host``).  ``classes``: the model's class
        count; ``zones`` / ``n_zones`` / ``patches`` / ``outlines`` / ``against`` / ``against_patches`` / ``distances`` /
        ``gaps`` / ``attributes`` / ``crowns`` / ``against_crowns`` / ``grid``: as in ``infer_tile``, with the same rules
        (``MapAnalysis``); the attributes are read from the
        loaded raster, and the host path has no probabilities, so ``confidence=True`` is refused.  Polygons are burnt by
        ``rasterize_host``; a ``patches`` configuration that sieves changes ``result`` itself, and the counts are those of the
        sieved map"""
        if self._outdata is None:
            raise RuntimeError("Tiler: load_file / load_array first")
        return self._analyse(MapAnalysis.of("Tiler.stats", self.result.shape, classes, zones, against, self._raster(),
                                            n_zones=n_zones, patches=patches, outlines=outlines,
                                            against_patches=against_patches, distances=distances, gaps=gaps,
                                            attributes=attributes, no_probs="Tiler.stats runs on the host, which has none",
                                            crowns=crowns, against_crowns=against_crowns, grid=grid))

    def _raster(self) -> np.ndarray:
        """the loaded raster cropped to its own size: a view of the padded input"""
        return self._indata[:, 0:self._tile_info.size[0], 0:self._tile_info.size[1]]

    def _analyse(self, request: MapAnalysis):
        """the ``RasterStats`` of ``result`` under a checked request (``analysis.run_host``); a sieved map replaces ``result``"""
        sieved, stats = run_host(request, self.result, raster=self._raster())
        if request.patches is not None and request.patches.sieves:
            self.result[...] = sieved                            # a view into ``_outdata``
        return stats

    def write_file(self, outfile: Union[str, Path]) -> None:
        """reference tiler.py:136-142 (LZW-compressed tiled GeoTIFF through rioxarray)"""
        if self._target is None:
            _rioxarray()
            raise RuntimeError("Tiler.write_file: no geo-registered source (load_file was not used); read Tiler.result")
        self._target[:] = self._outdata[0:self._tile_info.size[0], 0:self._tile_info.size[1]]
        self._target.rio.to_raster(outfile, compress="LZW", tiled=True)


def infer_rasters(inference, rasters, subtile: int = 256, batch_size: int = 64, rank: int = 0, world: int = 1,
                  device: str = "cuda", tile_shape: Optional[Tuple[int, int]] = None, skip_blank: bool = True,
                  overlap: int = 0, blend: str = "crop", return_probs: bool = False, tta=None, stats: bool = False,
                  zones=None, n_zones: Optional[int] = None, patches=None, outlines=None, against=None,
                  against_patches=None, distances=None, gaps=None, attributes=None, decision=None, crowns=None,
                  against_crowns=None, grid=None):
    """the directory loop of scripts/inference.py:71-115 over in-memory rasters (GeoTIFF I/O needs rioxarray, absent
    here): ``rasters`` yields ``array`` or ``(key, array)``; rank r of ``world`` takes rasters r, r + world, ... (tiles are
    independent: no collective).  Yields ``(key, class_map)`` in input order of the rank's share; rasters whose band 1
    holds only 0 / 255 (``is_valid_tile``, :60-62) are skipped like the reference does — ``(key, None)`` — without a
    forward pass (device reduction over the uploaded raster, ``ops.band_has_data``).  ``overlap`` / ``blend`` /
    ``return_probs`` / ``tta`` / ``stats`` / ``n_zones`` / ``patches`` / ``outlines`` / ``against_patches`` / ``distances`` /
    ``gaps`` / ``attributes`` / ``decision`` / ``crowns`` / ``against_crowns``: as in ``infer_tile``, with the same rules,
    checked before the first raster is read (every raster
    stays on its rank, so overlap needs no exchange); ``zones``: a callable ``key -> uint8 [h, w] array, PolygonSet or None``,
    or a mapping (a missing key is None); ``against``: the same for the map every raster is compared with (a uint8 array, a ``PolygonSet``
    or None: that raster's statistics carry no overlaps); ``grid``: one ``GridConfig`` for every raster, or a callable ``key ->
    GridConfig or None`` or a mapping (a missing key is None) — every raster has its own pixel frame, so a regional lattice is
    one ``GridConfig.from_world`` per geotransform, and ``CoverGrid.merge`` of the rasters' ``.grid`` is the regional grid.
    The second item of every pair is whatever ``infer_tile`` returned: with ``stats=True`` ``(map, RasterStats)`` — the
    ``RasterStats`` of a rank's share add up (``+``) to that rank's part of the regional totals."""
    per_raster = grid is not None and not isinstance(grid, GridConfig) and (callable(grid) or isinstance(grid, Mapping))
    if per_raster and not stats:
        raise ValueError("infer_rasters: grid needs stats=True")
    rules = MapAnalysis.rules("infer_rasters", getattr(inference, "classes", None) if stats else None, stats, zones, n_zones,
                              patches, outlines, against, against_patches, distances, gaps, attributes,
                              _no_probs(inference, overlap, blend, tta), crowns=crowns, against_crowns=against_crowns,
                              grid=None if per_raster else grid)
    decision = _check_decision("infer_rasters", inference, decision, overlap, blend, tta)
    for i, item in enumerate(rasters):
        if i % world != rank:
            continue
        key, arr = item if isinstance(item, tuple) else (i, item)
        z = None if zones is None else zones(key) if callable(zones) else zones.get(key)
        other = None if against is None else against(key) if callable(against) else against.get(key)
        if per_raster:
            try:
                rules = replace(rules, grid=check_grid(grid(key) if callable(grid) else grid.get(key)))
            except ValueError as e:
                raise ValueError(f"infer_rasters: {e}") from None
        request = None if rules is None else rules.bind("infer_tile", np.shape(arr)[1:], z, other, arr)
        yield key, _infer_tile(inference, arr, request, subtile, batch_size, 0, 1, device, None, tile_shape, None, skip_blank,
                               overlap, blend, return_probs, tta, decision)


def infer_tile(inference, arr_chw_u8: np.ndarray, subtile: int = 256, batch_size: int = 64, rank: int = 0,
               world: int = 1, device: str = "cuda", group=None, tile_shape: Optional[Tuple[int, int]] = None,
               on_device: Optional[bool] = None, skip_blank: bool = False, overlap: int = 0, blend: str = "crop",
               return_probs: bool = False, tta=None, stats: bool = False, zones=None, n_zones: Optional[int] = None,
               patches=None, outlines=None, against=None, against_patches=None, distances=None, gaps=None,
               attributes=None, decision=None, crowns=None, against_crowns=None, grid=None):
    """whole-tile inference of scripts/inference.py:80-115 on the MI355X path: split -> (uint8 H2D, normalise on the
    device) -> forward + fused argmax -> uint8 D2H -> merge.  With world > 1 the sub-tile batches j = rank (mod world)
    are processed locally and the uint8 class maps are all-gathered (no other collective: tiles are independent).
    ``on_device`` (default: single rank + uint8 raster + HIP device) does the block split / merge on the GPU as well:
    one H2D copy of the raster, one D2H copy of the merged map (``_infer_tile_on_device``; same result, tested).

    ``overlap`` > 0 (even, <= subtile/2): neighbouring windows share that many pixels (``window_grid``) and are stitched
    on the device, single rank only — ``blend="crop"``: every window keeps its centre (``window_keep``), the map is the
    fused argmax of exactly one window per pixel; ``blend="average"``: the windows' softmax probabilities are blended with
    the ramp weights of ``blend_ramp`` and the map is their argmax; ``return_probs=True`` (average mode) returns
    ``(map, probs fp32 [K,h,w])``.  ``overlap=0`` is the block path above, unchanged.

    ``tta`` (``tta_views``: ``"flips"``, ``"d4"`` or (flip, rot) pairs) averages every window's softmax over its views
    before the blend; an ensemble (an inference object with ``members``) votes over its models — ``vote="hard"``: the
    majority of the members' raster maps, ``vote="soft"``: all members add into one accumulator.  Both always take the
    stitched device path, ``overlap=0`` included (``_infer_tile_stitched``); ``batch_size`` counts forward tiles.

    ``stats=True`` returns ``(map, RasterStats)`` (``(map, probs, RasterStats)`` with ``return_probs``; a blank raster under
    ``skip_blank`` is still None): the class counts of the map (``deployment/stats.py``), K = ``inference.classes``.  The
    options below need it; their rules are checked by ``MapAnalysis`` (``deployment/analysis.py``) before anything runs.  On
    every device path the maps they name are uploaded next to the raster — a ``PolygonSet`` in the raster's pixel
    coordinates is burnt in HBM instead (``ops.rasterize_polygons``) — and everything is computed from the final map in
    HBM before its download, in the fixed order of ``analysis.run_device``; the host path (``on_device=False``,
    ``world > 1``, CPU) runs the same contracts in numpy / scipy on the merged map (``analysis.run_host``).

    ``zones``: a uint8 [h, w] array on the raster's grid (forest mask, land use, a previous year's map — the counts are then
    the year-to-year transition matrix) splits the counts by zone (ONE ``ops.zonal_counts``), ``n_zones`` (<= 8) defaults
    to ``zones.max() + 1``.  The map is the one the call without ``stats`` returns.  As a ``PolygonSet`` (``data/polygons.py``:
    forest masks and stand boundaries arrive as polygons; zone ids as values, 0 outside every polygon, ``n_zones`` defaults
    to the largest value + 1) maps and counts are those of the call with the burnt array.

    ``patches=True`` or a ``PatchConfig(connectivity=8, min_pixels=0)``: the ``RasterStats`` carries the map's ``PatchTable``
    as ``.patches`` (``deployment/patches.py``: one row per connected dead-tree patch).  With ``min_pixels > 1`` the map is
    sieved before the counts: the returned map is the sieved one and ``counts`` are the counts of the RETURNED map; the
    probabilities of ``return_probs`` are not touched by the sieve.  With ``min_pixels <= 1`` the map is bit-identical to the
    call without ``patches``.

    ``outlines=True`` (needs ``patches``): the ``RasterStats`` also carries ``.outlines``, a ``PolygonSet`` on the raster's
    grid with one polygon per patch — polygon ``k`` is row ``k`` of ``.patches`` (``deployment/outlines.py``: exact ring
    tracing along the pixel edges of the final label plane, after the sieve; ``outlines_geojson`` writes them out).  The
    map, the counts and the table are those of the call without ``outlines``.

    ``against`` (needs ``patches``): a map to compare the result with patch by patch — a uint8 [h, w] class map on the
    raster's grid with values < K (last year's map, a burnt annotation) or a ``PolygonSet`` in its pixel coordinates (the
    annotators' polygons; burnt with ``all_touched=True``, the rule of the training masks).  The ``RasterStats`` carries
    ``.overlaps``, a ``PatchOverlaps`` (``deployment/overlaps.py``): ``table_a`` the patches of ``against`` under
    ``against_patches`` (a ``PatchConfig``; default: the connectivity of ``patches``, no sieve), ``table_b`` the
    ``.patches`` of the final map, and one row per pair of patches that share a pixel — ``match()`` gives the crown-level
    accuracy, ``track()`` the year-to-year fate of every patch.  The map, the counts, the table and the outlines are those
    of the call without ``against``.

    ``distances=True`` or a ``ProximityConfig(max_distance=None)`` (needs ``against``): ``.overlaps.distances`` is a
    ``PatchDistances`` (``deployment/proximity.py``) — for every patch of either map the squared distance, pixel centre to
    pixel centre, to the nearest dead pixel of the other map and the table row of the patch that pixel belongs to: the
    spread distance of a ``NEW`` patch from last year's dead trees.  ``gaps=True`` or a ``ProximityConfig`` (needs
    ``patches``): ``.gaps`` is a ``PatchGaps`` aligned with ``.patches`` — every patch's distance to the nearest OTHER patch
    of the map.  ``max_distance`` (pixels) bounds the search: a patch farther than that from everything has no neighbour.
    Everything else is that of the call without the two options.

    ``attributes=True`` or an ``AttributeConfig(indices=None, confidence=False)`` (needs ``patches``; a uint8 raster of at most
    8 bands): ``.attributes`` is a ``PatchAttributes`` (``deployment/attributes.py``) aligned with ``.patches`` — per patch and
    band the sum, sum of squares, minimum and maximum of the raster's pixels (``mean()``, ``std()``), per index pair the mean
    normalised difference (``index(k)``; default NDVI = bands (3, 0) of an RGBN raster), all from the final, sieved label
    plane.  On the device paths ALL bands of the raster are uploaded, still in one copy, and the network reads its leading
    ``in_channels`` planes: an RGB model over an RGBN raster still yields NDVI.  ``confidence=True`` adds the mean and the
    minimum probability of the patch's class (``confidence()``, ``min_confidence()``); it is accepted exactly where
    ``return_probs=True`` is, and without ``return_probs`` the probabilities stay on the device.  Everything else is that of
    the call without the option.

    ``decision``: a ``Decision`` (``loss/curves.py``: a threshold per class ``1..K-1``, as ``validate(curves=True)`` finds them)
    replaces the arg-max as the rule that turns the blended probabilities into the map: a pixel takes the class c >= 1
    with the largest quantised probability among those that reach their threshold, class 0 without one
    (``ops.decide_classes`` on the probabilities of ``stitch_finalize``).  It is accepted exactly where ``return_probs=True``
    is, and everything downstream — counts, sieve, patch table, outlines, overlaps, gaps, attributes — sees the decided map;
    ``confidence`` is the probability of the decided class.  The probabilities are returned only when ``return_probs`` asks.
    Validation probabilities are single-tile softmaxes, these are blended ones: the threshold transfers, the bit-for-bit
    closure of the curves holds for identical inputs.  A patch-wise decision (``Decision(T, low=..., min_confidence=...,
    connectivity=...)``: grow patches at the low thresholds, keep those with a pixel at ``T`` and a mean of ``M``) runs
    through ``ops.decide_patchwise`` in the same place.  None: nothing changes.

    ``crowns=True`` or a ``CrownConfig(min_core2, max_rounds=256, depth_cap2=65535)`` (needs ``patches``; ``True``:
    ``CrownConfig.from_radius(2)``): touching crowns are split by their inscribed depth behind the sieve
    (``deployment/crowns.py``: cores where the squared distance to another class reaches ``min_core2``, grown back over their
    patch).  The label plane IS the crown plane from there on: ``.patches`` has one row per crown, and outlines, overlaps,
    distances, gaps and attributes align with it as they do with patches; ``.crowns`` is the ``CrownSplit`` (per crown the
    patch it was cut from and its inscribed depth; ``converged``).  ``against_crowns`` (needs ``against``) splits the patches of
    ``against`` the same way.  The returned map and the counts do not change: splitting moves no pixel between classes.

    ``grid``: a ``GridConfig`` (``deployment/cover.py``: cell size and origin in this raster's pixels, or
    ``GridConfig.from_world`` of its geotransform): ``.grid`` is the ``CoverGrid`` of the final map — the map the counts are
    taken from, after sieve, decision and crowns —, area-weighted sums per cell, zone and class in exact integers (ONE
    ``ops.cover_grid`` behind the counts on the device paths, ``cover_grid_host`` on the host path: identical), with
    ``zones`` — array or ``PolygonSet`` — splitting them as it splits the counts (a previous year's map gives per-cell
    transition matrices), and with ``patches`` the patch (or crown) count and area per cell and class, binned by centroid.
    Everything else is that of the call without the option."""
    decision = _check_decision("infer_tile", inference, decision, overlap, blend, tta)
    request = MapAnalysis.of("infer_tile", np.shape(arr_chw_u8)[1:], getattr(inference, "classes", None) if stats else None,
                             zones, against, arr_chw_u8, stats=stats, n_zones=n_zones, patches=patches, outlines=outlines,
                             against_patches=against_patches, distances=distances, gaps=gaps, attributes=attributes,
                             no_probs=_no_probs(inference, overlap, blend, tta), crowns=crowns, against_crowns=against_crowns,
                             grid=grid)
    return _infer_tile(inference, arr_chw_u8, request, subtile, batch_size, rank, world, device, group, tile_shape, on_device,
                       skip_blank, overlap, blend, return_probs, tta, decision)


def _check_decision(caller: str, inference, decision, overlap, blend, tta):
    """the ``decision`` argument, checked before anything runs: a ``Decision`` for the model's classes, and only where the
    call has raster probabilities (the rule of ``return_probs``); None stays None"""
    if decision is None:
        return None
    decision = check_decision(decision, getattr(inference, "classes", None), caller)
    lacking = _no_probs(inference, overlap, blend, tta)
    if lacking:
        raise ValueError(f"{caller}: decision thresholds the blended probabilities: " + lacking.replace("return_probs", "it"))
    return decision


def _no_probs(inference, overlap, blend, tta) -> Optional[str]:
    """what a call lacks to have raster probabilities — the rule of ``return_probs`` — or None when it has them"""
    members = getattr(inference, "members", None)
    if not (overlap or tta is not None or members is not None):
        return "return_probs needs overlap > 0 and blend='average'"
    if blend != "average" or (members is not None and getattr(inference, "vote", "hard") == "hard"):
        return "return_probs needs blend='average' and, for an ensemble, vote='soft'"
    return None


def _infer_tile(inference, arr_chw_u8, request: Optional[MapAnalysis], subtile, batch_size, rank, world, device, group,
                tile_shape, on_device, skip_blank, overlap, blend, return_probs, tta, decision=None):
    """``infer_tile`` behind the check of its statistics options: ``request`` is their ``MapAnalysis``, None without ``stats``"""
    if blend not in ("crop", "average"):
        raise ValueError(f"blend {blend!r}: use 'crop' or 'average'")
    members = getattr(inference, "members", None)
    if overlap or tta is not None or members is not None:
        views = None if tta is None else tta_views(tta)
        _check_overlap(subtile, overlap)
        if world != 1:
            raise ValueError("infer_tile: overlap stitching, test-time augmentation and ensembles are the single-rank form "
                             "(shard by raster: infer_rasters)")
        vote = getattr(inference, "vote", "hard") if members is not None else None
        if return_probs and _no_probs(inference, overlap, blend, tta):
            raise ValueError("infer_tile: " + _no_probs(inference, overlap, blend, tta))
        models = list(members) if members is not None else [inference]
        if on_device is False or not all(hasattr(m, "run_windows") for m in models):
            raise ValueError("infer_tile: overlap stitching, test-time augmentation and ensembles run on the device and need "
                             "inference objects with run_windows")
        if arr_chw_u8.dtype != np.uint8:
            raise ValueError(f"infer_tile: the stitched device path reads a uint8 raster, got {arr_chw_u8.dtype}")
        return _infer_tile_stitched(inference, models, vote, arr_chw_u8, subtile, overlap, blend, batch_size, device,
                                    skip_blank, return_probs, views, request, decision)
    if return_probs:
        raise ValueError("infer_tile: " + _no_probs(inference, overlap, blend, tta))
    if tile_shape is None:
        h, w = arr_chw_u8.shape[1], arr_chw_u8.shape[2]
        if h <= 2048 and w <= 2048 and 2048 % subtile == 0:
            tile_shape = (2048, 2048)           # the reference's tile (tiler.py:63)
        else:
            tile_shape = (-(-h // subtile) * subtile, -(-w // subtile) * subtile)
    if on_device is None:
        on_device = (world == 1 and str(device).startswith("cuda") and torch.cuda.is_available()
                     and arr_chw_u8.dtype == np.uint8)
    if on_device:
        if world != 1:
            raise ValueError("infer_tile: the on-device split / merge is the single-rank form")
        return _infer_tile_on_device(inference, arr_chw_u8, subtile, batch_size, device, tile_shape, skip_blank,
                                     request)
    if skip_blank and bool(np.isin(arr_chw_u8[0], [0, 255]).all()):    # scripts/inference.py:60-62 is_valid_tile
        return None
    t = Tiler(tile_shape=tile_shape, subtile_shape=(subtile, subtile))
    t.load_array(arr_chw_u8)
    used = t.get_batches()
    batches = np.array_split(used, math.ceil(len(used) / batch_size), axis=0)
    outs: List[Optional[np.ndarray]] = [None] * len(batches)
    for j, b in enumerate(batches):
        if j % world != rank:
            continue
        u8 = torch.from_numpy(np.ascontiguousarray(b.transpose(0, 2, 3, 1)))     # [B,d,d,C] uint8
        outs[j] = inference.run_u8(u8, device=device).cpu().numpy()
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, [(j, o) for j, o in enumerate(outs) if o is not None], group=group)
        for lst in gathered:
            for j, o in lst:
                outs[j] = o
    t.put_batches(np.concatenate(outs, axis=0))
    if request is not None:
        st = t._analyse(request)            # before the map is read: a sieve changes it; attributes read t's raster
        return t.result, st
    return t.result


def _upload(inference, arr_chw_u8: np.ndarray, device: str, skip_blank: bool, request: Optional[MapAnalysis]):
    """the start of every device path: ONE uint8 H2D copy of the band planes the network reads (the N of an RGBN raster
    under an RGB model stays on the host), the request's maps next to it (``MapAnalysis.device_planes``) and ``skip_blank``'s
    ``is_valid_tile`` on the device: ``(x, (zones, against), raster)``, or None for a raster with only 0 / 255 in band 1.  With
    ``attributes`` the one copy carries ALL bands: ``raster`` is that tensor and ``x`` the view of its leading planes the network
    reads; without them ``raster`` is None"""
    C = arr_chw_u8.shape[0]
    nch = int(getattr(inference, "in_channels", C) or C)
    everything = request is not None and request.attributes is not None
    if 0 < nch < C and not everything:
        arr_chw_u8 = arr_chw_u8[:nch]
    x = torch.from_numpy(np.ascontiguousarray(arr_chw_u8)).to(device, non_blocking=True)
    raster = x if everything else None
    if everything and 0 < nch < C:
        x = x[:nch]
    planes = (None, None) if request is None else request.device_planes(arr_chw_u8.shape[1:], x.device)
    if skip_blank:
        from .. import ops
        if int(ops.band_has_data(x[0])) == 0:
            return None
    return x, planes, raster


def _infer_tile_on_device(inference, arr_chw_u8: np.ndarray, subtile: int, batch_size: int, device: str,
                          tile_shape: Tuple[int, int], skip_blank: bool = False, request=None):
    """single-rank form of ``infer_tile`` with the block split / merge on the device: ONE uint8 H2D copy of the raster, the
    sub-tiles of ``Tiler.get_batches`` (same ones, same row-major order: the [0:ceil(h/d), 0:ceil(w/d)] blocks of the
    zero-padded tile, reference tiler.py:121-134 + utils/data_handling.py:9-20) as a strided view -> NHWC uint8 batches
    -> ``run_u8`` -> class maps merged like ``unmake_blocks_vectorized`` -> ONE uint8 D2H copy of the cropped map."""
    C, h, w = arr_chw_u8.shape
    d = subtile
    if h > tile_shape[0] or w > tile_shape[1]:
        raise ValueError(f"raster {(h, w)} larger than the tile shape {tuple(tile_shape)}")
    if tile_shape[0] % d or tile_shape[1] % d:
        raise ValueError(f"Shapes unaligned: {tuple(tile_shape)} / {d}")
    nby, nbx = -(-h // d), -(-w // d)
    up = _upload(inference, arr_chw_u8, device, skip_blank, request)
    if up is None:
        return None
    x, planes, raster = up
    C = x.shape[0]
    if hasattr(inference, "run_blocks"):
        # round 3: split + zero padding + Normalize + NHWC in one gather per batch (dt_split_normalize_u8), no ATen passes
        outs = [inference.run_blocks(x, d, j, min(batch_size, nby * nbx - j)) for j in range(0, nby * nbx, batch_size)]
    else:
        if (nby * d, nbx * d) != (h, w):
            xp = torch.zeros((C, nby * d, nbx * d), dtype=torch.uint8, device=x.device)
            xp[:, :h, :w] = x
            x = xp
        blocks = x.view(C, nby, d, nbx, d).permute(1, 3, 2, 4, 0).contiguous().view(nby * nbx, d, d, C)
        outs = [inference.run_u8(blocks[j:j + batch_size], device=device) for j in range(0, nby * nbx, batch_size)]
    maps = (outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)).to(torch.uint8)
    merged = maps.view(nby, nbx, d, d).permute(0, 2, 1, 3).reshape(nby * d, nbx * d)
    return run_device(request, merged[:h, :w].contiguous(), None, planes, raster)


def _infer_tile_stitched(inference, models, vote: Optional[str], arr_chw_u8: np.ndarray, d: int, overlap: int, blend: str,
                         batch_size: int, device: str, skip_blank: bool, return_probs: bool, views, request=None,
                         decision=None):
    """``infer_tile`` on the window grid: overlapping windows, test-time augmentation (``views``: canonical pairs, or None
    for the plain window), an ensemble (``models``; ``vote`` None for a single model) and their combinations.  ONE uint8 H2D
    copy of the raster; per model and batch of windows one gather (``dt_window_normalize_u8``) + forward + one stitch kernel
    into a raster-sized buffer in HBM; ONE uint8 D2H copy of the map (plus the fp32 probabilities when asked for).  Batches
    run in ascending window order, which is what makes the accumulator independent of ``batch_size``.

    A model's own raster result: plain crop mode scatters the fused argmax (``stitch_classes``); everything else
    accumulates probabilities (``weight="ramp"`` for ``blend="average"``, ``weight="keep"`` for crop with views) and
    finalizes.  Hard vote: one ``ops.ensemble_vote`` over the members' raster maps.  Soft vote: ONE accumulator, members
    outer / window batches inner, no 1/M (finalize normalises) — each pixel's terms arrive model-major, windows ascending,
    views ascending, for every batch size.

    ``decision``: the probabilities are finalized as for ``return_probs`` and ``ops.decide_classes`` (a patch-wise decision:
    ``ops.decide_patchwise``) overwrites the arg-max plane before ``run_device``, which relabels the decided map itself;
    they leave the device only when ``return_probs`` asks."""
    from .. import ops
    _, h, w = arr_chw_u8.shape
    ny, nx, _ = window_grid(h, w, d, overlap)
    n = ny * nx
    up = _upload(inference, arr_chw_u8, device, skip_blank, request)
    if up is None:
        return None
    x, planes, raster = up
    keep_probs = return_probs or (request is not None and request.attributes is not None and request.attributes.confidence)
    want_probs = keep_probs or decision is not None
    kw = {} if views is None else {"views": views}   # a duck-typed run_windows without TTA need not take the keyword
    per = batch_size if views is None else max(1, batch_size // len(views))     # batch_size counts forward tiles
    weight = "ramp" if blend == "average" else "keep"

    def accumulate(model, acc):
        for j in range(0, n, per):
            logits = model.run_windows(x, d, overlap, j, min(per, n - j), want="logits", **kw)
            if acc is None:
                acc = torch.zeros((logits.shape[-3], h, w), dtype=torch.float32, device=x.device)
            ops.stitch_accumulate(logits, acc, overlap, j, views=views, weight=weight)
        return acc

    def class_map(model):
        if views is None and blend == "crop":
            out = torch.empty((h, w), dtype=torch.uint8, device=x.device)      # the kept regions tile it: every byte is written
            for j in range(0, n, batch_size):
                ops.stitch_classes(model.run_windows(x, d, overlap, j, min(batch_size, n - j), want="classes"), out, overlap, j)
            return out
        return ops.stitch_finalize(accumulate(model, None))

    if vote != "soft" and not want_probs:            # one map per model (probabilities under a hard vote were refused)
        maps = [class_map(m) for m in models]
        if len(maps) > 1:
            maps = [ops.ensemble_vote(torch.stack(maps, dim=0), int(inference.classes), dtype="uint8")[0]]
        return run_device(request, maps[0], None, planes, raster)
    acc = None
    for m in models:
        acc = accumulate(m, acc)
    if want_probs:
        classes, probs = ops.stitch_finalize(acc, want_probs=True)
        if decision is not None and decision.patchwise:
            ops.decide_patchwise(probs, decision, out=classes)
        elif decision is not None:
            ops.decide_classes(probs, decision, out=classes)
        return run_device(request, classes, probs if keep_probs else None, planes, raster, return_probs)
    return run_device(request, ops.stitch_finalize(acc), None, planes, raster)
