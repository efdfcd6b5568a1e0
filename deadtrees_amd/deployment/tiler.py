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
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .outlines import outlines_geojson, polygonize, polygonize_host, write_outlines_geojson  # noqa: F401
from .overlaps import (PatchMatch, PatchOverlaps, PatchTracks, overlap_pairs_host, patch_overlaps)  # noqa: F401
from .patches import PatchConfig, PatchTable, check_patches  # noqa: F401  (the ``patches`` argument of infer_tile)


def check_outlines(outlines, config, who: str) -> bool:
    """the ``outlines`` argument of ``infer_tile`` / ``Tiler.stats`` -> bool; outlines without patches are a ``ValueError``"""
    if outlines is None:
        return False
    if not isinstance(outlines, bool):
        raise ValueError(f"{who}: outlines must be True, False or None, got {outlines!r}")
    if outlines and config is None:
        raise ValueError(f"{who}: outlines need patches (the outlines are those of the PatchTable's patches)")
    return outlines


def check_against(against, against_patches, config, shape, K, who: str):
    """the ``against`` / ``against_patches`` arguments of ``infer_tile`` / ``Tiler.stats`` -> ``(map, PatchConfig)``, or
    ``(None, None)`` when no map was given.  ``against`` without patches, on another grid, of another dtype or with a value
    >= K is a ``ValueError``; ``against_patches`` defaults to the connectivity of ``patches`` without a sieve"""
    from .overlaps import check_against_map
    if against is None:
        if against_patches is not None:
            raise ValueError(f"{who}: against_patches needs against")
        return None, None
    if config is None:
        raise ValueError(f"{who}: against needs patches (the overlaps are those of the PatchTable's patches)")
    if against_patches is None:
        against_patches = PatchConfig(config.connectivity)
    elif not isinstance(against_patches, PatchConfig):
        raise ValueError(f"{who}: against_patches must be a PatchConfig or None, got {against_patches!r}")
    return check_against_map(against, shape, int(K), who), against_patches


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
              against=None, against_patches=None):
        """``RasterStats`` of ``result`` (``stats.zonal_counts_host``): what ``infer_tile(..., stats=True)`` returns, for a
        caller of the reference's own ``get_batches`` / ``put_batches`` loop.  ``zones``: uint8 [h, w] on the raster's grid
        (``n_zones`` defaults to ``zones.max() + 1``) or a ``PolygonSet`` in its pixel coordinates (burnt by
        ``rasterize_host``; ``n_zones`` defaults to the largest value + 1); ``classes``: the model's class count.  ``patches`` (True or a
        ``PatchConfig``): the statistics carry the ``PatchTable`` of the map (``patches.patches_host``); a configuration
        that sieves changes ``result`` itself, and the counts are those of the sieved map.  ``outlines=True`` (needs
        ``patches``): the statistics also carry the patches' outlines (``outlines.polygonize_host`` on the final label
        plane), polygon ``k`` for row ``k`` of the table.  ``against`` (needs ``patches``): a uint8 class map on the raster's
        grid or a ``PolygonSet`` in its pixel coordinates (burnt with ``all_touched=True``), with ``against_patches`` its
        ``PatchConfig`` (default: the connectivity of ``patches``, no sieve): the statistics carry ``.overlaps``, the
        ``PatchOverlaps`` of that map (A) and the final map (B) (``deployment/overlaps.py``)"""
        from ..data.polygons import PolygonSet, rasterize_host
        from .outlines import outlines_from_labels
        from .overlaps import PatchOverlaps, overlap_pairs_host
        from .patches import labelled_patches_host
        from .stats import RasterStats, check_zones, zonal_counts_host
        if self._outdata is None:
            raise RuntimeError("Tiler: load_file / load_array first")
        config = check_patches(patches)
        outlines = check_outlines(outlines, config, "Tiler.stats")
        result = self.result
        against, against_config = check_against(against, against_patches, config, result.shape, classes, "Tiler.stats")
        zones, Z = check_zones(zones, result.shape, n_zones)
        if isinstance(zones, PolygonSet):
            zones = rasterize_host(zones, result.shape[0], result.shape[1])
        table = rings = pairs = None
        if config is not None:
            sieved, labels, table = labelled_patches_host(result, classes, config)
            if against is not None:
                if isinstance(against, PolygonSet):
                    against = rasterize_host(against, result.shape[0], result.shape[1], all_touched=True)
                _, labels_a, table_a = labelled_patches_host(against, classes, against_config)
                pairs = PatchOverlaps(table_a, table, *overlap_pairs_host(labels_a, labels))
            if outlines:
                rings = outlines_from_labels(labels, sieved, config.connectivity)
            if config.sieves:
                self._outdata[0:result.shape[0], 0:result.shape[1]] = sieved
                result = self.result
        return RasterStats(zonal_counts_host(np.ascontiguousarray(result), zones, classes, Z), patches=table,
                           outlines=rings, overlaps=pairs)

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
                  against_patches=None):
    """the directory loop of scripts/inference.py:71-115 over in-memory rasters (GeoTIFF I/O needs rioxarray, absent
    here): ``rasters`` yields ``array`` or ``(key, array)``; rank r of ``world`` takes rasters r, r + world, ... (tiles are
    independent: no collective).  Yields ``(key, class_map)`` in input order of the rank's share; rasters whose band 1
    holds only 0 / 255 (``is_valid_tile``, :60-62) are skipped like the reference does — ``(key, None)`` — without a
    forward pass (device reduction over the uploaded raster, ``ops.band_has_data``).  ``overlap`` / ``blend`` /
    ``return_probs`` / ``tta`` / ``stats`` / ``n_zones`` / ``patches`` / ``outlines``: as in ``infer_tile`` (every raster stays on its rank, so overlap
    needs no exchange); ``zones``: a callable ``key -> uint8 [h, w] array, PolygonSet or None``, or a mapping (a missing
    key is None); ``against``: the same for the map every raster is compared with (a uint8 array, a ``PolygonSet`` or
    None: that raster's statistics carry no overlaps), ``against_patches`` as in ``infer_tile``.
    The second item of every pair is whatever ``infer_tile`` returned: with ``stats=True`` ``(map, RasterStats)`` — the
    ``RasterStats`` of a rank's share add up (``+``) to that rank's part of the regional totals."""
    if zones is not None and not stats:
        raise ValueError("infer_rasters: zones need stats=True")
    if check_patches(patches) is not None and not stats:
        raise ValueError("infer_rasters: patches need stats=True")
    check_outlines(outlines, check_patches(patches), "infer_rasters")
    if against is not None and (not stats or check_patches(patches) is None):
        raise ValueError("infer_rasters: against needs stats=True and patches")
    if against is None and against_patches is not None:
        raise ValueError("infer_rasters: against_patches needs against")
    for i, item in enumerate(rasters):
        if i % world != rank:
            continue
        key, arr = item if isinstance(item, tuple) else (i, item)
        z = None if zones is None else zones(key) if callable(zones) else zones.get(key)
        other = None if against is None else against(key) if callable(against) else against.get(key)
        yield key, infer_tile(inference, arr, subtile=subtile, batch_size=batch_size, device=device, tile_shape=tile_shape,
                              skip_blank=skip_blank, overlap=overlap, blend=blend, return_probs=return_probs, tta=tta,
                              stats=stats, zones=z, n_zones=n_zones, patches=patches, outlines=outlines, against=other,
                              against_patches=None if other is None else against_patches)


def infer_tile(inference, arr_chw_u8: np.ndarray, subtile: int = 256, batch_size: int = 64, rank: int = 0,
               world: int = 1, device: str = "cuda", group=None, tile_shape: Optional[Tuple[int, int]] = None,
               on_device: Optional[bool] = None, skip_blank: bool = False, overlap: int = 0, blend: str = "crop",
               return_probs: bool = False, tta=None, stats: bool = False, zones=None, n_zones: Optional[int] = None,
               patches=None, outlines=None, against=None, against_patches=None):
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
    ``skip_blank`` is still None): the class counts of the map (``deployment/stats.py``), K = ``inference.classes``.
    ``zones``: a uint8 [h, w] array on the raster's grid (forest mask, land use, a previous year's map — the counts are then
    the year-to-year transition matrix) splits the counts by zone, ``n_zones`` (<= 8) defaults to ``zones.max() + 1``.  On
    every device path the zones are uploaded next to the raster and ONE ``ops.zonal_counts`` runs on the final device map
    before its download; the host path (``on_device=False``, ``world > 1``, CPU) counts the merged map with
    ``zonal_counts_host``.  The map is the one the call without ``stats`` returns.  ``zones`` may also be a ``PolygonSet``
    in the raster's pixel coordinates (``data/polygons.py``: forest masks and stand boundaries arrive as polygons; zone ids
    as values, 0 outside every polygon, ``n_zones`` defaults to the largest value + 1): on the device paths the plane is
    burnt on the device (``ops.rasterize_polygons``) in place of its upload, on the host path by ``rasterize_host``; maps
    and counts are those of the call with the burnt array.

    ``patches=True`` or a ``PatchConfig(connectivity=8, min_pixels=0)`` (needs ``stats=True``): the ``RasterStats`` carries
    the map's ``PatchTable`` as ``.patches`` (``deployment/patches.py``: one row per connected dead-tree patch).  On every
    device path the final map is labelled, measured and — with ``min_pixels > 1`` — sieved in HBM before the counts and the
    download (``ops.label_patches`` / ``patch_areas`` / ``sieve_patches`` / ``patch_table``); the host path runs the same
    contract in numpy / scipy.  With a sieve the returned map is the sieved one and ``counts`` are the counts of the
    RETURNED map; the probabilities of ``return_probs`` are not touched by the sieve.  With ``min_pixels <= 1`` the map is
    bit-identical to the call without ``patches``.

    ``outlines=True`` (needs ``patches``): the ``RasterStats`` also carries ``.outlines``, a ``PolygonSet`` on the raster's
    grid with one polygon per patch — polygon ``k`` is row ``k`` of ``.patches`` (``deployment/outlines.py``: exact ring
    tracing along the pixel edges; ``outlines_geojson`` writes them out).  On every device path they are traced from the
    final label plane, after the sieve, in HBM before the map leaves the device (``ops.patch_outlines``: only the four
    ``PolygonSet`` arrays are downloaded); the host path runs ``polygonize_host``.  The map, the counts and the table are
    those of the call without ``outlines``.

    ``against`` (needs ``stats=True`` and ``patches``): a map to compare the result with patch by patch — a uint8 [h, w]
    class map on the raster's grid with values < K (last year's map, a burnt annotation) or a ``PolygonSet`` in its pixel
    coordinates (the annotators' polygons; burnt with ``all_touched=True``, the rule of the training masks).  The
    ``RasterStats`` carries ``.overlaps``, a ``PatchOverlaps`` (``deployment/overlaps.py``): ``table_a`` the patches of
    ``against`` under ``against_patches`` (a ``PatchConfig``; default: the connectivity of ``patches``, no sieve),
    ``table_b`` the ``.patches`` of the final map, and one row per pair of patches that share a pixel — ``match()`` gives
    the crown-level accuracy, ``track()`` the year-to-year fate of every patch.  On every device path ``against`` is
    uploaded next to the raster (a ``PolygonSet`` is burnt in HBM instead), labelled, sieved if asked and tabled there, and
    ``ops.patch_overlaps`` runs on the two label planes before the map is downloaded; the host path runs
    ``overlap_pairs_host``.  The map, the counts, the table and the outlines are those of the call without ``against``."""
    if blend not in ("crop", "average"):
        raise ValueError(f"blend {blend!r}: use 'crop' or 'average'")
    want_stats = None
    config = check_patches(patches)
    outlines = check_outlines(outlines, config, "infer_tile")
    if not stats:
        if zones is not None or n_zones is not None:
            raise ValueError("infer_tile: zones / n_zones need stats=True")
        if config is not None:
            raise ValueError("infer_tile: patches need stats=True")
        if against is not None or against_patches is not None:
            raise ValueError("infer_tile: against / against_patches need stats=True")
    else:
        from .stats import check_zones
        zones, Z = check_zones(zones, np.shape(arr_chw_u8)[1:], n_zones)
        K = getattr(inference, "classes", None)
        if K is None:
            raise ValueError("infer_tile: stats=True needs an inference object with a `classes` count")
        against, against_patches = check_against(against, against_patches, config, np.shape(arr_chw_u8)[1:], K,
                                                 "infer_tile")
        want_stats = (zones, int(K), Z, config, outlines, against, against_patches)
    members = getattr(inference, "members", None)
    if overlap or tta is not None or members is not None:
        views = None if tta is None else tta_views(tta)
        _check_overlap(subtile, overlap)
        if world != 1:
            raise ValueError("infer_tile: overlap stitching, test-time augmentation and ensembles are the single-rank form "
                             "(shard by raster: infer_rasters)")
        vote = getattr(inference, "vote", "hard") if members is not None else None
        if return_probs and (blend != "average" or vote == "hard"):
            raise ValueError("infer_tile: return_probs needs blend='average' and, for an ensemble, vote='soft'")
        models = list(members) if members is not None else [inference]
        if on_device is False or not all(hasattr(m, "run_windows") for m in models):
            raise ValueError("infer_tile: overlap stitching, test-time augmentation and ensembles run on the device and need "
                             "inference objects with run_windows")
        if arr_chw_u8.dtype != np.uint8:
            raise ValueError(f"infer_tile: the stitched device path reads a uint8 raster, got {arr_chw_u8.dtype}")
        return _infer_tile_stitched(inference, models, vote, arr_chw_u8, subtile, overlap, blend, batch_size, device,
                                    skip_blank, return_probs, views, want_stats)
    if return_probs:
        raise ValueError("infer_tile: return_probs needs overlap > 0 and blend='average'")
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
                                     want_stats)
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
    if want_stats is not None:
        st = t.stats(*want_stats)           # before the map is read: a sieve changes it
        return t.result, st
    return t.result


def _upload(inference, arr_chw_u8: np.ndarray, device: str, skip_blank: bool, want_stats):
    """the start of every device path: ONE uint8 H2D copy of the band planes the network reads (the N of an RGBN raster
    under an RGB model stays on the host), the zones map of a ``stats=True`` call uploaded next to it (None without one;
    a ``PolygonSet`` is rasterised on the device instead),
    the ``against`` map alike (a ``PolygonSet`` is burnt with ``all_touched=True``),
    and ``skip_blank``'s ``is_valid_tile`` on the uploaded raster.  Returns ``(raster, (zones, against))`` on the device, or
    None for a raster with nothing but 0 / 255 in band 1"""
    C = arr_chw_u8.shape[0]
    nch = int(getattr(inference, "in_channels", C) or C)
    if 0 < nch < C:
        arr_chw_u8 = arr_chw_u8[:nch]
    x = torch.from_numpy(np.ascontiguousarray(arr_chw_u8)).to(device, non_blocking=True)
    zones_dev = against_dev = None
    if want_stats is not None and want_stats[0] is not None:
        from ..data.polygons import PolygonSet, rasterize
        if isinstance(want_stats[0], PolygonSet):          # burnt where it is read: the tables travel, not the plane
            zones_dev = rasterize(want_stats[0], arr_chw_u8.shape[1:], device=x.device)
        else:
            zones_dev = torch.from_numpy(np.ascontiguousarray(want_stats[0])).to(device, non_blocking=True)
    if want_stats is not None and want_stats[5] is not None:
        from ..data.polygons import PolygonSet, rasterize
        if isinstance(want_stats[5], PolygonSet):
            against_dev = rasterize(want_stats[5], arr_chw_u8.shape[1:], device=x.device, all_touched=True)
        else:                                              # (a copy: torch wraps writable memory only)
            against_dev = torch.from_numpy(np.array(want_stats[5], order="C")).to(device, non_blocking=True)
    if skip_blank:
        from .. import ops
        if int(ops.band_has_data(x[0])) == 0:
            return None
    return x, (zones_dev, against_dev)


def _download(out: torch.Tensor, probs: Optional[torch.Tensor], want_stats, planes):
    """the end of every device path: the D2H copy of the final map ``out`` (uint8 [h, w], contiguous) and of the
    probabilities when there are any.  ``planes``: ``_upload``'s (zones, against) on the device.  With ``want_stats`` =
    (zones, K, Z, patch config, outlines, against, its patch config) one ``ops.zonal_counts`` is enqueued
    on ``out`` BEFORE the download (no synchronisation of its own); the counts and the flag are read after the map has
    arrived.  With a patch configuration ``out`` is labelled, its patch areas are taken and — if the configuration sieves —
    it is sieved IN PLACE, all before the counts; the roots are compacted and measured behind the download (the compaction
    reads the row count back).  Labels, the area plane (reused as the root -> row plane) and the compaction's flags are
    the workspace: about 12 bytes per pixel next to the map.  With ``outlines`` the final label plane is traced behind the
    table (``ops.patch_outlines``: two more scalar read-backs, 4 bytes per pixel and 40 per boundary edge of workspace).
    With ``against`` that map is labelled, sieved if asked and tabled like ``out`` (its own label and area planes), and
    ``ops.patch_overlaps`` reads the two final label planes behind the tables: three more scalar read-backs, 8 bytes per
    1024 pixels and 12 per run of workspace"""
    if want_stats is None:
        return out.cpu().numpy() if probs is None else (out.cpu().numpy(), probs.cpu().numpy())
    from .. import ops
    from .stats import RasterStats
    _, K, Z, config, outlines, against, against_config = want_stats
    zones_dev, against_dev = planes
    labels = area = table = rings = pairs = None
    err = torch.zeros(1, dtype=torch.int32, device=out.device)
    if config is not None:
        labels, _ = ops.label_patches(out, K, config.connectivity, err=err)
        area = ops.patch_areas(labels)
        if config.sieves:
            ops.sieve_patches(out, labels, area, config.min_pixels)
    counts, _ = ops.zonal_counts(out, zones_dev, K, Z, err=err)
    host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True) if config is not None else None
    if host is not None:
        host.copy_(out, non_blocking=True)                      # enqueued; the table's read-back waits for it
        table = ops.patch_table(labels, out, area, reuse_area_plane=True)
        if outlines:
            rings = ops.patch_outlines(labels, out, config.connectivity)
        if against is not None:
            from .overlaps import PatchOverlaps, _device_patches
            labels_a, table_a = _device_patches(against_dev, K, against_config, err)
            pairs = PatchOverlaps(table_a, table, *ops.patch_overlaps(labels_a, labels))
        torch.cuda.current_stream(out.device).synchronize()
        result = (host.numpy(),)
    else:
        result = (out.cpu().numpy(),)
    if probs is not None:
        result += (probs.cpu().numpy(),)
    flag = int(err.cpu())
    if flag:          # cannot happen with checked zones: the map is an argmax over K classes
        raise RuntimeError(f"infer_tile: raster statistics met a value out of range (flag {flag}: 1 class >= {K}, "
                           f"2 zone >= {Z})")
    return result + (RasterStats(counts.cpu().numpy(), patches=table, outlines=rings, overlaps=pairs),)


def _infer_tile_on_device(inference, arr_chw_u8: np.ndarray, subtile: int, batch_size: int, device: str,
                          tile_shape: Tuple[int, int], skip_blank: bool = False, want_stats=None):
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
    up = _upload(inference, arr_chw_u8, device, skip_blank, want_stats)
    if up is None:
        return None
    x, planes = up
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
    return _download(merged[:h, :w].contiguous(), None, want_stats, planes)


def _infer_tile_stitched(inference, models, vote: Optional[str], arr_chw_u8: np.ndarray, d: int, overlap: int, blend: str,
                         batch_size: int, device: str, skip_blank: bool, return_probs: bool, views, want_stats=None):
    """``infer_tile`` on the window grid: overlapping windows, test-time augmentation (``views``: canonical pairs, or None
    for the plain window), an ensemble (``models``; ``vote`` None for a single model) and their combinations.  ONE uint8 H2D
    copy of the raster; per model and batch of windows one gather (``dt_window_normalize_u8``) + forward + one stitch kernel
    into a raster-sized buffer in HBM; ONE uint8 D2H copy of the map (plus the fp32 probabilities when asked for).  Batches
    run in ascending window order, which is what makes the accumulator independent of ``batch_size``.

    A model's own raster result: plain crop mode scatters the fused argmax (``stitch_classes``); everything else
    accumulates probabilities (``weight="ramp"`` for ``blend="average"``, ``weight="keep"`` for crop with views) and
    finalizes.  Hard vote: one ``ops.ensemble_vote`` over the members' raster maps.  Soft vote: ONE accumulator, members
    outer / window batches inner, no 1/M (finalize normalises) — each pixel's terms arrive model-major, windows ascending,
    views ascending, for every batch size."""
    from .. import ops
    _, h, w = arr_chw_u8.shape
    ny, nx, _ = window_grid(h, w, d, overlap)
    n = ny * nx
    up = _upload(inference, arr_chw_u8, device, skip_blank, want_stats)
    if up is None:
        return None
    x, planes = up
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

    if vote != "soft" and not return_probs:          # one map per model (return_probs under a hard vote was refused)
        maps = [class_map(m) for m in models]
        if len(maps) > 1:
            maps = [ops.ensemble_vote(torch.stack(maps, dim=0), int(inference.classes), dtype="uint8")[0]]
        return _download(maps[0], None, want_stats, planes)
    acc = None
    for m in models:
        acc = accumulate(m, acc)
    if return_probs:
        classes, probs = ops.stitch_finalize(acc, want_probs=True)
        return _download(classes, probs, want_stats, planes)
    return _download(ops.stitch_finalize(acc), None, want_stats, planes)
