"""What ``infer_tile`` / ``infer_rasters`` / ``Tiler.stats`` compute from a final class map — counts per zone, patch table,
outlines, overlaps with another map, nearest-patch distances, patch attributes — as ONE request (``MapAnalysis``, the only
place that checks the options' rules), one host runner and one device runner.  The results' contracts are those of
``stats`` / ``patches`` / ``outlines`` / ``overlaps`` / ``proximity`` / ``attributes``."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from ..data.polygons import PolygonSet, rasterize
from .attributes import AttributeConfig, attributes_of, check_attributes, check_raster
from .cover import MAX_SUMS, CoverGrid, GridConfig, check_grid, cover_grid_host
from .crowns import CrownConfig, CrownSplit, check_crowns
from .patches import PatchConfig, check_patches, labelled_patches_host
from .proximity import ProximityConfig, check_proximity, distances_of, gaps_of
from .stats import MAX_ZONES, RasterStats, zonal_counts_host


def check_zones(zones, shape, n_zones: Optional[int] = None):
    """the ``zones`` / ``n_zones`` arguments -> (uint8 [h, w] array, Z); ``ValueError`` for a wrong shape or dtype,
    ``n_zones`` outside 1..8 or smaller than ``zones.max() + 1``.  ``zones`` None -> (None, 1).  A ``PolygonSet`` in pixel
    coordinates (zone ids as values, 0 outside every polygon) is returned as it is, its largest value for ``zones.max()``"""
    if zones is None:
        if n_zones not in (None, 1):
            raise ValueError(f"n_zones={n_zones} needs a zones map (without one every pixel is zone 0)")
        return None, 1
    if isinstance(zones, PolygonSet):
        zones.tables()                              # raises for polygons that are still in world coordinates
        need = int(zones.values.max()) + 1 if len(zones) else 1
    else:
        zones = np.asarray(zones)
        if zones.dtype != np.uint8:
            raise ValueError(f"zones must be uint8, got {zones.dtype}")
        if tuple(zones.shape) != tuple(shape):
            raise ValueError(f"zones {tuple(zones.shape)} must lie on the raster's grid {tuple(shape)}")
        need = int(zones.max()) + 1
    Z = need if n_zones is None else int(n_zones)
    if not 1 <= Z <= MAX_ZONES:
        raise ValueError(f"n_zones must be in 1..{MAX_ZONES}, got {Z}")
    if Z < need:
        raise ValueError(f"n_zones={Z} is smaller than zones.max() + 1 = {need}")
    return zones, Z


def check_against_map(against, shape, K: int, who: str):
    """a map to compare with: a uint8 [h, w] class map on the grid ``shape`` with values < K, or a ``PolygonSet`` in pixel
    coordinates with values < K (returned as it is).  ``ValueError`` otherwise"""
    if isinstance(against, PolygonSet):
        against.tables()                            # raises for polygons that are still in world coordinates
        if len(against) and int(against.values.max()) >= K:
            raise ValueError(f"{who}: polygon value {int(against.values.max())} out of range (K={K})")
        return against
    m = np.asarray(against)
    if m.dtype != np.uint8:
        raise ValueError(f"{who}: the map must be uint8, got {m.dtype}")
    if m.ndim != 2 or m.size == 0 or (shape is not None and tuple(m.shape) != tuple(shape)):
        raise ValueError(f"{who}: the map {tuple(m.shape)} must lie on the raster's grid"
                         + ("" if shape is None else f" {tuple(shape)}"))
    if int(m.max()) >= K:
        raise ValueError(f"{who}: class value {int(m.max())} out of range (K={K})")
    return m


def map_plane(m, shape, all_touched: bool, device=None):
    """a checked map — uint8 [h, w] host array, ``PolygonSet`` or None — as the uint8 plane where it is read: a tensor on
    ``device``, or a numpy array on the host (``device`` None).  Polygons are burnt there (the tables travel, not the
    plane); an array is uploaded without waiting, from a copy unless torch can wrap it (contiguous and writable)"""
    if isinstance(m, PolygonSet):
        return rasterize(m, shape, device=device, all_touched=all_touched)
    if m is None or device is None:
        return m
    import torch
    m = np.ascontiguousarray(m)
    return torch.from_numpy(m if m.flags.writeable else m.copy()).to(device, non_blocking=True)


@dataclass(frozen=True, eq=False)
class MapAnalysis:
    """what a caller asked to be computed from a final class map.  ``K``: the model's class count; ``zones`` (uint8 [h, w]
    array, ``PolygonSet`` or None) and ``Z``: the counts are split by zone; ``patches``: the ``PatchConfig`` of the
    ``PatchTable``, or None; ``outlines``: the patches' outlines as well; ``against`` (array, ``PolygonSet`` or None) and
    ``against_patches``: the map the result is compared with, and its ``PatchConfig``; ``n_zones``: the caller's figure;
    ``distances`` / ``gaps``: the ``ProximityConfig`` of the distances to the patches of ``against`` / to the map's own other
    patches, or None; ``attributes``: the ``AttributeConfig`` of the patches' band statistics and confidence, or None — after
    ``bind`` with the index pairs of that raster written out; ``crowns`` / ``against_crowns``: the ``CrownConfig`` under which
    the patches of the map / of ``against`` are split into crowns behind the sieve (``deployment/crowns.py``), or None — with
    one, everything that follows the label plane is crown-level; ``grid``: the ``GridConfig`` of the map's ``CoverGrid``
    (``deployment/cover.py``), or None — after ``bind`` ``grid_edges`` holds its edge tables for that raster's shape.
    ``rules`` checks what depends on no raster, ``bind`` the maps of one raster, ``of`` both; ``stats=False`` gives None"""
    K: Optional[int]
    zones: object = None
    Z: int = 1
    patches: Optional[PatchConfig] = None
    outlines: bool = False
    against: object = None
    against_patches: Optional[PatchConfig] = None
    n_zones: Optional[int] = None
    distances: Optional[ProximityConfig] = None
    gaps: Optional[ProximityConfig] = None
    attributes: Optional[AttributeConfig] = None
    crowns: Optional[CrownConfig] = None
    against_crowns: Optional[CrownConfig] = None
    grid: Optional[GridConfig] = None
    grid_edges: Optional[tuple] = None

    @classmethod
    def rules(cls, who: str, K, stats: bool = True, zones=None, n_zones=None, patches=None, outlines=None, against=None,
              against_patches=None, distances=None, gaps=None, attributes=None, no_probs: Optional[str] = None,
              crowns=None, against_crowns=None, grid=None) -> Optional["MapAnalysis"]:
        """the options as ``infer_tile`` receives them -> a request without maps yet, or None without ``stats``; ``zones`` and
        ``against`` only say whether there are any (``infer_rasters`` passes its mappings).  ``ValueError``: an option without
        ``stats``, outlines, ``against``, ``gaps`` or ``attributes`` without patches, ``against_patches`` or ``distances`` without
        ``against``, a value of a wrong type, ``attributes`` with confidence in a call without probabilities (``no_probs``: what
        the caller's path would need to have some; None: it has), ``crowns`` without patches, ``against_crowns`` without
        ``against``, ``grid`` without ``stats``"""
        config = check_patches(patches)
        try:
            distances, gaps = check_proximity(distances, "distances"), check_proximity(gaps, "gaps")
            attributes = check_attributes(attributes)
            crowns, against_crowns = check_crowns(crowns), check_crowns(against_crowns, "against_crowns")
            grid = check_grid(grid)
        except ValueError as e:
            raise ValueError(f"{who}: {e}") from None
        if outlines is not None and not isinstance(outlines, bool):
            raise ValueError(f"{who}: outlines must be True, False or None, got {outlines!r}")
        if outlines and config is None:
            raise ValueError(f"{who}: outlines need patches (the outlines are those of the PatchTable's patches)")
        if not stats:
            if zones is not None or n_zones is not None:
                raise ValueError(f"{who}: zones / n_zones need stats=True")
            if config is not None:
                raise ValueError(f"{who}: patches need stats=True")
            if against is not None or against_patches is not None:
                raise ValueError(f"{who}: against / against_patches need stats=True")
            if distances is not None or gaps is not None:
                raise ValueError(f"{who}: distances / gaps need stats=True")
            if attributes is not None:
                raise ValueError(f"{who}: attributes need stats=True")
            if crowns is not None or against_crowns is not None:
                raise ValueError(f"{who}: crowns / against_crowns need stats=True")
            if grid is not None:
                raise ValueError(f"{who}: grid needs stats=True")
            return None
        if crowns is not None and config is None:
            raise ValueError(f"{who}: crowns need patches (the crowns are cut from the PatchTable's patches)")
        if against_crowns is not None and (config is None or against is None):
            raise ValueError(f"{who}: against_crowns needs patches and against (the crowns are cut from that map's patches)")
        if gaps is not None and config is None:
            raise ValueError(f"{who}: gaps need patches (the gaps are those of the PatchTable's patches)")
        if attributes is not None and config is None:
            raise ValueError(f"{who}: attributes need patches (the attributes are those of the PatchTable's patches)")
        if attributes is not None and attributes.confidence and no_probs is not None:
            raise ValueError(f"{who}: attributes with confidence=True need probabilities ({no_probs})")
        if distances is not None and against is None:
            raise ValueError(f"{who}: distances need against (they are measured to the patches of that map)")
        if against is None:
            if against_patches is not None:
                raise ValueError(f"{who}: against_patches needs against")
        elif config is None:
            raise ValueError(f"{who}: against needs patches (the overlaps are those of the PatchTable's patches)")
        elif against_patches is None:
            against_patches = PatchConfig(config.connectivity)
        elif not isinstance(against_patches, PatchConfig):
            raise ValueError(f"{who}: against_patches must be a PatchConfig or None, got {against_patches!r}")
        return cls(K=K, patches=config, outlines=bool(outlines), against_patches=against_patches, n_zones=n_zones,
                   distances=distances, gaps=gaps, attributes=attributes, crowns=crowns, against_crowns=against_crowns,
                   grid=grid)

    def bind(self, who: str, shape, zones=None, against=None, raster=None) -> "MapAnalysis":
        """the request of one raster of ``shape`` (h, w) and its maps, of the kinds ``rules`` was told of.  ``ValueError``: a map
        off the grid, not uint8 or with a value out of range; ``n_zones`` that does not fit the zones; no class count; with
        ``attributes`` a ``raster`` ([C, h, w]: only its dtype and shape are read) that is missing, not uint8, off the grid, of
        more than 8 bands, or without a band an index names; with ``grid`` a lattice whose tables for ``shape`` the contract
        refuses"""
        zones, Z = check_zones(zones, shape, self.n_zones)
        if self.K is None:
            raise ValueError(f"{who}: stats=True needs an inference object with a `classes` count")
        against = None if against is None else check_against_map(against, shape, int(self.K), who)
        attributes = self.attributes
        if attributes is not None:
            if raster is None:
                raise ValueError(f"{who}: attributes need the raster the map was made from")
            try:
                attributes = AttributeConfig(attributes.pairs(check_raster(raster, shape, "attributes")), attributes.confidence)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
        grid_edges = None
        if self.grid is not None:
            try:
                grid_edges = self.grid.edges(shape)
                if (len(grid_edges[1]) - 1) * (len(grid_edges[3]) - 1) * Z * int(self.K) > MAX_SUMS:
                    raise ValueError(f"grid: {len(grid_edges[1]) - 1} x {len(grid_edges[3]) - 1} cells of {Z} x {int(self.K)} "
                                     f"bins are more than {MAX_SUMS} sums")
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
        return replace(self, K=int(self.K), zones=zones, Z=Z, against=against, attributes=attributes, grid_edges=grid_edges,
                       against_patches=None if against is None else self.against_patches,
                       against_crowns=None if against is None else self.against_crowns,
                       distances=None if against is None else self.distances)

    @classmethod
    def of(cls, who: str, shape, K, zones=None, against=None, raster=None, **options) -> Optional["MapAnalysis"]:
        """``rules`` + ``bind``: the checked request of one raster, or None without ``stats``"""
        request = cls.rules(who, K, zones=zones, against=against, **options)
        return None if request is None else request.bind(who, shape, zones, against, raster)

    def device_planes(self, shape, device):
        """``(zones, against)`` as uint8 planes on ``device`` (None without one); polygons are burnt with ``all_touched=True``"""
        return map_plane(self.zones, shape, True, device), map_plane(self.against, shape, True, device)


def run_host(request: MapAnalysis, result: np.ndarray, raster=None, probs=None):
    """``(map, RasterStats)`` of a uint8 [h, w] host map in numpy / scipy: ``map`` is ``result``, or its sieved copy when the
    request sieves, and the counts are those of ``map``.  ``raster`` (uint8 [C, h, w]) and ``probs`` (fp32 [K, h, w]): what the
    request's ``attributes`` are read from, on the final label plane"""
    from .outlines import outlines_from_labels
    from .overlaps import PatchOverlaps, overlap_pairs_host
    K, config = request.K, request.patches
    zones = map_plane(request.zones, result.shape, True)
    table = rings = pairs = gaps = attributes = split = None
    if config is not None:
        if request.crowns is None:
            result, labels, table = labelled_patches_host(result, K, config)
        else:
            result, labels, table, split = labelled_patches_host(result, K, config, crowns=request.crowns)
        if request.gaps is not None:
            gaps = gaps_of(labels, table, request.gaps.limit2)
        if request.attributes is not None:
            attributes = attributes_of(labels, table, raster, result, probs, request.attributes)
        if request.against is not None:
            _, labels_a, table_a = labelled_patches_host(map_plane(request.against, result.shape, True), K,
                                                         request.against_patches, crowns=request.against_crowns)[:3]
            apart = (None if request.distances is None
                     else distances_of(labels_a, table_a, labels, table, request.distances.limit2))
            pairs = PatchOverlaps(table_a, table, *overlap_pairs_host(labels_a, labels), distances=apart)
        if request.outlines:
            rings = outlines_from_labels(labels, result, config.connectivity)
    counts = zonal_counts_host(np.ascontiguousarray(result), zones, K, request.Z)
    cover = None
    if request.grid_edges is not None:
        sums, _ = cover_grid_host(result, zones, K, request.Z, request.grid_edges[1], request.grid_edges[3])
        cover = CoverGrid.of(sums, request.grid_edges, result.shape, table)
    return result, RasterStats(counts, patches=table, outlines=rings, overlaps=pairs, gaps=gaps, attributes=attributes,
                               crowns=split, grid=cover)


class DeviceSplit:
    """what ``device_labels`` keeps of a split until the crown table is there: the label plane before the split, the
    per-crown depths and the flags of ``ops.split_patches``, all on the device; ``finish`` gathers them at the table's roots"""

    def __init__(self, labels_before, crown_depth, flags, config: CrownConfig):
        self.labels_before, self.crown_depth, self.flags, self.config = labels_before, crown_depth, flags, config

    def finish(self, table) -> CrownSplit:
        import torch
        root = torch.from_numpy(np.array(table.root)).to(self.crown_depth.device)
        parent = self.labels_before.view(-1)[root].to(torch.int64) - 1
        depth, flags = self.crown_depth[root].cpu().numpy(), self.flags.cpu().numpy()
        return CrownSplit(table, parent.cpu().numpy(), depth, not flags[1], self.config)


def device_labels(classes, K: int, config: PatchConfig, err=None, in_place: bool = False, areas: bool = True, crowns=None):
    """label -> areas -> (sieve) of a uint8 device map, no host synchronisation: ``(classes', labels, area plane, err)``.  A
    sieve writes ``classes`` itself with ``in_place``, else a clone; ``areas=False`` skips the plane when nothing sieves.
    With ``crowns`` (a ``CrownConfig``) ``ops.split_patches`` follows the sieve — it reads a few flags back per group of growth
    rounds —, ``labels`` is the crown plane, the area plane is recomputed on it, and a fifth item is the ``DeviceSplit``"""
    from .. import ops
    if config.sieves and not in_place:
        classes = classes.clone()
    labels, err = ops.label_patches(classes, K, config.connectivity, err=err)
    area = ops.patch_areas(labels) if areas or config.sieves else None
    if config.sieves:
        ops.sieve_patches(classes, labels, area, config.min_pixels)
    if crowns is None:
        return classes, labels, area, err
    before = labels
    labels, _, crown_depth, flags = ops.split_patches(classes, before, K, config.connectivity, crowns, err=err)
    return classes, labels, ops.patch_areas(labels), err, DeviceSplit(before, crown_depth, flags, crowns)


def device_patches(classes, K: int, config: PatchConfig, err, crowns=None):
    """``device_labels`` -> table of a uint8 device map the caller keeps: ``(labels, PatchTable)``; with ``crowns`` the crown
    plane, the crown table and, third, the ``CrownSplit``"""
    from .. import ops
    if crowns is None:
        classes, labels, area, _ = device_labels(classes, K, config, err)
        return labels, ops.patch_table(labels, classes, area, reuse_area_plane=True)
    classes, labels, area, _, split = device_labels(classes, K, config, err, crowns=crowns)
    table = ops.patch_table(labels, classes, area, reuse_area_plane=True)
    return labels, table, split.finish(table)


def run_device(request: Optional[MapAnalysis], out, probs=None, planes=(None, None), raster=None, return_probs: bool = True):
    """the end of every device path: the D2H copy of the final map ``out`` (uint8 [h, w], contiguous) and of the
    probabilities when there are any, with a request its ``RasterStats`` behind them: ``(map[, probs][, stats])`` as host
    arrays.  ``planes``: the request's ``device_planes``.  The order of the enqueued work is fixed: (1) with patches ``out``
    is labelled, measured and — if asked — sieved IN PLACE, and with ``crowns`` split behind the sieve (``ops.split_patches``
    reads its growth flags back once per group of rounds; the label plane is the crown plane from here on); (2) ONE
    ``ops.zonal_counts`` on ``out``, no synchronisation of its own, and with ``grid`` ONE ``ops.cover_grid`` on ``out`` and the
    same zones plane behind it (its two edge tables are uploaded, nothing is read back); (3) with patches the map leaves by a pinned,
    non-blocking copy (without them by ``out.cpu()``); (4) the roots
    are compacted and measured behind it (``ops.patch_table`` reads the row count back), and with ``gaps`` one
    ``ops.patch_proximity`` of the label plane against itself follows (no scalar read-back, its result is downloaded), and
    with ``attributes`` one ``ops.patch_attributes`` of the final label plane over ``raster`` (the uploaded uint8 [C, h, w]
    planes) and, with confidence, ``out`` and ``probs`` (no scalar read-back, its two tables are downloaded); (5)
    ``outlines`` traces the final label plane (two more scalar read-backs); (6) ``against`` is labelled, sieved on a clone if
    asked and tabled like ``out``, ``ops.patch_overlaps`` reads the two label planes (three more read-backs), and with
    ``distances`` two ``ops.patch_proximity`` calls, one per direction, read them again; (7) one stream synchronise, then
    the counts and the ``err`` flag are read.  Without ``gaps`` / ``distances`` / ``attributes`` nothing of theirs is enqueued.
    ``return_probs=False``: ``probs`` are there for the attributes only and stay on the device.  Workspace next
    to the map: about 12 bytes per pixel for the patches (labels, the area plane reused as the root -> row plane, the
    compaction's flags), as much again for ``against``; a proximity call holds 16 bytes per pixel while it runs (column
    tables and the root -> row plane), 28 for ``gaps``; the attributes hold 4 (their root -> row plane)"""
    if request is None:
        return out.cpu().numpy() if probs is None else (out.cpu().numpy(), probs.cpu().numpy())
    import torch
    from .. import ops
    from .overlaps import PatchOverlaps
    K, config = request.K, request.patches
    table = rings = pairs = gaps = attributes = split = None
    err = torch.zeros(1, dtype=torch.int32, device=out.device)
    if config is not None and request.crowns is None:
        _, labels, area, _ = device_labels(out, K, config, err, in_place=True)
    elif config is not None:
        _, labels, area, _, split = device_labels(out, K, config, err, in_place=True, crowns=request.crowns)
    counts, _ = ops.zonal_counts(out, planes[0], K, request.Z, err=err)
    cover = None
    if request.grid_edges is not None:
        cover, _ = ops.cover_grid(out, planes[0], K, request.Z, request.grid_edges[1], request.grid_edges[3], err=err)
    if config is not None:
        host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
        host.copy_(out, non_blocking=True)                      # enqueued; the table's read-back waits for it
        table = ops.patch_table(labels, out, area, reuse_area_plane=True)
        if split is not None:
            split = split.finish(table)
        if request.gaps is not None:
            gaps = gaps_of(labels, table, request.gaps.limit2, device=True)
        if request.attributes is not None:
            attributes = attributes_of(labels, table, raster, out, probs, request.attributes, device=True)
        if request.outlines:
            rings = ops.patch_outlines(labels, out, config.connectivity)
        if request.against is not None:
            labels_a, table_a = device_patches(planes[1], K, request.against_patches, err, request.against_crowns)[:2]
            rows = ops.patch_overlaps(labels_a, labels)
            apart = (None if request.distances is None
                     else distances_of(labels_a, table_a, labels, table, request.distances.limit2, device=True))
            pairs = PatchOverlaps(table_a, table, *rows, distances=apart)
        torch.cuda.current_stream(out.device).synchronize()
        result = (host.numpy(),)
    else:
        result = (out.cpu().numpy(),)
    if probs is not None and return_probs:
        result += (probs.cpu().numpy(),)
    flag = int(err.cpu())
    if flag:          # cannot happen with checked zones: the map is an argmax over K classes
        raise RuntimeError(f"infer_tile: raster statistics met a value out of range (flag {flag}: 1 class >= {K}, "
                           f"2 zone >= {request.Z})")
    if cover is not None:
        cover = CoverGrid.of(cover.cpu().numpy(), request.grid_edges, tuple(out.shape), table)
    return result + (RasterStats(counts.cpu().numpy(), patches=table, outlines=rings, overlaps=pairs, gaps=gaps,
                                 attributes=attributes, crowns=split, grid=cover),)
