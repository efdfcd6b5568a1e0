"""Raster statistics: the numbers the reference takes from a predicted map, from ONE table of class counts per zone.

Three places of the reference compute them, each with its own passes over the raster on the host:

* ``scripts/computestats_inference.py``: per predicted raster ``np.unique(..., return_counts=True)`` -> ``cl_0 / cl_1 /
  cl_2``, ``total`` and ``deadarea_m2``; the per-year tables are joined on the tile name (``stats_row``, ``merge_years``,
  ``write_stats_csv``);
* ``scripts/aggregate_results.py``: the dead share of the forest area per class, from the raster and its forest mask
  (``forest_dead_percent``);
* ``deployment/server.py:112``: ``dead_tree_fraction`` (``RasterStats.dead_fraction``).

All of them are functions of ``counts[z, c]`` = the number of pixels of zone ``z`` (forest mask, land use, a previous
year's map) and class ``c``.  On the device path ``ops.zonal_counts`` fills the table from the map in HBM before the
download (``tiler.infer_tile(..., stats=True)``); ``zonal_counts_host`` is the same contract in numpy: the CPU path and the
tests' oracle.  numpy and the standard library only: rows and tables are plain Python (GeoTIFF / shapefile I/O needs
rioxarray / geopandas, which are absent here).
"""
from __future__ import annotations

import csv
from typing import Dict, Iterable, List, Mapping, Optional, Sequence

import numpy as np

# ground size of one pixel of the reference's orthophotos (computestats_inference.py:58), m^2
PIXEL_AREA_M2 = 0.200022269188281 * 0.200022454940277
MAX_CLASSES = 8
MAX_ZONES = 8


def zonal_counts_host(classes, zones=None, K: int = 3, Z: int = 1) -> np.ndarray:
    """int64 [Z, K]: ``counts[z, c]`` = the number of pixels with ``zones == z`` and ``classes == c`` — the contract of
    ``dt_zonal_counts_u8`` (2 <= K <= 8, 1 <= Z <= 8, without ``zones`` every pixel is zone 0 and Z must be 1), except that
    a value out of range is a ``ValueError`` that names its kind instead of a flag"""
    K, Z = int(K), int(Z)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"zonal_counts: K must be in 2..{MAX_CLASSES}, got {K}")
    if not 1 <= Z <= MAX_ZONES:
        raise ValueError(f"zonal_counts: Z must be in 1..{MAX_ZONES}, got {Z}")
    c = np.asarray(classes)
    if c.dtype != np.uint8:
        raise ValueError(f"zonal_counts: classes must be uint8, got {c.dtype}")
    if c.size == 0:
        raise ValueError("zonal_counts: empty map")
    if zones is None:
        if Z != 1:
            raise ValueError(f"zonal_counts: Z={Z} needs a zones map (without one every pixel is zone 0)")
        code = c.ravel().astype(np.intp)
    else:
        z = np.asarray(zones)
        if z.dtype != np.uint8:
            raise ValueError(f"zonal_counts: zones must be uint8, got {z.dtype}")
        if z.shape != c.shape:
            raise ValueError(f"zonal_counts: classes {c.shape} and zones {z.shape} must have the same shape")
        if int(z.max()) >= Z:
            raise ValueError(f"zonal_counts: zone value {int(z.max())} out of range (Z={Z})")
        code = z.ravel().astype(np.intp) * K + c.ravel()
    if int(c.max()) >= K:
        raise ValueError(f"zonal_counts: class value {int(c.max())} out of range (K={K})")
    return np.bincount(code, minlength=Z * K).astype(np.int64).reshape(Z, K)


class RasterStats:
    """the counts table of one raster (or of a sum of rasters) and the reference's figures read off it.  ``counts`` int64
    [Z, K]: rows zones, columns classes; class 0 is background, classes >= 1 are dead trees.  ``patches``: the raster's
    ``PatchTable`` (``deployment/patches.py``) when one was asked for, else None; a sum of rasters has none, because the
    tables of different rasters do not share a grid.  ``outlines``: the patches' outlines (``deployment/outlines.py``: a
    ``PolygonSet`` on the raster's grid, polygon ``k`` is row ``k`` of ``patches``) when they were asked for, else None;
    a sum of rasters has none either.  ``overlaps``: the ``PatchOverlaps`` (``deployment/overlaps.py``) of the map asked
    for with ``against`` (its ``table_a``) and this raster's patches (its ``table_b`` is ``patches``), else None; a sum of
    rasters has none.  ``gaps``: the ``PatchGaps`` (``deployment/proximity.py``: every patch's distance to the nearest other
    patch, aligned with ``patches``) when they were asked for, else None — then ``repr`` and ``==`` do not mention them; a sum
    of rasters has none.  ``attributes``: the ``PatchAttributes`` (``deployment/attributes.py``: band statistics, indices and
    confidence per patch, aligned with ``patches``), handled like ``gaps``.  ``crowns``: the ``CrownSplit``
    (``deployment/crowns.py``) when the patches were split into crowns — ``patches`` then has one row per crown, and everything
    aligned with it is crown-level —, handled like ``gaps``.  ``grid``: the ``CoverGrid`` (``deployment/cover.py``: area-weighted counts per cell of a coarser grid, with the
    patches binned by centroid when there are any) when one was asked for, else None — then ``repr`` and ``==`` do not mention
    it; a sum of rasters has none: ``CoverGrid.merge`` is the explicit route"""

    def __init__(self, counts, pixel_area_m2: float = PIXEL_AREA_M2, patches=None, outlines=None, overlaps=None, gaps=None,
                 attributes=None, crowns=None, grid=None):
        counts = np.array(counts, dtype=np.int64)
        if counts.ndim != 2 or counts.shape[0] < 1 or counts.shape[1] < 2:
            raise ValueError(f"RasterStats: counts must be [Z >= 1, K >= 2], got shape {counts.shape}")
        if (counts < 0).any():
            raise ValueError("RasterStats: negative count")
        counts.setflags(write=False)
        self._counts = counts
        self.pixel_area_m2 = float(pixel_area_m2)
        if patches is not None:
            from .patches import PatchTable
            if not isinstance(patches, PatchTable):
                raise ValueError(f"RasterStats: patches must be a PatchTable or None, got {type(patches).__name__}")
        self._patches = patches
        if outlines is not None:
            from ..data.polygons import PolygonSet
            if not isinstance(outlines, PolygonSet):
                raise ValueError(f"RasterStats: outlines must be a PolygonSet or None, got {type(outlines).__name__}")
            if patches is None or len(outlines) != patches.n:
                raise ValueError("RasterStats: outlines need the PatchTable they belong to (one polygon per row)")
        self._outlines = outlines
        if overlaps is not None:
            from .overlaps import PatchOverlaps
            if not isinstance(overlaps, PatchOverlaps):
                raise ValueError(f"RasterStats: overlaps must be a PatchOverlaps or None, got {type(overlaps).__name__}")
            if patches is None or overlaps.table_b != patches:
                raise ValueError("RasterStats: overlaps need the PatchTable they belong to (their table_b)")
        self._overlaps = overlaps
        if gaps is not None:
            from .proximity import PatchGaps
            if not isinstance(gaps, PatchGaps):
                raise ValueError(f"RasterStats: gaps must be a PatchGaps or None, got {type(gaps).__name__}")
            if patches is None or gaps.table != patches:
                raise ValueError("RasterStats: gaps need the PatchTable they belong to")
        self._gaps = gaps
        if attributes is not None:
            from .attributes import PatchAttributes
            if not isinstance(attributes, PatchAttributes):
                raise ValueError(f"RasterStats: attributes must be a PatchAttributes or None, got {type(attributes).__name__}")
            if patches is None or attributes.table != patches:
                raise ValueError("RasterStats: attributes need the PatchTable they belong to")
        self._attributes = attributes
        if crowns is not None:
            from .crowns import CrownSplit
            if not isinstance(crowns, CrownSplit):
                raise ValueError(f"RasterStats: crowns must be a CrownSplit or None, got {type(crowns).__name__}")
            if patches is None or crowns.table != patches:
                raise ValueError("RasterStats: crowns need the PatchTable they belong to")
        self._crowns = crowns
        if grid is not None:
            from .cover import CoverGrid
            if not isinstance(grid, CoverGrid):
                raise ValueError(f"RasterStats: grid must be a CoverGrid or None, got {type(grid).__name__}")
            if (grid.Z, grid.K) != counts.shape:
                raise ValueError(f"RasterStats: the grid's [Z, K] = {(grid.Z, grid.K)} must be that of the counts {counts.shape}")
        self._grid = grid

    @property
    def grid(self):
        return self._grid

    @property
    def crowns(self):
        return self._crowns

    @property
    def patches(self):
        return self._patches

    @property
    def outlines(self):
        return self._outlines

    @property
    def overlaps(self):
        return self._overlaps

    @property
    def gaps(self):
        return self._gaps

    @property
    def attributes(self):
        return self._attributes

    @property
    def counts(self) -> np.ndarray:
        return self._counts

    @property
    def class_counts(self) -> np.ndarray:
        """int64 [K]: pixels per class, over all zones"""
        return self._counts.sum(axis=0)

    @property
    def zone_pixels(self) -> np.ndarray:
        """int64 [Z]: pixels per zone, over all classes"""
        return self._counts.sum(axis=1)

    @property
    def total(self) -> int:
        return int(self._counts.sum())

    @property
    def dead_pixels(self) -> int:
        return int(self._counts[:, 1:].sum())

    @property
    def dead_fraction(self) -> float:
        """deployment/server.py:112 ``out.sum() / out.size`` of a 0 / 1 map: the share of dead pixels (classes >= 1)"""
        return self.dead_pixels / self.total if self.total else 0.0

    @property
    def dead_area_m2(self) -> float:
        """computestats_inference.py:57-59: ``((cl_1 + cl_2) * pixel area).round(1)``"""
        return float(np.round(self.dead_pixels * self.pixel_area_m2, 1))

    def __add__(self, other: "RasterStats") -> "RasterStats":
        if not isinstance(other, RasterStats):
            return NotImplemented
        if other._counts.shape != self._counts.shape or other.pixel_area_m2 != self.pixel_area_m2:
            raise ValueError(f"RasterStats: cannot add counts {other._counts.shape} to {self._counts.shape} "
                             "(or the pixel areas differ)")
        return RasterStats(self._counts + other._counts, self.pixel_area_m2)

    def __eq__(self, other) -> bool:
        if not isinstance(other, RasterStats):
            return NotImplemented
        if (self._patches is None) != (other._patches is None) or (self._outlines is None) != (other._outlines is None):
            return False
        if (self._overlaps is None) != (other._overlaps is None) or (self._gaps is None) != (other._gaps is None):
            return False
        if (self._attributes is None) != (other._attributes is None) or (self._crowns is None) != (other._crowns is None):
            return False
        if (self._grid is None) != (other._grid is None):
            return False
        return (self._counts.shape == other._counts.shape and bool((self._counts == other._counts).all())
                and self.pixel_area_m2 == other.pixel_area_m2
                and (self._patches is None or self._patches == other._patches)
                and (self._outlines is None or all(
                    np.array_equal(getattr(self._outlines, a), getattr(other._outlines, a))
                    for a in ("xy", "ring_offsets", "ring_polygon", "values")))
                and (self._overlaps is None or self._overlaps == other._overlaps)
                and (self._gaps is None or self._gaps == other._gaps)
                and (self._attributes is None or self._attributes == other._attributes)
                and (self._crowns is None or self._crowns == other._crowns)
                and (self._grid is None or self._grid == other._grid))

    __hash__ = None

    def __repr__(self) -> str:
        tail = "" if self._patches is None else f", patches={self._patches!r}"
        if self._outlines is not None:
            tail += f", outlines={self._outlines!r}"
        if self._overlaps is not None:
            tail += f", overlaps={self._overlaps!r}"
        if self._gaps is not None:
            tail += f", gaps={self._gaps!r}"
        if self._attributes is not None:
            tail += f", attributes={self._attributes!r}"
        if self._crowns is not None:
            tail += f", crowns={self._crowns!r}"
        if self._grid is not None:
            tail += f", grid={self._grid!r}"
        return f"RasterStats(counts={self._counts.tolist()}, pixel_area_m2={self.pixel_area_m2!r}{tail})"


# ---------------------------------------------------------------------- computestats_inference.py
REFERENCE_CLASSES = (0, 1, 2)       # computestats_inference.py:12


def stats_row(stats: RasterStats, tile) -> dict:
    """the row of computestats_inference.py:16-30 + :57-59: ``{"tile", "total", "cl_0", "cl_1", "cl_2", "deadarea_m2"}``.
    ``cl_*`` always come in class order with 0 for a class the model does not have (a two-class model has ``cl_2 = 0``); a
    model with more classes gets ``cl_3`` ... as well.  Deliberate difference: the reference's column order follows
    whichever classes ``np.unique`` met in the raster (missing ones are appended behind)."""
    cc = stats.class_counts
    row = {"tile": tile, "total": stats.total}
    for c in range(max(len(REFERENCE_CLASSES), len(cc))):
        row[f"cl_{c}"] = int(cc[c]) if c < len(cc) else 0
    row["deadarea_m2"] = stats.dead_area_m2
    return row


def merge_years(rows_by_year: Mapping[object, Iterable[dict]]) -> List[dict]:
    """the join of computestats_inference.py:63-75 over ``{year: [rows]}`` (rows of ``stats_row``), as a list of dicts with
    identical keys: an outer join on ``tile``; every column except ``tile`` gets the suffix ``_<year>``; there is ONE
    ``total``, that of the FIRST year given (None — an empty CSV field — for a tile that year lacks, as in the reference);
    columns: ``tile``, ``total``, then the years' columns in the order given.  Rows are sorted by ``tile`` like the keys of
    pandas' outer merge (tile names that do not compare with each other stay in order of first appearance)."""
    years = list(rows_by_year)
    if not years:
        return []
    tables, tiles, seen, columns = {}, [], set(), ["tile", "total"]
    for year in years:
        by_tile = {}
        for row in rows_by_year[year]:
            if row["tile"] in by_tile:
                raise ValueError(f"merge_years: tile {row['tile']!r} twice in year {year}")
            by_tile[row["tile"]] = row
            if row["tile"] not in seen:
                seen.add(row["tile"])
                tiles.append(row["tile"])
            for key in row:
                if key not in ("tile", "total") and f"{key}_{year}" not in columns:
                    columns.append(f"{key}_{year}")
        tables[year] = by_tile
    try:
        tiles = sorted(tiles)
    except TypeError:
        pass
    out = []
    for tile in tiles:
        first = tables[years[0]].get(tile)
        merged = dict.fromkeys(columns)
        merged["tile"] = tile
        merged["total"] = first["total"] if first is not None else None
        for year in years:
            row = tables[year].get(tile)
            if row is not None:
                for key, value in row.items():
                    if key not in ("tile", "total"):
                        merged[f"{key}_{year}"] = value
        out.append(merged)
    return out


def write_stats_csv(path, table: Sequence[dict]) -> None:
    """``predicted.stats.csv``: the table of ``merge_years`` (or a list of ``stats_row`` rows) through the ``csv`` module;
    None is an empty field"""
    table = list(table)
    fields = list(table[0]) if table else ["tile", "total"]
    with open(path, "w", newline="") as f:
        writer = csv.DictWriter(f, fieldnames=fields)
        writer.writeheader()
        for row in table:
            writer.writerow({k: ("" if v is None else v) for k, v in row.items()})


# ---------------------------------------------------------------------- aggregate_results.py
def forest_dead_percent(stats: RasterStats, limit: float = 10, forest_zone: int = 1,
                        label_weighted: bool = True) -> Optional[Dict[str, float]]:
    """aggregate_results.process_tile (:60-81) from the counts of a raster zoned by its forest mask: None when the raster
    has less than ``limit`` % forest (``zone_pixels[forest_zone] / total * 100 < limit``), else ``{"conifer", "broadleaf",
    "total"}``: dead conifers (class 1) and dead broadleaves (class 2) in percent of the forest pixels, and their sum.

    ``label_weighted=True`` (default) reproduces the reference as it is written: it sums label VALUES
    (``a[(a == c) & (b == 1)].sum()``), so its class-2 figure is TWICE the pixel share.  ``label_weighted=False`` gives
    plain pixel shares.  A two-class model has ``broadleaf = 0``."""
    counts = stats.counts
    if not 0 <= forest_zone < counts.shape[0]:
        raise ValueError(f"forest_dead_percent: forest_zone {forest_zone} outside the {counts.shape[0]} zones of the counts")
    forest = int(stats.zone_pixels[forest_zone])
    # the reference's own order of operations, (x / y) * 100, so that the floats agree to the last bit
    if forest == 0 or (forest / stats.total) * 100 < limit:      # no forest at all: nothing to take a share of
        return None
    shares = []
    for c in (1, 2):
        pixels = int(counts[forest_zone, c]) if c < counts.shape[1] else 0
        shares.append(((pixels * c if label_weighted else pixels) / forest) * 100)
    return {"conifer": shares[0], "broadleaf": shares[1], "total": shares[0] + shares[1]}
