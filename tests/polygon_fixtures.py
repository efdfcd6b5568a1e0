"""Seeded polygon sets shared by tests/test_polygons_host.py and tests/test_polygons_gpu.py (pixel coordinates, as
``PolygonSet.from_polygons`` takes them), and the four known answers of the rasterisation contract."""
import functools

import numpy as np

# (name, polygons, (h, w), pixels burnt with all_touched=True, pixels burnt with all_touched=False)
KNOWN = [
    ("rectangle on the grid", [(1, [(3, 2), (9, 2), (9, 7), (3, 7)])], (12, 12), 30, 30),
    ("rectangle off the grid", [(1, [(3.5, 2.25), (9.01, 2.25), (9.01, 7), (3.5, 7)])], (12, 12), 35, None),
    ("sliver", [(1, [(1.1, 4.6), (10.9, 4.7), (10.9, 4.8)])], (12, 12), 10, 0),
    ("square with a hole", [(1, [(2, 2), (20, 2), (20, 20), (2, 20)], [[(6, 6), (16, 6), (16, 16), (6, 16)]])], (24, 24),
     224, 224),
]


def _star(rng, cx, cy, radius, k):
    """k vertices around (cx, cy) at sorted random angles, radii in 0.35 .. 1 of ``radius``"""
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, k))
    rad = radius * rng.uniform(0.35, 1.0, k)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def star_polygons(seed, n, h, w, values=(1, 2, 3), radius=(0.04, 0.22)):
    """n random star polygons over an h x w raster: centres up to 10 % outside it (some polygons reach outside, a few lie
    outside altogether), every third one with a hole around its centre"""
    rng = np.random.default_rng(seed)
    side = max(h, w)
    out = []
    for i in range(n):
        cx, cy = rng.uniform(-0.1 * w, 1.1 * w), rng.uniform(-0.1 * h, 1.1 * h)
        r = side * rng.uniform(*radius) + 0.6
        ext = _star(rng, cx, cy, r, int(rng.integers(5, 13)))
        holes = [_star(rng, cx, cy, 0.3 * r, int(rng.integers(3, 7)))] if i % 3 == 0 else []
        out.append((int(values[i % len(values)]), ext, holes))
    return out


def packed_polygons(seed, n, h, w, values=(1, 2, 3)):
    """n small polygons (3 .. 6 vertices, about 1 .. 2.5 pixels across) packed over the raster's first 32 x 64 tile, and
    twelve stars over the whole raster behind them"""
    rng = np.random.default_rng(seed)
    th, tw = min(h, 32), min(w, 64)
    out = []
    for i in range(n):
        cx, cy = rng.uniform(0.0, tw), rng.uniform(0.0, th)
        out.append((int(values[i % len(values)]), _star(rng, cx, cy, rng.uniform(0.5, 1.25), int(rng.integers(3, 7))), []))
    return out + star_polygons(seed + 1, 12, h, w, values)


def ring_polygon(seed, nv, h, w, value=2):
    """one ring of nv vertices around the raster's centre, reaching outside it here and there, with a hole of nv // 6"""
    rng = np.random.default_rng(seed)

    def wobbly(k, radius, depth):
        ang = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False)
        rad = radius * (1.0 + depth * np.sin(7 * ang) + 0.04 * rng.uniform(-1.0, 1.0, k))
        return np.stack([w / 2 + rad * w / 2 * np.cos(ang), h / 2 + rad * h / 2 * np.sin(ang)], axis=1)

    return [(value, wobbly(nv, 0.78, 0.25), [wobbly(max(nv // 6, 3), 0.3, 0.1)])]


@functools.lru_cache(maxsize=None)
def fixture(name, h, w):
    """the seeded sets of the GPU tests as a ``PolygonSet``: "stars" (60 star polygons, values 1..3, holes, some reaching
    outside), "packed" (400 small polygons over one tile: more than one chunk of the kernel's polygon list) and "ring"
    (3000 vertices and a hole: more than one chunk of its edge list, plus four small stars of the other values)"""
    from deadtrees_amd.data.polygons import PolygonSet
    if name == "stars":
        polys = star_polygons(11, 60, h, w)
    elif name == "packed":
        polys = packed_polygons(23, 400, h, w)
    elif name == "ring":
        polys = ring_polygon(5, 3000, h, w) + star_polygons(6, 4, h, w, values=(1, 3), radius=(0.08, 0.15))
    else:
        raise KeyError(name)
    return PolygonSet.from_polygons(polys)
