"""Golden fixtures kept in parts: ``<stem>.part<i>.npz`` (compressed), each holding whole arrays and staying under the
1 MiB limit for a committed file.  TEST INFRASTRUCTURE (the generators write them, the tests read them)."""
from __future__ import annotations

import glob
import os
import re

import numpy as np

PART_BYTES = 900_000      # raw bytes per part; random fp32 data does not compress, so this bounds the file size


def save_npz_parts(stem: str, data: dict) -> list:
    """name -> array, packed in insertion order into as few parts as PART_BYTES allows; stale parts are removed"""
    parts, cur, size = [], {}, 0
    for k, v in data.items():
        a = np.asarray(v)
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    for old in glob.glob(stem + ".part*.npz"):
        os.remove(old)
    paths = []
    for i, p in enumerate(parts):
        paths.append(f"{stem}.part{i}.npz")
        np.savez_compressed(paths[-1], **p)
    return paths


def load_npz_parts(stem: str) -> dict:
    """every array of ``<stem>.part*.npz`` -> one dict"""
    paths = sorted(glob.glob(stem + ".part*.npz"), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    if not paths:
        raise FileNotFoundError(stem + ".part*.npz")
    out = {}
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                assert k not in out, (p, k)
                out[k] = z[k]
    return out
