"""Synthetic webdataset shards for the shard / pool tests: written with tarfile + PIL into a temporary directory, so no
binary fixture is committed."""
import io
import tarfile

import numpy as np
from PIL import Image


def tiff_bytes(arr: np.ndarray, compression=None) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="TIFF", **({"compression": compression} if compression else {}))
    return buf.getvalue()


def random_samples(rng, n, h, w, prefix, bands=4, labels=3):
    """[(key, image uint8 [h,w,bands], mask uint8 [h,w] in [0, labels), lu uint8 [h,w] in [0, 6), frac)]"""
    out = []
    for i in range(n):
        img = rng.integers(0, 256, (h, w, bands), dtype=np.uint8)
        mask = rng.integers(0, labels, (h, w)).astype(np.uint8)
        lu = rng.integers(0, 6, (h, w)).astype(np.uint8)
        out.append((f"{prefix}_{i:03d}", img, mask, lu, float(np.round((mask > 0).mean(), 6))))
    return out


def write_shard(path, samples, compression=None, skip=()):
    """samples as ``random_samples`` makes them; ``skip``: (key, field) pairs to leave out"""
    with tarfile.open(str(path), "w") as tar:
        for key, img, mask, lu, frac in samples:
            for field, data in (("rgbn.tif", tiff_bytes(img, compression)), ("mask.tif", tiff_bytes(mask, compression)),
                                ("lu.tif", tiff_bytes(lu, compression)), ("txt", repr(frac).encode())):
                if (key, field) in skip:
                    continue
                info = tarfile.TarInfo(f"{key}.{field}")
                info.size = len(data)
                tar.addfile(info, io.BytesIO(data))
    return str(path)


def stack(samples):
    """(images [n,h,w,4] with 255 as the fourth band of 3-band samples, masks, lu, keys, fracs)"""
    imgs = []
    for _, img, _, _, _ in samples:
        if img.shape[2] == 3:
            img = np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], axis=2)
        imgs.append(img)
    return (np.stack(imgs), np.stack([s[2] for s in samples]), np.stack([s[3] for s in samples]),
            [s[0] for s in samples], [s[4] for s in samples])
