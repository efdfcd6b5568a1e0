"""One convolution descriptor per kernel variant the dispatch table names, for the coverage test and the fp64 parity test.

The variant key of a descriptor comes from the library's host-only queries (dt_conv2d_config, dt_conv2d_uses_zi,
dt_conv2d_bf16_config): nothing here repeats a dispatch rule.  A small, fixed search over candidate shapes keeps, per key,
the cheapest descriptor (multiply-accumulates) among the most ragged ones: maps that are no multiple of any pixel tile,
input channels that leave a partial K chunk, output channels that leave the last channel tile half empty.  The 64-wide
tiles want at least 512 workgroups (the 512-pixel and LDS-DMA tiles 1024 / 256): the search gets there with the batch."""
import ctypes as C
import functools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("B", "Hin", "Win", "C0", "C1", "mode0", "Ho", "Wo", "Cout", "ksize", "stride", "pad", "cout_split", "accumulate")
FP32_KEY = ("ksize", "stride", "mode0", "tw", "tn", "ck", "uses_zi", "concat", "split", "accumulate")
BF16_KEY = ("ksize", "stride", "mode0", "tw", "tn", "ck", "mt", "concat", "split", "accumulate")

MAX_MACS = 2 * 10 ** 9          # of the fp64 CPU reference
MAX_TENSOR_BYTES = 64 * 2 ** 20   # of every device tensor

# bf16 variants no network row names with the default options, but which the default dispatch does pick off the table:
# the 512-pixel register-staged tiles (mt = 4) — where the LDS-DMA kernel takes a shape, it takes it first
EXTRA_BF16_KEYS = ((3, 1, 0, 32, 64, 16, 4, 0, 0, 0),)

# full-resolution (Hin, Win); the even ones also serve stride 2, up-sampling and zero insertion
MAPS = ((37, 70), (17, 65), (17, 33), (13, 11), (5, 7), (2, 2),
        (22, 70), (18, 66), (18, 34), (26, 22), (14, 12), (10, 14), (4, 4))
BATCHES = (1, 2, 3, 5, 8, 11, 15, 18, 22, 29, 32, 43, 57, 64, 86, 114, 128, 171, 228, 256, 342, 456, 512, 683, 1024)
# (C0, C1, penalty): 0 = full chunks and a partial one for every chunk size (8, 16, 32), 1 = several full chunks, or a
# partial chunk of the 8- and 16-channel steps only, 2 = a single full chunk
CIN = ((40, 0, 0), (48, 0, 0), (24, 0, 1), (64, 0, 1), (96, 0, 1), (16, 0, 2), (32, 0, 2))
CIN_CONCAT = ((32, 8, 0), (32, 24, 0), (16, 24, 0), (48, 24, 0), (32, 32, 1), (64, 32, 1), (16, 16, 2))
# (Cout, penalty): 0 = the last channel tile is half empty
COUT = ((48, 0), (96, 0), (160, 0), (16, 1), (32, 1), (64, 1), (128, 1), (192, 1))
SPLITS = (32, 64, 128)
FORMS = ((3, 1, 1), (1, 1, 0), (3, 2, 1), (1, 2, 0))     # (ksize, stride, pad)


def _lib():
    from deadtrees_amd import _lib
    return _lib


def descriptor(t):
    return _lib().ConvDesc(*t)


def make(B, Hin, Win, C0, C1, mode0, Cout, k, stride, pad, split=0, acc=0):
    """the descriptor as a tuple in FIELDS order, sizes from ops.conv_desc (the bf16 space-to-depth stem, ksize 4, pads 2
    before and 1 after: same-size output, as ops.stem_conv_bf16 builds it)"""
    from deadtrees_amd import ops
    d = ops.conv_desc(B, Hin, Win, C0, C1, mode0, Cout, k, stride, pad, split, acc)
    if k == 4:
        d.Ho, d.Wo = Hin, Win
    return tuple(getattr(d, f) for f in FIELDS)


def fp32_config(t):
    """(tw, tn, ck, uses_zi) or None when the fp32 validator refuses the descriptor"""
    lib, d = _lib().load(), descriptor(t)
    tw, tn, ck = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    if lib.dt_conv2d_config(C.byref(d), C.byref(tw), C.byref(tn), C.byref(ck)) != 0:
        return None
    return tw.value, tn.value, ck.value, int(lib.dt_conv2d_uses_zi(C.byref(d)))


def bf16_config(t):
    """(tw, tn, ck, mt) or None when the bf16 validator refuses the descriptor"""
    return _lib().bf16_config(descriptor(t))


def dma_default():
    """the value the bf16_dma option starts a process with: DT_BF16_DMA of the environment if it is 0, 1 or 2, else 1 (auto).
    The library has no query for the option; the tests that switch it put this value back, so a run started with the
    LDS-DMA kernel off stays so"""
    e = os.environ.get("DT_BF16_DMA", "")
    return int(e[0]) if e[:1] in ("0", "1", "2") else 1


def bf16_config_without_dma(t):
    """bf16_config with the LDS-DMA kernel switched off (dt_set_option bf16_dma 0), the option put back to dma_default()"""
    lib = _lib().load()
    try:
        _lib().check(lib.dt_set_option(b"bf16_dma", 0), "dt_set_option")
        return bf16_config(t)
    finally:
        _lib().check(lib.dt_set_option(b"bf16_dma", dma_default()), "dt_set_option")


def _key(t, cfg):
    d = dict(zip(FIELDS, t))
    return (d["ksize"], d["stride"], d["mode0"]) + tuple(cfg) + (int(d["C1"] > 0), int(d["cout_split"] > 0), d["accumulate"])


def fp32_key(t):
    cfg = fp32_config(t)
    return None if cfg is None else _key(t, cfg)


def bf16_key(t):
    cfg = bf16_config(t)
    return None if cfg is None else _key(t, cfg)


def golden_keys():
    """(fp32 keys, bf16 keys) of the network rows of tests/golden/dispatch_table.json: read from the file, no library"""
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_table.json")))
    assert tuple(table["desc_fields"]) == FIELDS
    q = table["queries"]
    i32, izi, ibf = q.index("dt_conv2d_config"), q.index("dt_conv2d_uses_zi"), q.index("dt_conv2d_bf16_config")
    f32, bf = set(), set()
    for t, ans in table["network"]:
        if ans[i32][0] == 0:
            f32.add(_key(t, ans[i32][1:] + [ans[izi]]))
        if ans[ibf][0] == 0:
            bf.add(_key(t, ans[ibf][1:]))
    return f32, bf


def macs(t):
    d = dict(zip(FIELDS, t))
    return d["B"] * d["Ho"] * d["Wo"] * d["ksize"] ** 2 * (d["C0"] + d["C1"]) * d["Cout"]


def largest_tensor_bytes(t, elem=4):
    """of the device tensors of a case with `elem`-byte activations: the sources as stored, the outputs, the weights"""
    d = dict(zip(FIELDS, t))
    sh = 1 if d["mode0"] else 0
    src0 = d["B"] * (d["Hin"] >> sh) * (d["Win"] >> sh) * d["C0"]
    src1 = d["B"] * d["Hin"] * d["Win"] * d["C1"]
    out = d["B"] * d["Ho"] * d["Wo"] * d["Cout"]
    return max(elem * src0, elem * src1, elem * out, 4 * d["ksize"] ** 2 * (d["C0"] + d["C1"]) * d["Cout"])


def within_budget(t):
    return macs(t) <= MAX_MACS and largest_tensor_bytes(t) < MAX_TENSOR_BYTES


def _shapes():
    """(penalty, descriptor without batch) of every candidate shape, in a fixed order"""
    for k, s, pad in FORMS:
        for mode0 in ((0, 1, 2) if s == 1 else (0,)):
            for H, W in MAPS:
                if (s == 2 or mode0) and (H % 2 or W % 2):
                    continue
                if s == 2 and H < 4:
                    continue      # at least 2 x 2 output pixels
                if s == 1 and mode0 == 0 and not (H % 2 or W % 2) and (H, W) != (4, 4):
                    continue      # plain stride-1 layers take the odd maps
                for c0, c1, pc in (CIN + (CIN_CONCAT if mode0 == 1 else ())):
                    for cout, po in COUT:
                        for split, acc in [(0, 0), (0, 1)] + [(sp, 0) for sp in SPLITS if sp < cout]:
                            if mode0 == 1 and (split or acc):
                                continue      # the up-sampling forward forms neither split nor join
                            if (mode0 == 2 or s == 2) and split:
                                continue
                            yield pc + po, (H, W, c0, c1, mode0, cout, k, s, pad if mode0 != 2 else k - 1 - pad, split, acc)
    for H, W in MAPS:      # the two stems: 7x7 / stride 2 (fp32) and its 4x4 space-to-depth form (bf16)
        yield 0, (H, W, 3, 0, 0, 64, 7, 2, 3, 0, 0)
        yield 0, (H, W, 16, 0, 0, 64, 4, 1, 2, 0, 0)


@functools.lru_cache(maxsize=None)
def cases():
    """{"fp32": {key: descriptor}, "bf16": {key: descriptor}, "bf16_extra": {...}, "off_table": {...}}: for every variant key the search meets,
    the best descriptor by (raggedness penalty, multiply-accumulates, the descriptor itself); the batch of an LDS-DMA
    case is large enough for the 64-wide register-staged tiles to take it when that kernel is off.  Host only and
    deterministic: the same list wherever the same library is loaded.

    "fp32" and "bf16" hold the keys of the golden table only, so they can fall short of the table but never exceed it: that
    a key of the library has a table row is what tests/test_dispatch_table.py and its descriptor list are for.  The keys
    the search met beyond the table (and beyond EXTRA_BF16_KEYS) are listed, without descriptors, under "off_table"""
    best = {"fp32": {}, "bf16": {}}
    for pen, sh in _shapes():
        seen = {"fp32": set(), "bf16": set()}
        for B in BATCHES:      # ascending cost: only the first descriptor of a key can be the cheapest of this shape
            t = make(B, *sh)
            if not within_budget(t):
                break
            for prec, kf in (("fp32", fp32_key), ("bf16", bf16_key)):
                key = kf(t)
                if key is None or key in seen[prec]:
                    continue
                if prec == "bf16" and key[6] == _lib().BF16_MT_DMA and bf16_config_without_dma(t)[1] != 64:
                    continue      # an LDS-DMA case also serves, with that kernel off, the register-staged 64-wide tiles
                seen[prec].add(key)
                rank = (pen, macs(t), t)
                if key not in best[prec] or rank < best[prec][key][0]:
                    best[prec][key] = (rank, t)
    f32_keys, bf_keys = golden_keys()
    out = {"fp32": {k: v[1] for k, v in sorted(best["fp32"].items()) if k in f32_keys},
           "bf16": {k: v[1] for k, v in sorted(best["bf16"].items()) if k in bf_keys},
           "bf16_extra": {k: v[1] for k, v in sorted(best["bf16"].items()) if k in EXTRA_BF16_KEYS},
           "off_table": {"fp32": sorted(set(best["fp32"]) - f32_keys),
                         "bf16": sorted(set(best["bf16"]) - bf_keys - set(EXTRA_BF16_KEYS))}}
    return out


def case_id(prec, key):
    names = FP32_KEY if prec == "fp32" else BF16_KEY
    d = dict(zip(names, key))
    s = f"{prec}-k{d['ksize']}s{d['stride']}m{d['mode0']}-tw{d['tw']}tn{d['tn']}ck{d['ck']}"
    s += f"zi{d['uses_zi']}" if prec == "fp32" else f"mt{d['mt']}"
    return s + ("-cat" if d["concat"] else "") + ("-split" if d["split"] else "") + ("-join" if d["accumulate"] else "")
