#!/usr/bin/env python
"""Record what the host side of libdeadtrees_hip.so decides, without a GPU.

Every sizing / selection query of the C ABI is host-only.  For a fixed, deterministic list of convolution descriptors
(the convolutions of the three decoders in their forward, data-gradient and weight-gradient forms, a grid of off-network
shapes, and descriptors that must be rejected) and a short list of plain sizes this script calls every such query and
writes the answers as JSON.  tests/test_dispatch_table.py compares the in-tree library row by row with the committed
table (tests/golden/dispatch_table.json), so a change of the host plumbing that alters a kernel choice, a buffer size or
an error text is seen on a machine without a GPU.

    python scripts/dump_dispatch_table.py [-o tests/golden/dispatch_table.json]

DT_HIP_LIB selects another build of the library (e.g. one made from an earlier commit).  The table is recorded with the
default environment: the DT_* kernel switches are cleared before the library is loaded.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the read-once "default on" switches of csrc/ and the run-time DMA option: the table is the DEFAULT behaviour
SWITCHES = ("DT_BF16_FUSE_UPSAMPLE_BWD", "DT_BF16_WGRAD_DMA", "DT_BF16_NARROW", "DT_FP32_SUBPIXEL_WGRAD",
            "DT_FP32_NARROW", "DT_FP32_SUBPIXEL", "DT_FP32_SUBPIXEL_DGRAD", "DT_FP32_WINO_UPSAMPLE_BWD",
            "DT_FP32_WINO_WGRAD_CO32", "DT_BF16_DMA")

DESC_FIELDS = ("B", "Hin", "Win", "C0", "C1", "mode0", "Ho", "Wo", "Cout", "ksize", "stride", "pad", "cout_split",
               "accumulate")

# descriptor queries, in the column order of a row: (name, kind); "cfg3"/"cfg4" fill int out-parameters
DESC_QUERIES = (
    ("dt_conv2d_stat_rows", "int"), ("dt_conv2d_config", "cfg3"), ("dt_conv2d_uses_zi", "int"),
    ("dt_conv2d_narrow_supported", "int"),
    ("dt_conv2d_winograd_supported", "int"), ("dt_conv2d_winograd_stat_rows", "int"),
    ("dt_conv2d_winograd_upsampled_dgrad_supported", "int"), ("dt_conv2d_winograd_upsampled_dgrad_rows", "int"),
    ("dt_conv2d_winograd_upsampled_dgrad_x_rows", "int"),
    ("dt_conv2d_upsampled_dgrad_supported", "int"), ("dt_conv2d_upsampled_dgrad_rows", "int"),
    ("dt_conv2d_wgrad_workspace", "int"), ("dt_conv2d_wgrad_winograd_supported", "int"),
    ("dt_conv2d_wgrad_winograd_workspace", "int"),
    ("dt_conv2d_bf16_config", "cfg4"), ("dt_conv2d_bf16_stat_rows", "int"), ("dt_conv2d_wgrad_bf16_workspace", "int"),
    ("dt_conv2d_bf16_upsampled_dgrad_supported", "int"),
)
# the queries whose failure leaves a message: one per validator of csrc/ (fp32, bf16, weight gradient, bf16 weight gradient)
ERROR_QUERIES = ("dt_conv2d_config", "dt_conv2d_bf16_config", "dt_conv2d_wgrad_workspace", "dt_conv2d_wgrad_bf16_workspace")

BATCHES = (1, 2, 32, 64)
SIZES = (64, 256, 512)


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def network_descriptors():
    """every convolution of build_spec() for the three decoders, in the forms the engines give the library"""
    sys.path.insert(0, ROOT)
    from deadtrees_amd.network.spec import build_spec

    shapes = set()   # (cin0, cin1, mode0, cout, k, stride, pad, log2 of the input down-scale)
    for dec in ("unet", "resunet", "unetplusplus"):
        s = build_spec(3, 2, dec)
        shapes.add((3, 0, 0, 64, 7, 2, 3, 0))
        shapes.add((4, 0, 0, 64, 7, 2, 3, 0))
        scale = 2   # after the stem (/2) and the max-pool (/2)
        for blocks in s.layers:
            for b in blocks:
                out_scale = scale + (1 if b.conv1.stride == 2 else 0)
                for c, sc in ((b.conv1, scale), (b.conv2, out_scale), (b.down, scale)):
                    if c is not None:
                        shapes.add((c.cin, 0, 0, c.cout, c.k, c.stride, c.pad, sc))
                scale = out_scale
        # decoder blocks: conv1 reads the up-sampled low map (mode0 = 1) concatenated with the skip; conv2 and the
        # ResUnet identity_conv read plain maps.  Block i of the plain decoders (node x_d_l of Unet++: i = l) writes at
        # 1/2^(4-i) of the input size
        for i, blk in enumerate(s.decoder):
            sc = 4 - (int(blk.name.split("_")[2]) if blk.name else i)
            c1 = blk.conv1
            shapes.add((blk.in_ch, blk.skip_ch, 1, c1.cout, c1.k, 1, c1.pad, sc))
            shapes.add((blk.conv2.cin, 0, 0, blk.conv2.cout, 3, 1, 1, sc))
            if blk.idc is not None:
                shapes.add((blk.in_ch, blk.skip_ch, 1, blk.idc.cout, 1, 1, 0, sc))
        shapes.add((s.head.cin, 0, 0, s.head.cout, 3, 1, 1, 0))
    out = []
    for (c0, c1, m0, cout, k, st, pad, sc) in sorted(shapes):
        for B in BATCHES:
            for size in SIZES:
                if B * size > 64 * 256:    # the B x size product is thinned: no 64 x 512 x 512 batch
                    continue
                hin = size >> sc
                if hin < 2 or (st == 2 and hin < 4):
                    continue
                ho = _out(hin, k, st, pad)
                # forward (and weight gradient: the same descriptor)
                out.append((B, hin, hin, c0, c1, m0, ho, ho, cout, k, st, pad, 0, 0))
                if k == 7:
                    continue
                cin = c0 + c1
                dpad = k - 1 - pad
                if st == 1:
                    # data gradient: channels swapped, flipped weights; plain, joined (accumulate) and, for a concat
                    # input, split into the up-sampled part and the skip part
                    out.append((B, ho, ho, cout, 0, 0, hin, hin, cin, k, 1, dpad, 0, 0))
                    out.append((B, ho, ho, cout, 0, 0, hin, hin, cin, k, 1, dpad, 0, 1))
                    if c1:
                        out.append((B, ho, ho, cout, 0, 0, hin, hin, cin, k, 1, dpad, c0, 0))
                    if m0 == 1 and c1 == 0:
                        # sub-pixel data gradient of an up-sampled input (asked with the forward descriptor, mode0 = 1)
                        out.append((B, hin, hin, cin, 0, 1, hin, hin, cout, k, 1, pad, 0, 0))
                else:
                    # stride 2: zero-insertion (transposed) form over the full-resolution map
                    out.append((B, hin, hin, cout, 0, 2, hin, hin, cin, k, 1, dpad, 0, 0))
                    out.append((B, hin, hin, cout, 0, 2, hin, hin, cin, k, 1, dpad, 0, 1))
        # the bf16 path's space-to-depth stem
    for B in BATCHES:
        for size in SIZES:
            if B * size > 64 * 256:
                continue
            h = size // 2
            out.append((B, h, h, 16, 0, 0, h, h, 64, 4, 1, 2, 0, 0))
    return out


def off_network_descriptors():
    """a small grid of shapes no decoder has: odd sizes, channels 8 / 12 / 48 / 96"""
    out = []
    for B in (1, 3):
        for h, w in ((17, 23), (33, 31), (64, 48), (100, 100)):
            for cin in (8, 12, 48, 96):
                for cout in (8, 12, 48, 96):
                    for k, st, pad in ((3, 1, 1), (3, 2, 1), (1, 1, 0), (1, 2, 0)):
                        out.append((B, h, w, cin, 0, 0, _out(h, k, st, pad), _out(w, k, st, pad), cout, k, st, pad, 0, 0))
            for cin, c1 in ((16, 8), (32, 48), (48, 96), (96, 32)):
                if h % 2 == 0 and w % 2 == 0:
                    out.append((B, h, w, cin, c1, 1, h, w, 48, 3, 1, 1, 0, 0))
                    out.append((B, h, w, cin, 0, 2, h, w, 96, 3, 1, 1, 32, 0))
    return out


def rejected_descriptors():
    """descriptors some validator of csrc/ refuses: one per DT_REQUIRE of the four validators, and pairs that break two
    rules at once (the first message reported is part of the behaviour)"""
    ok = dict(B=2, Hin=64, Win=64, C0=64, C1=0, mode0=0, Ho=64, Wo=64, Cout=64, ksize=3, stride=1, pad=1, cout_split=0,
              accumulate=0)

    def d(**kw):
        v = dict(ok)
        v.update(kw)
        return tuple(v[f] for f in DESC_FIELDS)

    return [
        d(B=0), d(Hin=0, Ho=0), d(Win=-1), d(C0=0), d(C1=-8), d(Cout=0),
        d(ksize=5, pad=2), d(ksize=2, pad=0, Ho=63, Wo=63), d(stride=3, Ho=22, Wo=22), d(stride=0),
        d(mode0=3), d(mode0=-1), d(mode0=2, C0=64),
        d(mode0=1, Hin=63, Win=63, Ho=63, Wo=63), d(mode0=2, Hin=64, Win=33, Ho=64, Wo=33),
        d(Ho=65), d(Wo=63), d(pad=0),
        d(C0=24, C1=16), d(C0=16, C1=32), d(C0=48, C1=16),
        d(cout_split=16), d(cout_split=64), d(cout_split=96), d(cout_split=48, Cout=128),
        d(ksize=7, stride=2, pad=3, Ho=32, Wo=32, C0=8), d(ksize=7, stride=1, pad=3, C0=3),
        d(ksize=7, stride=2, pad=3, Ho=32, Wo=32, C0=3, C1=4), d(ksize=7, stride=2, pad=3, Ho=32, Wo=32, C0=3, mode0=1),
        d(C0=12), d(C0=6), d(Cout=12), d(Cout=6), d(C0=64, C1=4), d(C0=3),
        # the space-to-depth stem of the bf16 path (ksize 4) with one rule broken each
        d(ksize=4, pad=2, C0=16, Cout=64, stride=2), d(ksize=4, pad=1, C0=16, Cout=64), d(ksize=4, pad=2, C0=32, Cout=64),
        d(ksize=4, pad=2, C0=16, Cout=48), d(ksize=4, pad=2, C0=16, Cout=32), d(ksize=4, pad=2, C0=16, Cout=64, Hin=16, Win=16, Ho=16, Wo=16),
        d(ksize=4, pad=2, C0=16, Cout=64, accumulate=1), d(ksize=4, pad=2, C0=16, Cout=64, Ho=65),
        # two rules at once: which message comes first
        d(Ho=65, cout_split=16), d(mode0=3, Ho=65), d(C0=24, C1=16, mode0=3), d(ksize=5, pad=2, C0=12),
        d(C0=12, Ho=65), d(mode0=1, Hin=63, Win=63, Ho=64, Wo=64), d(B=0, ksize=5), d(ksize=7, stride=2, pad=3, Ho=33, C0=8),
    ]


def plain_sizes(lib):
    """the size queries that take plain numbers"""
    rows = []
    for P in (1, 7, 64, 2048, 40000):
        for Cc in (16, 64, 512):
            rows.append(["dt_bn_stats_floats", P, Cc, lib.dt_bn_stats_floats(P, Cc)])
    for n in (1, 255, 4096, 64 * 64 * 64, 32 * 256 * 256, 64 * 512 * 512):
        rows.append(["dt_bn_bwd_rows_bf16", n, lib.dt_bn_bwd_rows_bf16(n)])
        rows.append(["dt_sumsq_rows", n, lib.dt_sumsq_rows(n)])
        for Cc in (16, 64, 512):
            rows.append(["dt_bn_bwd_rows", n, Cc, lib.dt_bn_bwd_rows(n, Cc)])
            rows.append(["dt_bn_bwd_red_floats", n, Cc, lib.dt_bn_bwd_red_floats(n, Cc)])
            rows.append(["dt_channel_sums_workspace", n, Cc, lib.dt_channel_sums_workspace(n, Cc)])
            rows.append(["dt_channel_sums_bf16_workspace", n, Cc, lib.dt_channel_sums_bf16_workspace(n, Cc)])
    for B in (1, 2, 32, 64):
        for H, W in ((8, 8), (15, 16), (64, 64), (256, 256), (512, 512)):
            rows.append(["dt_head_bwd_rows", B, H, W, lib.dt_head_bwd_rows(B, H, W)])
            for K in (1, 2, 3):
                rows.append(["dt_head_bwd_red_floats", B, H, W, 16, K, lib.dt_head_bwd_red_floats(B, H, W, 16, K)])
            for Cc in (8, 12, 16, 64, 96, 256, 2048):
                for name in ("dt_maxpool3x3s2_bwd_bn_rows", "dt_maxpool3x3s2_bwd_bn_bf16_rows", "dt_upsample2x_bwd_bn_rows",
                             "dt_upsample2x_bwd_bn_bf16_rows"):
                    rows.append([name, B, H, W, Cc, getattr(lib, name)(B, H, W, Cc)])
    return rows


def _query(lib, name, kind, desc):
    if name == "dt_conv2d_wgrad_bf16_workspace" and (min(desc.B, desc.Hin, desc.Win, desc.C0, desc.Cout) <= 0 or desc.C1 < 0):
        return None   # this validator has no "bad sizes" rule and the sizing divides by the sizes: not asked
    fn = getattr(lib, name)
    if kind == "int":
        return int(fn(C.byref(desc)))
    outs = [C.c_int(-1) for _ in range(3 if kind == "cfg3" else 4)]
    rc = fn(C.byref(desc), *[C.byref(o) for o in outs])
    return [int(rc)] + [o.value for o in outs]


def _family(answers):
    """the kernel family of the fp32 forward / bf16 forward of a row (for the summary only)"""
    q = dict(zip((n for n, _ in DESC_QUERIES), answers))
    fams = []
    rc, tw, tn, ck = q["dt_conv2d_config"]
    if rc == 0:
        if q["dt_conv2d_winograd_supported"]:
            fams.append("winograd")
        if ck >= 1000:
            fams.append("narrow")
        elif tn == 16:
            fams.append("n16")
        elif q["dt_conv2d_uses_zi"]:
            fams.append("zero-insertion")
        elif ck == 4:
            fams.append("stem")
        else:
            fams.append("tiled")
    brc, _, _, _, mt = q["dt_conv2d_bf16_config"]
    if brc == 0:
        from deadtrees_amd._lib import BF16_MT_DMA, BF16_MT_NARROW
        fams.append({BF16_MT_DMA: "bf16 lds-dma", BF16_MT_NARROW: "bf16 narrow", 4: "bf16 512-pixel"}.get(mt, "bf16 tiled"))
    if q["dt_conv2d_wgrad_winograd_supported"]:
        fams.append("winograd wgrad")
    return fams


def build_table():
    for k in SWITCHES:
        os.environ.pop(k, None)
    sys.path.insert(0, ROOT)
    from deadtrees_amd import _lib
    lib = _lib.load()

    def uniq(seq):
        seen, out = set(), []
        for t in seq:
            if t not in seen:
                seen.add(t)
                out.append(t)
        return out

    parts = (("network", uniq(network_descriptors())), ("off_network", uniq(off_network_descriptors())),
             ("rejected", uniq(rejected_descriptors())))
    table = {"desc_fields": list(DESC_FIELDS), "queries": [n for n, _ in DESC_QUERIES],
             "error_queries": list(ERROR_QUERIES)}
    counts = {}
    for part, descs in parts:
        rows = []
        for t in descs:
            desc = _lib.ConvDesc(*t)
            if part == "rejected":
                # only the queries that go through a validator: the others trust their caller with the sizes
                ans, errs = [], []
                for n in ERROR_QUERIES:
                    r = _query(lib, n, dict(DESC_QUERIES)[n], desc)
                    failed = r is not None and ((r[0] != 0) if isinstance(r, list) else (r == 0))
                    ans.append(r)
                    errs.append(lib.dt_last_error().decode() if failed else None)
                row = [list(t), ans, errs]
            else:
                ans = [_query(lib, n, k, desc) for n, k in DESC_QUERIES]
                row = [list(t), ans]
                for f in _family(ans):
                    counts[f] = counts.get(f, 0) + 1
            rows.append(row)
        table[part] = rows
    # the null descriptor: every validator's first rule
    null = C.POINTER(_lib.ConvDesc)()
    table["null"] = []
    for n in ERROR_QUERIES:
        kind = dict(DESC_QUERIES)[n]
        outs = [C.byref(C.c_int(-1)) for _ in range({"int": 0, "cfg3": 3, "cfg4": 4}[kind])]
        table["null"].append([n, int(getattr(lib, n)(null, *outs)), lib.dt_last_error().decode()])
    table["sizes"] = plain_sizes(lib)
    return table, counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output", default=None, help="write the table here (default: print a summary only)")
    args = ap.parse_args()
    table, counts = build_table()
    n = {k: len(table[k]) for k in ("network", "off_network", "rejected", "null", "sizes")}
    print("rows:", json.dumps(n), file=sys.stderr)
    print("accepted descriptors per family:", json.dumps(counts, sort_keys=True), file=sys.stderr)
    if args.output:
        with open(args.output, "w") as f:
            f.write("{\n")
            keys = list(table)
            for i, k in enumerate(keys):
                v = table[k]
                f.write(f' "{k}": ')
                if k in ("network", "off_network", "rejected", "null", "sizes"):
                    f.write("[\n" + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in v) + "\n ]")
                else:
                    f.write(json.dumps(v))
                f.write(",\n" if i + 1 < len(keys) else "\n")
            f.write("}\n")


if __name__ == "__main__":
    main()
