"""Generate tests/golden/effunetpp_decoder*.part*.npz by EXECUTING the reference's EfficientUnet++ decoder unmodified.

TEST INFRASTRUCTURE.  Usage (where a checkout of the reference exists):   python tests/make_golden_effunetpp.py <reference root>

``deadtrees/network/extra/modules.py`` and ``extra/efficientunetplusplus/decoder.py`` are loaded BY FILE PATH (the pattern
of oracle/make_golden_unetpp.py) and ``EfficientUnetPlusPlusDecoder`` runs in eval mode on a seeded feature pyramid with
seeded, non-trivial convolution weights, BatchNorm parameters and running statistics — once per (squeeze, expansion) in
``CASES``.  Stored per case: the state_dict, the feature pyramid, the output.  Data only.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.golden import save_npz_parts  # noqa: E402
from tests.effunetpp_ref import randomize_  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "effunetpp_decoder")     # <OUT>_s{squeeze}e{expansion}.part*.npz
ENC_CH = (3, 16, 16, 32, 64, 128)
DEC_CH = (64, 32, 16, 16, 8)
CASES = ((1, 1), (2, 2))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(ref_root: str):
    ref = os.path.join(ref_root, "deadtrees", "network", "extra")
    for pkg in ("deadtrees", "deadtrees.network", "deadtrees.network.extra"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    md = _load("deadtrees.network.extra.modules", os.path.join(ref, "modules.py"))
    sys.modules["deadtrees.network.extra"].modules = md
    dec_mod = _load("deadtrees.network.extra.efficientunetplusplus.decoder",
                    os.path.join(ref, "efficientunetplusplus", "decoder.py"))
    for squeeze, expansion in CASES:
        torch.manual_seed(0)
        dec = dec_mod.EfficientUnetPlusPlusDecoder(encoder_channels=ENC_CH, decoder_channels=DEC_CH, n_blocks=5,
                                                   squeeze_ratio=squeeze, expansion_ratio=expansion)
        g = torch.Generator().manual_seed(10 * squeeze + expansion)
        randomize_(dec, g).eval()
        B, S = 2, 32
        feats = [torch.randn((B, c, S >> i, S >> i), generator=g) for i, c in enumerate(ENC_CH)]
        with torch.no_grad():
            out = dec(*feats)
        data = {"enc_ch": np.array(ENC_CH), "dec_ch": np.array(DEC_CH), "ratios": np.array([squeeze, expansion]),
                "out": out.numpy()}
        for i, f in enumerate(feats):
            if i > 0:
                data[f"feat{i}"] = f.numpy()
        for k, v in dec.state_dict().items():
            data[f"sd:{k}"] = v.numpy()
        paths = save_npz_parts(f"{OUT}_s{squeeze}e{expansion}", data)
        print("wrote", [os.path.basename(p) for p in paths], [os.path.getsize(p) for p in paths], "bytes;",
              len(dec.state_dict()), "state tensors; max|out|", float(out.abs().max()))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
