"""The case table of tests/unwritten_cases.py names every public wrapper of deadtrees_amd/ops.py that allocates with
torch.empty / empty_like / empty_strided / new_empty, directly or through one of the five shared helpers: a wrapper that
gains an allocation, or a new wrapper, fails here until a case runs it on poisoned memory (tests/test_unwritten_gpu.py).
The shapes of the cases have the row / slab form they are there for, by the library's own host queries.  Host only:
the source of ops.py and the library's queries (the idea of tests/test_grid_caps.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unwritten_cases as uc  # noqa: E402

uc.add_variant_cases()


def test_every_allocating_wrapper_has_a_case():
    wrappers = uc.allocating_wrappers()
    assert len(wrappers) >= 60 and "conv2d" in wrappers and "FlatAdam" in wrappers, sorted(wrappers)
    covered = {w for c in uc.CASES for w in c.wrappers}
    missing = sorted(set(wrappers) - covered)
    assert not missing, "wrappers of ops.py that allocate and have no case in tests/unwritten_cases.py: " + ", ".join(
        f"{w} ({', '.join(wrappers[w])})" for w in missing)
    unknown = sorted(covered - set(wrappers))
    assert not unknown, f"cases name wrappers that do not allocate (or do not exist): {unknown}"


def test_the_named_wrappers_and_helpers_exist():
    from deadtrees_amd import ops
    for name in uc.HELPERS:
        assert callable(getattr(ops, name)), name
    for c in uc.CASES:
        for w in c.wrappers:
            assert hasattr(ops, w), (c.name, w)


def test_the_scan_sees_what_it_should(tmp_path):
    src = tmp_path / "fake_ops.py"
    src.write_text("import torch\nimport numpy as np\n"
                   "def _helper(n):\n    return torch.empty(n)\n"
                   "def _rows_buffer(n):\n    return torch.empty(n)\n"
                   "def direct(x):\n    return torch.empty_like(x)\n"
                   "def through_helper(n):\n    return _rows_buffer(n)\n"
                   "def through_other(n):\n    return _helper(n)\n"
                   "def host(n):\n    return np.empty(n)\n"
                   "def method(x):\n    return x.new_empty(3)\n"
                   "class Holder:\n    def __init__(self):\n        self.t = torch.empty_strided((2,), (1,))\n")
    found = uc.allocating_wrappers(str(src))
    assert found == {"direct": ["empty_like"], "through_helper": ["_rows_buffer"], "method": ["new_empty"],
                     "Holder": ["empty_strided"]}, found
    sites = uc.allocation_sites(str(src))
    assert [(top, fn) for _, top, fn in sites] == [("_helper", "empty"), ("_rows_buffer", "empty"), ("direct", "empty_like"),
                                                   ("method", "new_empty"), ("Holder.__init__", "empty_strided")], sites


def test_case_names_are_unique_and_cuts_are_listed():
    names = [c.name for c in uc.CASES]
    assert len(set(names)) == len(names)
    for c in uc.CASES:
        assert (c.cut is None) == (c.name not in uc.CUTS), f"{c.name}: every cut is listed in CUTS with its reason"


@pytest.mark.parametrize("name,form", uc.FORMS, ids=[n for n, _ in uc.FORMS])
def test_case_shape_has_its_form(name, form):
    form()


def test_variant_cases_cover_the_kernel_configurations():
    import conv_variant_cases as cvc
    for prec, names in (("fp32", cvc.FP32_KEY), ("bf16", cvc.BF16_KEY)):
        want = {(k[names.index("tn")], k[names.index("ck")], k[6]) for k in cvc.cases()[prec] if k[0] != 4}
        picked = uc.variant_descriptors(prec)
        keys = {cvc.fp32_key(t) if prec == "fp32" else cvc.bf16_key(t) for _, t in picked}
        got = {(k[3 + 1], k[3 + 2], k[6]) for k in keys}
        assert want <= got, (prec, sorted(want - got))
        assert any(k[8] for k in keys) and any(k[9] for k in keys), "one split and one join case"
