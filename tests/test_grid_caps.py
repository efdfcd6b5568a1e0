"""The inventory of capped launches (tests/grid_cap_cases.py) names exactly the capped launches the sources have: every
``dt_ew_grid(`` / ``dt_slice_grid(`` call and every ``if (g > N) g = N;`` clamp of deadtrees_amd/csrc, attributed to its
enclosing function.  A kernel that gains a capped grid, or a cap that changes, fails here until a row names a GPU case that
runs it past the cap (the idea of tests/test_conv_variant_coverage.py).  Host only: sources and the library's grid queries."""
import collections
import glob
import os
import re

import pytest

import grid_cap_cases as gcc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deadtrees_amd", "csrc")
# a definition starts in column 0 and names the function before its first parenthesis (after __launch_bounds__(..))
FUNC = re.compile(r"^(?!template|#|//|\}|typedef|using|struct|namespace)\S.*?\b(\w+)\s*\(")
CALL = re.compile(r"\b(dt_ew_grid|dt_slice_grid)\(")
# the clamp idiom: a bound that is an integer or a constant (or starts with one), neither a variable as in
# `if (p1 > n_pix) p1 = n_pix;` nor a float as in `if (c > 1.f) c = 1.f;`
CLAMP = re.compile(r"if \((\w+) > ((?:\d+(?![\d.])|[A-Z][A-Z0-9_]{2,})[^;]*?)\) \1 = \2;")


def _argument_text(text, start):
    """the text between the parenthesis at `start` and its partner"""
    depth = 0
    for j in range(start, len(text)):
        depth += {"(": 1, ")": -1}.get(text[j], 0)
        if depth == 0:
            return text[start + 1:j]
    raise AssertionError(text[start:start + 80])


def scan_sources(sources):
    """{file name: text} -> Counter of (file, enclosing function, cap text)"""
    found = collections.Counter()
    for name in sorted(sources):
        lines = [line.split("//")[0].rstrip() for line in sources[name].split("\n")]
        function = None
        for k, line in enumerate(lines):
            m = FUNC.match(re.sub(r"__launch_bounds__\(\w+\)\s*", "", line))
            if m and not line.endswith(";"):
                function = m.group(1)
            for m in CALL.finditer(line):
                if function == m.group(1):
                    continue                                      # the definition of the helper itself
                joined = line + " " + " ".join(t.strip() for t in lines[k + 1:k + 4])   # arguments may wrap
                found[(name, function, f"{m.group(1)}({_argument_text(joined, m.end() - 1)})")] += 1
            m = CLAMP.search(line)
            if m:
                found[(name, function, m.group(0))] += 1
    return found


def _sources():
    paths = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))
    assert len(paths) > 20
    out = {}
    for p in paths:
        with open(p) as f:
            out[os.path.basename(p)] = f.read()
    return out


def _table(rows):
    return collections.Counter((r.file, r.function, r.cap) for r in rows)


def _assert_same(found, table):
    missing, stale = found - table, table - found
    assert not missing, f"capped launches without a row in tests/grid_cap_cases.py: {sorted(missing)}"
    assert not stale, f"rows of tests/grid_cap_cases.py that no source line matches: {sorted(stale)}"


def test_the_table_names_every_capped_launch_of_the_sources():
    found = scan_sources(_sources())
    assert sum(found.values()) == 45                  # the count when this test was written
    _assert_same(found, _table(gcc.ROWS))
    for r in gcc.ROWS:
        assert r.tests and r.item and r.items, r
        for t in r.tests:                             # the named test exists
            path, name = t.split("::")
            with open(os.path.join(os.path.dirname(CSRC), "..", path)) as f:
                assert re.search(rf"^def {name}\(", f.read(), re.M), t


# rows whose third turn would need a tensor of 270 MB (one item of the bf16 2 x 2 backward is 64 bytes of input against a cap of
# 2,097,152 items): run past one cap only
PAST_ONE_CAP_ONLY = {"dt_maxpool3x3s2_bwd_bf16"}
# weight tensors have Cin * Cout elements per tap: whole workgroups; the ragged counts of these kernels are those of their
# small-shape tests
WHOLE_WORKGROUPS = {"dt_pack_dgrad_weights_bf16", "wgrad_impl"}


def _new_cases_only(r):
    return all(t.startswith(gcc.ABOVE) for t in r.tests)


def test_every_case_is_past_its_cap_and_the_library_reports_the_capped_grids():
    import __graft_entry__ as g
    g.build()
    from deadtrees_amd import _lib
    lib = _lib.load()
    values = {"EW_CAP": gcc.EW_CAP, "EW_CAP_WIDE": gcc.EW_CAP_WIDE, "ST_CAP": gcc.ST_CAP, "RS_CAP": gcc.RS_CAP}
    for r in gcc.ROWS:
        m = re.search(r", ([^,()]+)\)$", r.cap) if r.cap.startswith("dt_ew_grid") else None
        if m:                                         # the table's number is the value of the source's expression
            assert eval(m.group(1), {"__builtins__": {}}, values) == r.workgroups, r
        elif r.cap.startswith("dt_slice_grid"):
            assert r.workgroups == gcc.EW_CAP_WIDE, r
        cap_items = r.workgroups * r.per_wg
        assert all(n > cap_items for n in r.items), (r, cap_items)
        if _new_cases_only(r):                              # the new cases: one between one and two caps, one past two
            assert any(n > 2 * cap_items for n in r.items) or r.function in PAST_ONE_CAP_ONLY, (r, cap_items)
            assert any(n % 256 for n in r.items) or r.function in WHOLE_WORKGROUPS, r      # a ragged last workgroup
    # the fused BatchNorm-backward passes write one partial row per workgroup: the rows query is the capped grid
    for C, H, W in gcc.MAXPOOL_BN:
        assert lib.dt_maxpool3x3s2_bwd_bn_rows(1, H, W, C) == gcc.EW_CAP
    for C, H, W in gcc.MAXPOOL_BN_BF16:
        assert lib.dt_maxpool3x3s2_bwd_bn_bf16_rows(1, H, W, C) == gcc.EW_CAP
    for C, H, W in gcc.UPSAMPLE:
        assert lib.dt_upsample2x_bwd_bn_rows(1, H, W, C) == gcc.EW_CAP
    for C, H, W in gcc.UPSAMPLE_BF16:
        assert lib.dt_upsample2x_bwd_bn_bf16_rows(1, H, W, C) == gcc.EW_CAP
    assert lib.dt_upsample2x_bwd_bn_rows(1, 16, 16, 4) == 1 and lib.dt_maxpool3x3s2_bwd_bn_rows(1, 32, 32, 4) == 1
    # the row blocks of the two-pass reduction: 256 rows up to 524,288 pixels, larger blocks and at most 2048 of them beyond
    for entry, query, pixels, tests in gcc.ROW_BLOCK_ROWS:
        rows = (lambda n: lib.dt_bn_bwd_rows(n, 4)) if query == "dt_bn_bwd_rows" else lib.dt_bn_bwd_rows_bf16
        assert rows(gcc.ROW_BLOCK_PIXELS) == 2048 and rows(1000) == 4
        assert tests and len(pixels) >= 2
        for n in pixels:
            assert n > gcc.ROW_BLOCK_PIXELS
            block = -(-(-(-n // 2048)) // 256) * 256
            assert block > 256 and rows(n) == -(-n // block) <= 2048, (entry, n, rows(n))


def test_a_missing_row_and_a_new_capped_launch_are_noticed():
    """the comparison of the first test on a table with one row taken out, and on sources with one more capped launch"""
    sources = _sources()
    found = scan_sources(sources)
    for k in range(0, len(gcc.ROWS), 5):
        with pytest.raises(AssertionError, match="without a row"):
            _assert_same(found, _table(gcc.ROWS[:k] + gcc.ROWS[k + 1:]))
    more = dict(sources)
    more["optim.hip"] += ('\nextern "C" int dt_new_kernel(float* p, int64_t n, void* stream) {\n'
                          "  hipLaunchKernelGGL(new_kernel, dim3(dt_ew_grid(n, 1024)), dim3(256), 0, (hipStream_t)stream, p, n);\n"
                          "  return DT_OK;\n}\n")
    with pytest.raises(AssertionError, match=r"without a row.*dt_new_kernel.*dt_ew_grid\(n, 1024\)"):
        _assert_same(scan_sources(more), _table(gcc.ROWS))
    more = dict(sources)
    more["stitch.hip"] = more["stitch.hip"].replace("#define ST_CAP (256 * 16)", "#define ST_CAP (256 * 16)\nstatic int f(int g) {\n"
                                                    "  if (g > 512) g = 512;\n  return g;\n}")
    with pytest.raises(AssertionError, match=r"without a row.*'f', 'if \(g > 512\) g = 512;'"):
        _assert_same(scan_sources(more), _table(gcc.ROWS))
    changed = dict(sources)
    changed["patches.hip"] = changed["patches.hip"].replace("dt_ew_grid(n, 4096)", "dt_ew_grid(n, 2048)")
    with pytest.raises(AssertionError, match="without a row"):
        _assert_same(scan_sources(changed), _table(gcc.ROWS))
