"""What the host side of the library decides — kernel family, tile configuration, statistics rows, workspace sizes, error
texts — equals the recorded table (tests/golden/dispatch_table.json, written by scripts/dump_dispatch_table.py).  Host
only: no GPU needed."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_dispatch_table_matches_golden(tmp_path):
    import __graft_entry__ as g
    g.build()
    import dump_dispatch_table as ddt
    # a fresh process with the default environment: the kernel switches are read once per process, and the table is
    # about the in-tree library
    env = {k: v for k, v in os.environ.items() if k not in ddt.SWITCHES and k != "DT_HIP_LIB"}
    out = tmp_path / "table.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "dump_dispatch_table.py"), "-o", str(out)],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.load(open(out))
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "dispatch_table.json")))
    assert sorted(got) == sorted(want)
    for key in ("desc_fields", "queries", "error_queries"):
        assert got[key] == want[key], key
    for part in ("network", "off_network", "rejected", "null", "sizes"):
        assert len(got[part]) == len(want[part]), part
        for i, (a, b) in enumerate(zip(got[part], want[part])):
            assert a == b, f"{part} row {i}: got {a}, recorded {b}"
    assert len(want["network"]) > 1000 and len(want["rejected"]) >= 30
