"""Replay of tests/golden/scratch_ledger.json (tools/record_scratch_ledger.py): rmx_scratch_bytes after rmx_create and
after every call of the tool's script must be what the library of the commit in front of the buffer type
(radio-mapper_amd/csrc/dev_buf.hpp) returned -- the ledger that the buffers keep counts exactly what the scattered
+= / -= counted.  Small shapes that still grow every counted buffer."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_scratch_ledger  # noqa: E402

with open(record_scratch_ledger.TABLE) as _f:
    TABLE = json.load(_f)["steps"]


def test_table_is_the_tool_s_script():
    assert [r["name"] for r in TABLE] == record_scratch_ledger.names()
    grew = [b["scratch_bytes"] > a["scratch_bytes"] for a, b in zip(TABLE, TABLE[1:]) if a["name"].split(":")[0] == b["name"].split(":")[0]]
    assert sum(grew) >= 10, "the script is there to make the counted buffers grow"


def test_ledger_equals_the_recorded_one():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    got = record_scratch_ledger.run()
    for r, w in zip(got, TABLE):
        print("%-40s %14d %14d" % (r["name"], r["scratch_bytes"], w["scratch_bytes"]))
    assert got == TABLE
