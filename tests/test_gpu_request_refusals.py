"""Replay of tests/golden/request_refusals.json (tools/record_refusals.py): every recorded call to one of the ten
correlation and Doppler-search entries must return the recorded rc, leave the recorded rmx_last_error text and, where the
recorded call wrote nothing, write nothing.  The table was recorded with the library of the commit in front of the checked
request (host_request.hpp: check_request), so this pins "the one function refuses what the scattered checks refused, for
the same reason, in the same words".  Only the controls launch kernels."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_refusals  # noqa: E402

with open(record_refusals.TABLE) as _f:
    TABLE = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    with record_refusals.engine() as e:
        yield e


def test_table_is_the_tool_s_list():
    """the committed table holds exactly the calls the tool makes today, arguments included"""
    assert [(r["name"], r["entry"], r["args"]) for r in TABLE] == [(c["name"], c["entry"], c["args"]) for c in record_refusals.cases()]
    assert len(TABLE) <= 200
    entries = {r["entry"] for r in TABLE}
    assert entries == set(record_refusals.ENTRIES) and len(entries) == 10
    for e in entries:   # per entry a control that ran, refusals, and an empty batch that wrote nothing
        rows = [r for r in TABLE if r["entry"] == e]
        assert any(r["rc"] == 0 and not r["untouched"] for r in rows), e
        assert any(r["rc"] == -1 for r in rows) and any(r["rc"] == 0 and r["untouched"] for r in rows), e


@pytest.mark.parametrize("row", TABLE, ids=[r["name"] for r in TABLE])
def test_call(eng, row):
    got = record_refusals.run_case(eng, row)
    print(row["name"], got)
    assert got["rc"] == row["rc"]
    assert got["text"] == row["text"]
    assert got["untouched"] == row["untouched"]
