"""Replay of tests/golden/route_table.json and tests/golden/caf_route_table.json (tools/record_routes.py): every case must
launch the kernel families the recorded library launched, as often, and produce the same bytes in every output array (or
refuse with the same text).  Each table was recorded with the library of the commit in front of its planner (host_plan.hpp:
plan_route for the correlation, plan_caf for the Doppler search), so this pins "the planner chooses what the scattered rules
chose".  A case recorded as not reproducible (digest null) carries its arrays and is compared with the bars of
test_gpu_parity: integer outputs exact, 1e-5 on the lag (and on dop_frac), rtol 1e-5 on the rest."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_routes  # noqa: E402

TABLES = []
for _path in (record_routes.TABLE, record_routes.CAF_TABLE):
    with open(_path) as _f:
        TABLES.append(json.load(_f)["cases"])
TABLE = TABLES[0] + TABLES[1]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"


def test_table_is_mostly_reproducible():
    for table in TABLES:   # each on its own
        nulls = [r["name"] for r in table if "error" not in r and r["digest"] is None]
        assert 10 * len(nulls) <= len(table), nulls


@pytest.mark.parametrize("row", TABLE, ids=[r["name"] for r in TABLE])
def test_route(built, row):
    got = record_routes.run_case(row)
    if "error" in row:
        assert got.get("error") == row["error"]
        return
    assert "error" not in got, got
    print(row["name"], got["launches"])
    assert got["launches"] == row["launches"]
    if row["digest"] is not None:
        assert record_routes.digest(got["arrays"]) == row["digest"]
        return
    ref = [np.asarray(a, dtype=g.dtype).reshape(g.shape) for a, g in zip(row["arrays"], got["arrays"])]
    caf = row["kind"] == "caf"
    if caf:
        assert np.array_equal(got["arrays"][0], ref[0])
    first = (2 if row.get("fine") else 1) if caf else 0   # behind dop_idx (and dop_frac)
    if first == 2:
        assert np.all(np.abs(got["arrays"][1] - ref[1]) <= 1e-5)
    li, lf, pk = got["arrays"][first:][:3]
    ri, rf, rp = ref[first:][:3]
    assert np.array_equal(li, ri)
    lag, rlag = li + lf.astype(np.float64), ri + rf.astype(np.float64)
    assert np.all(np.abs(lag - rlag) <= 1e-5 * np.maximum(np.abs(rlag), 1.0))
    assert np.allclose(pk, rp, rtol=1e-5, atol=0)
    if row["quality"]:
        assert np.allclose(got["arrays"][first + 3], ref[first + 3], rtol=1e-5, atol=0)
