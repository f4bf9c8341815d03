"""The halo-exchange timers without a GPU: tse_comm_timing is part of the C ABI of both product libraries (72 and 64 levels), and the
HommeTime_stats rows of a multi-rank run put bndry_exchange and bndry_exchange_wait behind the reference's four, which keep their order."""
import os
import re

import numpy as np

from transport_se_amd import _lib
from transport_se_amd import prim_main as pm
from transport_se_amd.hip_mod import COMM_GROUPS, COMM_TOTALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_comm_timing_is_declared_and_exported_by_both_product_libraries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+tse_comm_timing\s*\(\s*tse_ctx\s*\*\s*ctx\s*,\s*int\s+enable\s*\)\s*;", text)
    assert "tse_comm_timing" in _lib.SYMBOLS
    for L in (_lib.lib(), _lib.lib(nlev=64)):
        assert hasattr(L, "tse_comm_timing")


def test_comm_group_names_leave_the_existing_groups_sums_alone():
    """tse_kernel_time matches by prefix: no existing group name is a prefix of a comm_* name or the other way round, and the totals
    are prefixes of exactly the groups they sum"""
    existing = ("advance0", "advance1", "advance2", "dss", "lap", "minmax", "remap", "level", "dcmip", "avg", "stateq")
    for old in existing + ("advance",):
        for new in COMM_GROUPS:
            assert not new.startswith(old) and not old.startswith(new), (old, new)
    assert [g for g in COMM_GROUPS if g.startswith("comm")] == list(COMM_GROUPS)
    assert [g for g in COMM_GROUPS if g.startswith("comm_exchange")] == ["comm_exchange_q", "comm_exchange_mm"]
    assert all(len([g for g in COMM_GROUPS if g.startswith(t)]) == 2 for t in COMM_TOTALS[1:])


def _rows(path):
    return [l.split() for l in open(path).read().splitlines()[1:]]


def test_hommetime_keeps_the_four_rows_and_appends_the_exchange_rows(tmp_path):
    one = np.array([[10.0, 1.0, 7.0, 2.0]])
    path = str(tmp_path / "one")
    pm.write_hommetime(path, pm.hommetime_timers(one, [2, 6, 6, 2]), 1)
    rows = _rows(path)
    assert [r[0] for r in rows] == list(pm.HOMMETIME_ROWS)

    two = np.array([[10.0, 1.0, 7.0, 2.0, 0.5, 0.2], [11.0, 1.5, 7.5, 2.5, 0.7, 0.1]])
    path = str(tmp_path / "two")
    pm.write_hommetime(path, pm.hommetime_timers(two, [2, 6, 6, 2, 24, 30]), 2)
    rows = _rows(path)
    assert [r[0] for r in rows] == list(pm.HOMMETIME_ROWS) + ["bndry_exchange", "bndry_exchange_wait"]
    assert rows[0][0] == "prim_run" and open(path).read().splitlines()[1].startswith("prim_run")
    # name, processes, threads, count (x ranks), walltotal, wallmax, wallmin
    assert rows[4][1:] == ["2", "1", "48", "1.200000", "0.700000", "0.500000"]
    assert rows[5][1:] == ["2", "1", "60", "0.300000", "0.200000", "0.100000"]
    assert rows[0][1:] == ["2", "1", "4", "21.000000", "11.000000", "10.000000"]
