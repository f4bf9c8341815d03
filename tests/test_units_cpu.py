"""The library's two products in translation units and code objects of their own, without a GPU: the tracer path (csrc/tse_api.hip,
tse_stage3.hip) and the operators on a resident host's arrays (csrc/tse_views_api.hip, tse_column.hip).  Read from the built default
library with tools/kernel_digest.py: every kernel sits in exactly one code object and no view kernel in the path's; from the sources:
tse_api.hip does not see the view headers; and through the C ABI: the entries of both units write the one message of tse_last_error."""
import ctypes as C
import importlib.util
import os
import re

import pytest

from transport_se_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transport_se_amd", "csrc")
# the symbols of the view families (csrc/tse_view_kernels.h)
VIEW_FAMILIES = ("k_view_", "k_forcing", "k_remap_view", "k_dss_view", "k_lap_view", "k_vlap_view", "k_vec_fold", "k_sphere_op", "k_stats_view", "k_column_view")
HIP_UNITS = [name for name, _ in _lib.UNITS if name.endswith(".hip")]   # the code objects of the library, in link order


@pytest.fixture(scope="module")
def units():
    """[{symbol: (code hash, resource record)}] per code object of the default library"""
    pytest.importorskip("msgpack")   # tools/kernel_digest.py reads the code objects' metadata notes with it
    spec = importlib.util.spec_from_file_location("kernel_digest", os.path.join(ROOT, "tools", "kernel_digest.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    return [kd.kernels(elf) for elf in kd.code_objects(open(_lib.SO, "rb").read())]


def test_every_kernel_sits_in_exactly_one_unit(units):
    assert HIP_UNITS == ["tse_api.hip", "tse_stage3.hip", "tse_column.hip", "tse_views_api.hip"]
    assert len(units) == len(HIP_UNITS) and all(units), [len(u) for u in units]
    seen = {}
    for i, table in enumerate(units):
        for sym in table:
            assert sym not in seen, "%s is in %s and %s" % (sym, HIP_UNITS[seen[sym]], HIP_UNITS[i])
            seen[sym] = i


def test_the_path_units_hold_no_view_kernel(units):
    is_view = lambda sym: any(f in sym for f in VIEW_FAMILIES)   # noqa: E731
    for i in (0, 1):
        assert not [s for s in units[i] if is_view(s)], HIP_UNITS[i]
    for i in (2, 3):   # ... and the view units nothing else
        assert not [s for s in units[i] if not is_view(s)], HIP_UNITS[i]
    assert all("k_column_view" in s for s in units[2])
    assert {f for f in VIEW_FAMILIES for s in units[3] if f in s} == set(VIEW_FAMILIES) - {"k_column_view"}


def test_the_path_unit_does_not_include_the_view_headers():
    includes = lambda name: re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M)   # noqa: E731
    seen, todo = set(), ["tse_api.hip", "tse_stage3.hip"]
    while todo:   # ... nor does a header they include
        name = todo.pop()
        if name in seen or not os.path.exists(os.path.join(CSRC, name)):
            continue
        seen.add(name)
        todo += [os.path.basename(i) for i in includes(name)]
    assert "tse_kernels.h" in seen and "tse_ctx.h" in seen
    assert not seen & {"tse_view_kernels.h", "tse_view_launch.h"}, sorted(seen)
    assert "tse_view_launch.h" in includes("tse_views_api.hip") and "tse_view_launch.h" in includes("tse_column.hip")


def test_both_units_write_one_error_message():
    L = _lib.lib()
    v = _lib.View(None, (C.c_longlong * 5)(1152, 0, 16, 4, 1))
    assert L.tse_dss_view(None, 1, 72, 0, C.byref(v), None) == 1          # tse_views_api.hip
    assert L.tse_last_error() == b"tse_dss_view: null context"
    assert L.tse_view_plan(b"temperature", 3, 3, C.byref(v), 0, None, None, None) != 0   # tse_views.cpp, through tse_api.hip's channel
    assert b"unknown field" in L.tse_last_error() and b"tse_dss_view" not in L.tse_last_error()
    args = _lib.InitArgs()
    assert L.tse_init(None, C.byref(args)) == 1                           # tse_api.hip
    assert L.tse_last_error() == b"tse_init: null argument"
