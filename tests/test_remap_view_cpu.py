"""tse_remap_view without a GPU: the three entries in the header, the symbol list and the three product libraries; tse_remap_view_plan
(csrc/tse_views.cpp: path and footprint of the field and the two grids, the refusals that need no device); and the column check that
check_remap_grids now shares with the device (csrc/tse_remap_check.h), held to what check_remap_grids reported before it was shared."""
import os
import re

import numpy as np
import pytest

import remap_ld
from host_tables import check_remap_grids
from transport_se_amd import _lib
from transport_se_amd.hip_mod import TseError, remap_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tse_remap_view", "tse_remap_view_status", "tse_remap_view_plan")
NE = remap_ld.NELEM


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_remap_view"] == ("int tse_remap_view(tse_ctx *ctx, int nf, int mode, int alg, const tse_view *field, const tse_view *dp_src, "
                                      "const tse_view *dp_tgt, void *stream);")
    assert decl["tse_remap_view_status"] == "int tse_remap_view_status(tse_ctx *ctx, int *nrefused, int where[4] );"
    assert decl["tse_remap_view_plan"] == ("int tse_remap_view_plan(int nelemd, int nf, const tse_view *field, const tse_view *dp_src, const tse_view *dp_tgt, "
                                           "int path[3], long long lo[3], long long hi[3]);")
    assert re.search(r"#define\s+TSE_REMAP_MASS\s+0\b", text) and re.search(r"#define\s+TSE_REMAP_MEAN\s+1\b", text)
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert not [n for n in NAMES if not hasattr(L, n)], nlev
    assert any(p.endswith("tse_remap_check.h") for p in _lib.SRC)
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    for name in ("remap_view_hip", "remap_view_status_hip"):
        assert re.search(r"subroutine\s+%s\s*\(" % name, src) and re.search(r"public\s*::[^\n]*\b%s\b" % name, src), name
    assert "name='tse_remap_view'" in src and "name='tse_remap_view_status'" in src


# ---- tse_remap_view_plan -----------------------------------------------------------------------------------------------------
def _dense(nf, nlev):
    """point-fastest [e][q][k][j][i] and [e][k][j][i]"""
    return [nf * nlev * 16, nlev * 16, 16, 4, 1], [nlev * 16, 0, 16, 4, 1]


def _levels(nf, nlev, pad):
    """level-fastest [e][q][j][i][k + pad]"""
    S = nlev + pad
    return [nf * 16 * S, 16 * S, 1, 4 * S, S], [16 * S, 0, 1, 4 * S, S]


def _permuted(nf, nlev):
    """[q][e][k][i][j]: q outermost, i and j swapped -> the generic path"""
    return [nlev * 16, NE * nlev * 16, 16, 1, 4], [nlev * 16, 0, 16, 1, 4]


@pytest.mark.parametrize("nlev", [72, 64, 80])
@pytest.mark.parametrize("nf", [1, 3, 35])
def test_plan_paths_and_footprints(nf, nlev):
    n = NE * nf * nlev * 16
    for make, path, span_f, span_g in ((_dense, 0, n, NE * nlev * 16), (lambda a, b: _levels(a, b, 0), 1, n, NE * nlev * 16),
                                       (lambda a, b: _levels(a, b, 3), 1, NE * nf * 16 * (nlev + 3) - 3, NE * 16 * (nlev + 3) - 3),
                                       (_permuted, 2, n, NE * nlev * 16)):
        f, g = make(nf, nlev)
        got = remap_view_plan(NE, nf, f, g, g, nlev=nlev)
        assert [p["path"] for p in got] == [path] * 3, (make, got)
        assert (got[0]["lo"], got[0]["hi"]) == (0, span_f), got
        assert (got[1]["lo"], got[1]["hi"]) == (0, span_g) and got[1] == got[2], got
    # the path is chosen per view; a negative level stride (still whole 128-byte lines: point-fastest) moves the footprint below the pointer
    f, g = _dense(nf, nlev)
    fl, gl = _levels(nf, nlev, 3)
    neg = list(g); neg[2] = -16
    got = remap_view_plan(NE, nf, fl, g, neg, nlev=nlev)
    assert [p["path"] for p in got] == [1, 0, 0] and (got[2]["lo"], got[2]["hi"]) == (-(nlev - 1) * 16, (NE - 1) * nlev * 16 + 16), got
    got = remap_view_plan(NE, nf, f, gl, g, nlev=nlev)
    assert [p["path"] for p in got] == [0, 1, 0]


def test_plan_refusals_and_broadcast():
    nlev, nf = 72, 3
    f, g = _dense(nf, nlev)
    with pytest.raises(TseError, match="nf = 0"):
        remap_view_plan(NE, 0, f, g, g)
    for axis in range(5):   # a zero stride in the field, on any axis
        z = list(f); z[axis] = 0
        with pytest.raises(TseError, match="field.*stride 0"):
            remap_view_plan(NE, nf, z, g, g)
    with pytest.raises(TseError, match="field.*overlap itself"):   # the field overlapping itself: tracers half a tracer apart
        remap_view_plan(NE, nf, [nf * nlev * 16, nlev * 8, 16, 4, 1], g, g)
    with pytest.raises(TseError, match="dp_src.*no q axis"):
        remap_view_plan(NE, nf, f, [nlev * 16, 1, 16, 4, 1], g)
    # a broadcast target grid: one column of thicknesses for every point of every element
    got = remap_view_plan(NE, nf, f, g, [0, 0, 1, 0, 0])
    assert (got[2]["lo"], got[2]["hi"]) == (0, nlev)
    # the three pointers as byte offsets into one allocation: field, then dp_src, then dp_tgt
    nfield, ngrid = NE * nf * nlev * 16, NE * nlev * 16
    got = remap_view_plan(NE, nf, (f, 0), (g, nfield * 8), (g, (nfield + ngrid) * 8))
    assert [p["path"] for p in got] == [0, 0, 0]
    with pytest.raises(TseError, match="overlaps dp_src"):   # dp_src starts on the field's last double
        remap_view_plan(NE, nf, (f, 0), (g, (nfield - 1) * 8), (g, (nfield + ngrid) * 8))
    with pytest.raises(TseError, match="overlaps dp_tgt"):   # dp_tgt ends on the field's first double
        remap_view_plan(NE, nf, (f, ngrid * 8 - 8), (g, (nfield + ngrid) * 8), (g, 0))
    assert remap_view_plan(NE, nf, (f, ngrid * 8), (g, 0), (g, 0))   # the two grids may be one array
    with pytest.raises(TseError, match="overlaps dp_src"):   # (one null pointer is an offset of 0, not "unknown")
        remap_view_plan(NE, nf, (f, 0), (g, 8), (g, nfield * 8))


# ---- the shared column check -------------------------------------------------------------------------------------------------
def planted(dp1, dp2, nlev):
    """{name: (dp1, dp2)} with one offence each -- NaN and -1.0 in dp1, -1e-3 in dp2, a dp2 column scaled by 3, a dp1 column that sums to
    2^53 -- and all five together"""
    def nan_dp1(a, b): a[3, 10, 1, 2] = np.nan
    def neg_dp1(a, b): a[5, 0, 0, 0] = -1.0
    def neg_dp2(a, b): b[7, 20, 3, 3] = -1e-3
    def dp2_x3(a, b): b[11, :, 2, 1] *= 3.0
    def sum_2p53(a, b): a[13, :, 0, 1] = 1.0; a[13, 0, 0, 1] = 2.0 ** 53 - (nlev - 1)
    each = (nan_dp1, neg_dp1, neg_dp2, dp2_x3, sum_2p53)
    out = {}
    for fn in each:
        a, b = dp1.copy(), dp2.copy(); fn(a, b); out[fn.__name__] = (a, b)
    a, b = dp1.copy(), dp2.copy()
    for fn in each:
        fn(a, b)
    out["all"] = (a, b)
    return out


# (element, column, level) and message of check_remap_grids on planted(remap_ld.grids(nlev)), recorded from the library as it was BEFORE the
# column test moved into csrc/tse_remap_check.h (every message of that library ends on "sum(dp1) + 1 = ...", "nan" where there is no limit)
_NAN = "dp1 is not a finite positive number: dp1 = nan at element 3, column 6, level 10 (counted from 0); sum(dp1) + 1 = nan"
_TAIL = "the search of the last level cannot end: sum(dp1) = 9007199254740992 at element 13, column 1, level %d (counted from 0); sum(dp1) + 1 = 9007199254740992"
RECORDED = {
    (72, "nan_dp1"): ((3, 6, 10), _NAN),
    (72, "neg_dp1"): ((5, 0, 0), "dp1 is not a finite positive number: dp1 = -1 at element 5, column 0, level 0 (counted from 0); sum(dp1) + 1 = nan"),
    (72, "neg_dp2"): ((7, 15, 20), "dp2 is negative or not finite: dp2 = -0.001 at element 7, column 15, level 20 (counted from 0); sum(dp1) + 1 = nan"),
    (72, "dp2_x3"): ((11, 9, 40), "the target grid leaves the source column: partial sum of dp2 = 101907.82717205044 at element 11, column 9, level 40 "
                                  "(counted from 0); sum(dp1) + 1 = 99238.974826670048"),
    (72, "sum_2p53"): ((13, 1, 71), "sum(dp1) is so large that sum(dp1) + 1 == sum(dp1), " + _TAIL % 71),
    (72, "all"): ((3, 6, 10), _NAN),
    (64, "nan_dp1"): ((3, 6, 10), _NAN),
    (64, "neg_dp1"): ((5, 0, 0), "dp1 is not a finite positive number: dp1 = -1 at element 5, column 0, level 0 (counted from 0); sum(dp1) + 1 = nan"),
    (64, "neg_dp2"): ((7, 15, 20), "dp2 is negative or not finite: dp2 = -0.001 at element 7, column 15, level 20 (counted from 0); sum(dp1) + 1 = nan"),
    (64, "dp2_x3"): ((11, 9, 31), "the target grid leaves the source column: partial sum of dp2 = 74887.498387779386 at element 11, column 9, level 31 "
                                  "(counted from 0); sum(dp1) + 1 = 74190.592365675198"),
    (64, "sum_2p53"): ((13, 1, 63), "sum(dp1) is so large that sum(dp1) + 1 == sum(dp1), " + _TAIL % 63),
    (64, "all"): ((3, 6, 10), _NAN),
}


@pytest.mark.parametrize("nlev", [72, 64])
def test_shared_column_check_reports_what_check_remap_grids_reported(nlev):
    dp1, dp2 = remap_ld.grids(nlev)
    assert check_remap_grids(dp1, dp2) is None
    for name, (a, b) in planted(dp1, dp2, nlev).items():
        assert check_remap_grids(a, b) == RECORDED[(nlev, name)], name
