"""tse_biharmonic_view without a GPU: the two entries in the header, the symbol list, the product libraries and the Fortran seam;
tse_biharmonic_view_plan (csrc/tse_views.cpp: paths and footprints of every layout of tests/dss_view_model.py for `in` and for `out`, the
in-place and the disjoint form, every refusal that needs no device); and the model the GPU bound rests on (biharmonic_model.longdouble):
the oracle's fp64 composition lies under its bound, four planted errors do not."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import biharmonic_model as bm
import dss_view_model as dm
import elem_ops_ld as ld
import pyoracle as po
from transport_se_amd import _lib
from transport_se_amd.hip_mod import TseError, biharmonic_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tse_biharmonic_view", "tse_biharmonic_view_plan")
E = 24
BASE = 1 << 20   # a made-up address: the plan never touches memory


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_biharmonic_view"] == ("int tse_biharmonic_view(tse_ctx *ctx, int nf, int nk, int order, const tse_view *in, const tse_view *out, "
                                           "void *stream);")
    assert decl["tse_biharmonic_view_plan"] == ("int tse_biharmonic_view_plan(int nelemd, int nf, int nk, const tse_view *in, const tse_view *out, "
                                                "int path[2], long long lo[2], long long hi[2]);")
    assert re.search(r"#define\s+TSE_LAPLACE\s+1\b", text) and re.search(r"#define\s+TSE_BIHARMONIC\s+2\b", text)
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert not [n for n in NAMES if not hasattr(L, n)], nlev
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert re.search(r"subroutine\s+biharmonic_view_hip\s*\(", src) and re.search(r"public\s*::[^\n]*\bbiharmonic_view_hip\b", src)
    assert re.search(r"lap_order1\s*=\s*1\s*,\s*lap_order2\s*=\s*2", src) and "name='tse_biharmonic_view'" in src


# ---- tse_biharmonic_view_plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_plan_paths_and_footprints_of_in_and_out(nlev):
    seen = set()
    for nf in (1, 2, 5):
        for nk in (1, nlev, nlev + 1):
            lay = {name: dm.layout(name, E, nf, nk) for name in dm.LAYOUTS}
            for i, name in enumerate(dm.LAYOUTS):
                other = dm.LAYOUTS[(i + 3) % len(dm.LAYOUTS)]
                # in place (strides alone), then `out` another layout in an allocation of its own right behind in's
                got = biharmonic_view_plan(E, nf, nk, lay[name][0], nlev=nlev)
                assert got[0] == got[1] and got[0]["path"] == dm.expected_path(name, nk, nlev), (name, nf, nk, got)
                assert (got[0]["lo"], got[0]["hi"]) == dm.footprint(name, E, nf, nk), (name, nf, nk, got)
                got = biharmonic_view_plan(E, nf, nk, (lay[name][0], BASE), (lay[other][0], BASE + 8 * lay[name][2]), nlev=nlev)
                for g, nm in zip(got, (name, other)):
                    assert g["path"] == dm.expected_path(nm, nk, nlev), (name, other, nf, nk, got)
                    assert (g["lo"], g["hi"]) == dm.footprint(nm, E, nf, nk) and g["hi"] <= lay[nm][2], (name, other, nf, nk, got)
                seen.add((got[0]["path"], got[1]["path"]))
    assert {a for a, _ in seen} == {b for _, b in seen} == {0, 1, 2} and any(a != b for a, b in seen)


def test_plan_in_place_disjoint_and_refusals():
    nlev, nf = 72, 2
    plane = nlev * 16
    dense = [nf * plane, plane, 16, 4, 1]
    size = E * nf * plane                                               # doubles of the dense field
    lev = [nf * 16 * nlev, 16 * nlev, 1, 4 * nlev, nlev]
    # identical views: in place
    assert biharmonic_view_plan(E, nf, nlev, (dense, BASE), (dense, BASE)) == [dict(path=0, lo=0, hi=size)] * 2
    # disjoint: touching footprints on either side, other strides
    for off in (size, -size):
        assert [g["path"] for g in biharmonic_view_plan(E, nf, nlev, (dense, BASE), (lev, BASE + 8 * off))] == [0, 1]
    # out overlapping in without being it: a shifted pointer (by one double, by all but one), other strides inside one footprint
    for off in (1, -1, size - 1, -(size - 1), 16):
        with pytest.raises(TseError, match="overlaps in"):
            biharmonic_view_plan(E, nf, nlev, (dense, BASE), (dense, BASE + 8 * off))
    with pytest.raises(TseError, match="overlaps in"):
        biharmonic_view_plan(E, nf, nlev, (dense, BASE), (lev, BASE))
    with pytest.raises(TseError, match="overlaps in"):                  # the same addresses, the fields' order reversed
        biharmonic_view_plan(E, nf, nlev, (dense, BASE), ([nf * plane, -plane, 16, 4, 1], BASE + 8 * plane))
    # the refusals of either view, the view named
    for which in ("in", "out"):
        def plan(n_f, n_k, bad):
            a, b = ((bad, BASE), (dense, BASE + 8 * size)) if which == "in" else ((dense, BASE), (bad, BASE + 8 * size))
            return biharmonic_view_plan(E, n_f, n_k, a, b)
        for axis, word in enumerate(("element", "q", "level", "j", "i")):   # a zero stride on an extent above 1, the axis named
            z = list(dense); z[axis] = 0
            with pytest.raises(TseError, match=r"stride 0 on the %s axis.*\(%s\)" % (word, which)):
                plan(nf, nlev, z)
        with pytest.raises(TseError, match=r"overlap itself.*q stride.*\(%s\)" % which):     # fields half a field apart
            plan(nf, nlev, [nf * plane, plane // 2, 16, 4, 1])
        with pytest.raises(TseError, match=r"overlap itself.*\(%s\)" % which):               # levels interleaved with the points of a row
            plan(nf, nlev, [nf * plane, plane, 2, 4, 1])
    with pytest.raises(TseError, match="tse_biharmonic_view: nf = 0"):
        biharmonic_view_plan(E, 0, nlev, dense)
    with pytest.raises(TseError, match="tse_biharmonic_view: nk = 0"):
        biharmonic_view_plan(E, nf, 0, dense)
    with pytest.raises(TseError, match="tse_biharmonic_view: nk = %d" % (nlev + 2)):
        biharmonic_view_plan(E, nf, nlev + 2, dense)
    with pytest.raises(TseError, match="null view"):
        biharmonic_view_plan(E, nf, nlev, None)
    L = _lib.lib()
    v = _lib.View(BASE, (C.c_longlong * 5)(*dense))
    assert L.tse_biharmonic_view_plan(E, nf, nlev, C.byref(v), None, None, None, None) != 0 and b"null view" in L.tse_last_error()
    # an axis of extent 1 may carry stride 0: a surface field [e][j][i], interfaces
    assert biharmonic_view_plan(E, 1, 1, [16, 0, 0, 4, 1]) == [dict(path=0, lo=0, hi=E * 16)] * 2
    assert biharmonic_view_plan(E, 1, nlev + 1, [(nlev + 1) * 16, 0, 16, 4, 1])[0]["path"] == 0
    assert L.tse_biharmonic_view(None, 1, 1, 2, None, None, None) != 0 and b"null context" in L.tse_last_error()   # (refused before any device call)


# ---- the model -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh(ne):
    return po.Oracle(ne, 1)


NF, NK = 1, 3


def _fields(o):
    return (("random", bm.random_field(o.nelem, NF, NK)), ("smooth", bm.smooth_field(o, NF, NK)), ("dss_view", 300.0 * dm.field(o.nelem, NF, NK)))


@pytest.mark.parametrize("ne", [2, 3, 5])
def test_oracle_composition_within_the_longdouble_bound(ne):
    """bound(19, A) for order 1, bound(42, A) for order 2.  Measured here (worst error / bound over ne2, ne3, ne5 and the three fields):
    order 1 0.128, order 2 0.030."""
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    o = _mesh(ne)
    for order in bm.ORDERS:
        for name, f in _fields(o):
            ref, A = bm.longdouble(o, f, order)
            worst = float(bm.ratio(bm.oracle_fp64(o, f, order), ref, A, order).max())
            print("biharmonic model ne%d order %d %s: worst error / bound = %.3f" % (o.ne, order, name, worst))
            assert worst < 1.0, (order, name, worst)


@pytest.mark.parametrize("ne", [2, 3])
def test_planted_errors_exceed_the_bound(ne):
    """each planted error is beyond bound(42, A) in every element it touches: the one element whose node sum lacks a contribution, or all"""
    o = _mesh(ne)
    for name, f in _fields(o)[:2]:
        ref, A = bm.longdouble(o, f, 2)
        for plant in bm.PLANTS:
            got = bm.longdouble(o, f, 2, plant)[0].astype(np.float64)
            per_elem = bm.ratio(got, ref, A, 2).reshape(o.nelem, -1).max(axis=1)
            touched = [bm.dropped_copy(o)[0]] if plant == "dropped" else list(range(o.nelem))
            print("biharmonic planted %s ne%d %s: least error / bound over the touched elements = %.3g" % (plant, o.ne, name, per_elem[touched].min()))
            assert (per_elem[touched] > 1.0).all(), (plant, name, per_elem[touched].min())
            if plant == "dropped":
                rest = np.delete(per_elem, touched)
                assert (rest < 1.0).all()
