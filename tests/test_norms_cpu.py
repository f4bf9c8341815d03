"""The DCMIP error norms from element partials, without a GPU: tests/norm_model.py (the device's order of addition in numpy) against an exact
referee at the textbook summation bound, diagnostics.norms_from_partials against diagnostics.dcmip_norms at the forward bound derived in
norm_model.forward_bounds, three planted errors that those bounds must catch, the edge cases, and the declarations of the new entry points.

Inputs: the real ne2 and ne3 meshes with smooth synthetic fields on the shipped 72-level grid.  ne2 has a GLL node on each pole
(cos(lat) = 6e-17: a column of almost no weight) and elements that own only 4 of their 16 points; ne3 has no polar node."""
import math
import os
import re

import numpy as np
import pytest

import norm_model as nm
from transport_se_amd import _lib
from transport_se_amd import cube_mesh as cm
from transport_se_amd import diagnostics as dg
from transport_se_amd.hybvcoord import HvCoord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def case(ne):
    """mesh, weights and two smooth positive fields (a blob that has moved and lost some of its peak), computed once per mesh"""
    if ne not in _cache:
        hv = HvCoord()
        g = cm.geometry(ne)
        lat, lon = g["lat"], g["lon"]
        zm = dg.level_heights(hv.hyam, hv.hybm)
        owner, colw, dh = dg.column_weights(ne, lat, lon, zm)
        z = (zm / zm.max())[None, :, None, None]

        def blob(lon0, amp):
            r2 = (lat[:, None] - 0.3) ** 2 + (np.cos(lat) * np.sin(0.5 * (lon - lon0)))[:, None] ** 2
            return 0.1 + amp * np.exp(-3.0 * r2) * np.exp(-8.0 * (z - 0.45) ** 2) + 0.05 * np.sin(lat)[:, None] * z
        q0 = blob(1.0, 0.9); qf = blob(1.4, 0.8)
        dlat = 0.5 * np.pi / (ne * 3)
        colw_all = (dg.R_EARTH * np.cos(lat) * dlat) * (dg.R_EARTH * dlat)
        _cache[ne] = dict(ne=ne, lat=lat, lon=lon, zm=zm, owner=owner, colw=colw, dh=dh, q0=q0, qf=qf, colw_all=colw_all, nlev=hv.nlev,
                          avg=nm.model_avg(q0, owner))
    return _cache[ne]


def norms_of(c, partials):
    return dg.norms_from_partials(partials, np.arange(partials.shape[0]), partials.shape[0])


@pytest.mark.parametrize("ne,ncol", [(2, 218), (3, 488)])
def test_meshes_have_the_edge_cases_the_tests_rely_on(ne, ncol):
    c = case(ne)
    assert int(c["owner"].sum()) == ncol == dg.unique_columns(c["lat"], c["lon"]).size
    per = c["owner"].reshape(-1, 16).sum(1)
    assert per.min() == 4 and per.max() == 16
    polar = np.abs(np.cos(c["lat"])) < 1e-12
    assert polar.any() == (ne == 2)
    if ne == 2:
        w = c["colw"][polar & (c["owner"] == 1)]
        assert w.size == 2 and (w > 0).all() and (w < 1e-3).all()    # cos(pi/2) = 6e-17 in fp64: a positive weight of almost nothing
    assert (c["colw"][c["owner"] == 1] > 0).all() and (c["colw"][c["owner"] == 0] == 0).all()
    assert np.array_equal(c["colw"][c["owner"] == 1], c["colw_all"][c["owner"] == 1])
    assert (c["dh"] > 0).all() and c["dh"].size == c["nlev"]


@pytest.mark.parametrize("ne", [2, 3])
def test_model_element_sums_lie_within_the_textbook_bound_of_the_exact_referee(ne):
    c = case(ne)
    got = nm.element_partials(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])
    S, n = nm.exact_element_sums(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])
    bound = nm.element_bound(S, n)
    err = np.abs(got[:, :4] - S)
    print("ne%d: worst element-sum error / bound = %.3f" % (ne, (err / bound).max()))
    assert (S > 0).all() and (err <= bound).all()
    # the order matters (so the bound is not vacuous: the model does round) and the extrema do not
    E, nlev = c["q0"].shape[:2]
    t = nm.terms(c["q0"], c["qf"], c["colw"], c["dh"], c["avg"])
    own = c["owner"].reshape(E, 16) != 0
    assert (got[:, :4] != S).any()
    for e in range(E):
        assert got[e, 4] == t[0, e][:, own[e]].max() and got[e, 5] == t[1, e][:, own[e]].max()
        x = c["qf"].reshape(E, nlev, 16)[e][:, own[e]]
        assert got[e, 6] == x.max() and got[e, 7] == x.min()
    s0 = nm.element_sum0(c["q0"], c["owner"]); x0 = nm.exact_sum0(c["q0"], c["owner"])
    assert (np.abs(s0 - x0) <= nm.element_bound(x0, n)).all()


@pytest.mark.parametrize("ne", [2, 3])
def test_norms_from_partials_meet_dcmip_norms_at_the_derived_forward_bound(ne):
    c = case(ne)
    host = dg.dcmip_norms(ne, c["lat"], c["lon"], c["q0"], c["qf"], c["zm"])
    new = norms_of(c, nm.element_partials(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"]))
    fb = nm.forward_bounds(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])
    # the ingredients of the bound, each judged by the exact sum: numpy's sums, and the two means
    g = nm.exact_globals(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])
    cols = dg.unique_columns(c["lat"], c["lon"])
    nlev = c["nlev"]
    qi = np.moveaxis(c["q0"], 1, 0).reshape(nlev, -1)[:, cols]
    qf = np.moveaxis(c["qf"], 1, 0).reshape(nlev, -1)[:, cols]
    dV = c["colw"].reshape(-1)[cols][None, :] * c["dh"][:, None]
    e_n = nm.gamma(nm.numpy_depth(nlev, qi.size))
    for arr in (np.abs(qf - qi) * dV, (qf - qi) * (qf - qi) * dV, qi):
        exact = math.fsum(arr.ravel().tolist())
        assert abs(float(arr.sum()) - exact) <= (e_n + nm.U) * exact
    assert abs(float(qi.mean()) - c["avg"]) <= fb["davg"]
    assert abs(g["S"][0] - math.fsum((np.abs(qf - qi) * dV).ravel().tolist())) == 0.0    # the same terms on both routes
    for k in ("L1", "L2", "Linf"):
        rel = abs(new[k] - host[k]) / host[k]
        print("ne%d %s: host %.17g, partials %.17g, relative difference %.3e, bound %.3e" % (ne, k, host[k], new[k], rel, fb[k]))
        assert 0 < fb[k] < 1e-12 and rel <= fb[k]
    assert new["q_max"] == host["q_max"] and new["q_min"] == host["q_min"]


def weighted_mean(c):
    own = c["owner"].reshape(-1, 1, 16) != 0
    E, nlev = c["q0"].shape[:2]
    dV = np.broadcast_to(c["colw"].reshape(E, 1, 16) * c["dh"].reshape(1, nlev, 1), (E, nlev, 16))
    m = np.broadcast_to(own, (E, nlev, 16))
    return math.fsum((c["q0"].reshape(E, nlev, 16) * dV)[m].tolist()) / math.fsum(dV[m].tolist())


@pytest.mark.parametrize("plant", ["owner", "dh", "mean"])
@pytest.mark.parametrize("ne", [2, 3])
def test_planted_errors_are_caught_at_the_bounds(ne, plant):
    """the owner mask ignored (shared nodes counted twice), dh in reversed level order, dev against the weighted mean: each must leave the
    element bound against the referee AND the forward bound against dcmip_norms"""
    c = case(ne)
    bad = nm.element_partials(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"], plant=plant, colw_all=c["colw_all"],
                              avg_weighted=weighted_mean(c))
    S, n = nm.exact_element_sums(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])
    assert (np.abs(bad[:, :4] - S) > nm.element_bound(S, n)).any()
    host = dg.dcmip_norms(ne, c["lat"], c["lon"], c["q0"], c["qf"], c["zm"])
    new = norms_of(c, bad)
    fb = nm.forward_bounds(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])
    out = [k for k in ("L1", "L2", "Linf") if abs(new[k] - host[k]) > fb[k] * host[k]]
    assert out, (plant, new, host)
    if plant == "mean":   # (dq does not see the mean: the error sits in the denominators alone)
        assert np.array_equal(bad[:, [0, 2, 4]], nm.element_partials(c["q0"], c["qf"], c["owner"], c["colw"], c["dh"], c["avg"])[:, [0, 2, 4]])


def test_an_element_without_an_owned_point_gives_the_neutral_values():
    c = case(2)
    owner = c["owner"].copy(); owner[5] = 0
    got = nm.element_partials(c["q0"], c["qf"], owner, c["colw"], c["dh"], c["avg"])
    assert np.array_equal(got[5], [0, 0, 0, 0, 0, 0, -np.inf, np.inf])
    assert nm.element_sum0(c["q0"], owner)[5] == 0.0
    # ... and they are neutral: the norms are those of the other elements
    rest = np.delete(np.arange(got.shape[0]), 5)
    a = dg.norms_from_partials(got, np.arange(got.shape[0]), got.shape[0])
    b = dg.norms_from_partials(got[rest], np.arange(rest.size), rest.size)
    assert a == b


def test_no_change_gives_zero_norms_exactly():
    c = case(3)
    got = nm.element_partials(c["q0"], c["q0"], c["owner"], c["colw"], c["dh"], c["avg"])
    assert not got[:, [0, 2, 4]].any()
    n = norms_of(c, got)
    assert n["L1"] == 0.0 and n["L2"] == 0.0 and n["Linf"] == 0.0
    assert n["q_max"] == c["q0"].max() and n["q_min"] == c["q0"].min()


def test_column_weights_are_dcmip_norms_own_numbers():
    """both routes multiply the same dV: dcmip_norms' result is what it is when its weights are rebuilt from column_weights"""
    c = case(2)
    cols = dg.unique_columns(c["lat"], c["lon"])
    assert np.array_equal(np.flatnonzero(c["owner"].reshape(-1)), cols)
    nlev = c["nlev"]
    qi = np.moveaxis(c["q0"], 1, 0).reshape(nlev, -1)[:, cols]; qf = np.moveaxis(c["qf"], 1, 0).reshape(nlev, -1)[:, cols]
    dV = c["colw"].reshape(-1)[cols][None, :] * c["dh"][:, None]
    host = dg.dcmip_norms(2, c["lat"], c["lon"], c["q0"], c["qf"], c["zm"])
    assert host["L1"] == float((np.abs(qf - qi) * dV).sum() / (np.abs(qi - qi.mean()) * dV).sum())
    assert host["Linf"] == float((np.abs(qf - qi) * dV).max() / (np.abs(qi - qi.mean()) * dV).max())


# ---- the declarations (no GPU): header, loader, Fortran seam ----
SIGNATURES = {
    "tse_norm_setup": "int tse_norm_setup(tse_ctx *ctx, const int *owner, const double *colw, const double *dh)",
    "tse_norm_reference": "int tse_norm_reference(tse_ctx *ctx, int nt, int q, double *sum0)",
    "tse_norm_partials": "int tse_norm_partials(tse_ctx *ctx, int nt, int q, double avg, double *out)",
}


def test_header_loader_and_library_declare_the_norm_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()).rstrip(";").strip() for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    for name, sig in SIGNATURES.items():
        assert decl.get(name) == sig, decl.get(name)
        assert name in _lib.SYMBOLS
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):     # the 72-, 64- and 80-level libraries
        L = _lib.lib(nlev=nlev)
        assert all(hasattr(L, n) for n in SIGNATURES), nlev
    import ctypes as C
    H = C.CDLL(_lib.HOOKS_SO)                          # ... and the hooks twin
    assert all(hasattr(H, n) for n in SIGNATURES)


def test_fortran_seam_has_the_norm_wrappers():
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    for c_name in SIGNATURES:
        assert "name='%s'" % c_name in src, c_name
    for name, args in (("norm_setup_hip", "owner, colw, dh"), ("norm_reference_hip", "nt, q, sum0"), ("norm_partials_hip", "nt, q, avg, out")):
        assert re.search(r"subroutine\s+%s\s*\(\s*%s\s*\)" % (name, re.escape(args)), src), name
        assert re.search(r"public\s*::[^\n]*\b%s\b" % name, src), name
        body = src[src.index("subroutine %s" % name):src.index("end subroutine %s" % name)]
        assert "call check(" in body      # the module's error route (check -> seam_abort)
