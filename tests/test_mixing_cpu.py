"""The mixing and filament diagnostics (Lauritzen and Thuburn 2012) without a GPU: the distance of tests/mixing_model.py (the device's
algorithm in numpy) against its longdouble referee, diagnostics.mixing_from_partials of the model's element shares against
diagnostics.mixing_diagnostics at the textbook summation bound on the real ne2 and ne3 meshes, the DCMIP 1-1 initial state, three planted
errors that must be caught, empty elements, the --mixing argument's refusals and the declarations of the new entry point.

The bound on d.  D_MEASURED is the largest |d(model) - d(referee)| found over the families below for three parameter sets (DCMIP 1-1's
range [0, 1]; a range that ends below the curve's top, as a coarse mesh gives; a range with xmin < 0, the only way to three sign changes):
4.32e-16, at an on-the-curve point, where the bisection's last ulp of x is all there is to d.  The tests assert 4 x that figure, the margin
standing for what the referee's finite scan might not have met."""
import math
import os
import re

import numpy as np
import pytest

import mixing_model as mm
import norm_model as nm
from transport_se_amd import _lib
from transport_se_amd import cube_mesh as cm
from transport_se_amd import diagnostics as dg
from transport_se_amd import prim_main as pm
from transport_se_amd.hybvcoord import HvCoord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_MEASURED = 4.4e-16
D_BOUND = 4 * D_MEASURED
TAU = np.array(dg.MIX_TAU)
PARS = {"dcmip": (0.0, 1.0, 0.9, -0.8), "coarse": (0.0, 0.9717, 0.9, -0.8), "negative xmin": (-0.6, 1.0, 0.9, -0.8)}
_cache = {}


def mesh(ne):
    if ne not in _cache:
        hv = HvCoord()
        g = cm.geometry(ne)
        zm = dg.level_heights(hv.hyam, hv.hybm)
        owner, colw, dh = dg.column_weights(ne, g["lat"], g["lon"], zm)
        par = PARS["dcmip" if ne == 2 else "negative xmin"]
        chi, xi = mm.synthetic_fields(mm.constants(*par), TAU, 6 * ne * ne, hv.nlev, np.random.default_rng(40 + ne))
        _cache[ne] = dict(ne=ne, lat=g["lat"], lon=g["lon"], zm=zm, owner=owner, colw=colw, dh=dh, nlev=hv.nlev, par=par, chi=chi, xi=xi)
    return _cache[ne]


def from_partials(P, P0=None, ntau=TAU.size):
    return dg.mixing_from_partials(P, P if P0 is None else P0, np.arange(P.shape[0]), P.shape[0], ntau=ntau)


def close(a, b, bound):
    return abs(a - b) <= bound * abs(b)


def test_the_default_thresholds_are_the_papers():
    assert len(dg.MIX_TAU) == 19 and dg.MIX_TAU[0] == 0.10 and dg.MIX_TAU[1] == 0.15 and dg.MIX_TAU[-1] == 1.00
    assert len(dg.MIX_TAU) <= dg.MIX_NTAU == mm.NTAU and dg.MIX_NB == mm.NB


@pytest.mark.parametrize("name", list(PARS))
def test_model_distance_against_the_longdouble_referee(name):
    m = mm.constants(*PARS[name])
    fam = mm.families(m, TAU, np.random.default_rng(7))
    needed = ["on the curve", "near the curve", "inside the hull", "on the chord", "on the rectangle's edges", "on the rectangle's corners", "outside, left",
              "outside, right", "outside, below", "outside, above", "P >= 0", "P < 0, one sign change(s)", "P < 0, two sign change(s)",
              "chi equal to a threshold"]
    if name == "negative xmin":
        needed.append("P < 0, three sign change(s)")
    worst = 0.0
    for k in needed:
        x, y = fam[k]
        assert x.size > 0, k
        d = mm.distance(m, x, y)
        ref = mm.referee_distance(m, x, y)
        err = d.astype(np.longdouble) - ref
        print("%-14s %-30s n = %4d  max |d - referee| = %.3e  min (d - referee) = %.3e" % (name, k, x.size, float(np.abs(err).max()), float(err.min())))
        assert (np.abs(err) <= D_BOUND).all(), k
        assert (d >= ref - D_BOUND).all(), k          # (every candidate lies in [xmin, xmax]: never below the true minimum)
        worst = max(worst, float(np.abs(err).max()))
        # the product's host expression is the same algorithm: the same bits
        assert np.array_equal(d, dg.mixing_distance(dg.mixing_constants(*PARS[name]), x, y)), k
    print("%s: worst %.3e (D_MEASURED %.1e, asserted %.2e)" % (name, worst, D_MEASURED, D_BOUND))
    assert worst <= D_MEASURED
    # the families are what they say
    assert (mm.distance(m, *fam["on the curve"]) <= D_BOUND).all()
    A, B, C = mm.classes(m, *fam["inside the hull"])
    assert A.all()
    for side in ("left", "right", "below", "above"):
        assert mm.classes(m, *fam["outside, " + side])[2].all(), side
    assert (mm.cubic(m, *fam["P >= 0"])[0] >= 0).all()
    assert (mm.sign_changes(m, *fam["P < 0, one sign change(s)"]) == 1).all()
    if name == "negative xmin":
        assert (mm.sign_changes(m, *fam["P < 0, three sign change(s)"]) == 3).all()


def test_constants_are_the_same_bits_on_both_sides():
    for par in PARS.values():
        a, b = mm.constants(*par), dg.mixing_constants(*par)
        assert all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in a)
    with pytest.raises(ValueError):
        dg.mixing_constants(1.0, 1.0, 0.9, -0.8)
    with pytest.raises(ValueError):
        dg.mixing_constants(0.0, 1.0, 0.9, 0.0)


@pytest.mark.parametrize("ne", [2, 3])
def test_mixing_from_partials_meets_mixing_diagnostics_at_the_summation_bound(ne):
    c = mesh(ne)
    P = mm.element_partials(c["chi"], c["xi"], c["owner"], c["colw"], c["dh"], *c["par"], TAU)
    chi0 = np.roll(c["chi"], 1, axis=0)              # another field as "t0", so that l_f is not trivially 100
    P0 = mm.element_partials(chi0, c["xi"], c["owner"], c["colw"], c["dh"], *c["par"], TAU)
    new = from_partials(P, P0)
    host = dg.mixing_diagnostics(ne, c["lat"], c["lon"], c["chi"], c["xi"], c["zm"], *c["par"], TAU, chi0=chi0)
    sb = mm.summation_bounds(c["owner"], c["nlev"])
    assert 0 < sb["l"] < sb["l_f"] < 1e-12
    for k in ("l_r", "l_u", "l_o"):
        print("ne%d %s: host %.17g, partials %.17g, bound %.3e" % (ne, k, host[k], new[k], sb["l"]))
        assert host[k] > 0 and close(new[k], host[k], sb["l"]), k
    assert len(new["l_f"]) == len(host["l_f"]) == TAU.size
    for a, b in zip(new["l_f"], host["l_f"]):
        assert b > 0 and close(a, b, sb["l_f"])
    assert new["counts"] == host["counts"] and sum(new["counts"]) == c["nlev"] * int(c["owner"].sum()) and min(new["counts"]) > 0
    assert new["d_max"] == host["d_max"] > 0.5
    # entry 3 is the volume, whatever the fields are, and the element sums meet the exact referee at the textbook bound
    E = P.shape[0]
    own = c["owner"].reshape(E, 16) != 0
    dV = c["colw"].reshape(E, 1, 16) * c["dh"].reshape(1, -1, 1)
    exact = np.array([math.fsum(dV[e][:, own[e]].ravel().tolist()) for e in range(E)])
    assert (np.abs(P[:, 3] - exact) <= nm.element_bound(exact, own.sum(1) * c["nlev"])).all()
    assert not P[:, 8 + TAU.size:].any()


def test_dcmip11_initial_state_has_no_mixing_and_whole_filaments():
    """q1, q2 of DCMIP 1-1 at t0 on the ne2 mesh (the CPU restatement's initial state): the points sit on the curve to rounding, so
    l_r + l_u + l_o <= 1e-14; l_f is exactly 100 at every threshold that the field reaches (and 0.0, by definition, above its maximum)"""
    import pyoracle as po
    o = po.Oracle(2, 4)
    try:
        o.dcmip_init(1)
        Q = o.qdp[0] / dg.hybrid_dp(o.hyai, o.hybi, o.ps_v)[:, None]
        chi, xi = Q[:, 0].copy(), Q[:, 1].copy()
        lat, lon = o.lat.copy(), o.lon.copy()
        zm = dg.level_heights(o.hyam, o.hybm)
    finally:
        o.close()
    owner, colw, dh = dg.column_weights(2, lat, lon, zm)
    xmin, xmax = float(chi.min()), float(chi.max())
    assert xmin == 0.0 and 0.5 < xmax <= 1.0
    P = mm.element_partials(chi, xi, owner, colw, dh, xmin, xmax, 0.9, -0.8, TAU)
    got = from_partials(P)
    print("t0:", got)
    assert 0 <= got["l_r"] + got["l_u"] + got["l_o"] <= 1e-14 and got["d_max"] <= 1e-14
    reached = TAU <= xmax
    assert reached.sum() >= 10
    assert [f for f, r in zip(got["l_f"], reached) if r] == [100.0] * int(reached.sum())
    assert [f for f, r in zip(got["l_f"], reached) if not r] == [0.0] * int((~reached).sum())
    host = dg.mixing_diagnostics(2, lat, lon, chi, xi, zm, xmin, xmax, 0.9, -0.8, TAU)
    assert host["l_f"] == got["l_f"] and host["l_r"] + host["l_u"] + host["l_o"] <= 1e-14


@pytest.mark.parametrize("plant", ["slope", "ends", "swap"])
@pytest.mark.parametrize("ne", [2, 3])
def test_planted_errors_are_caught(ne, plant):
    """the chord's slope with the wrong sign, the end-point candidates left out, B and C exchanged: each leaves the summation bound against
    mixing_diagnostics; the missing end points also leave the bound on d against the referee"""
    c = mesh(ne)
    bad = from_partials(mm.element_partials(c["chi"], c["xi"], c["owner"], c["colw"], c["dh"], *c["par"], TAU, plant=plant))
    host = dg.mixing_diagnostics(ne, c["lat"], c["lon"], c["chi"], c["xi"], c["zm"], *c["par"], TAU)
    sb = mm.summation_bounds(c["owner"], c["nlev"])
    out = [k for k in ("l_r", "l_u", "l_o") if not close(bad[k], host[k], sb["l"])]
    print(plant, out, bad["counts"], host["counts"])
    assert out, (plant, bad, host)
    if plant == "ends":
        m = mm.constants(*c["par"])
        x, y = mm.families(m, TAU, np.random.default_rng(7))["outside, left"]
        assert (np.abs(mm.distance(m, x, y, plant="ends").astype(np.longdouble) - mm.referee_distance(m, x, y)) > D_BOUND).any()
    else:
        assert bad["counts"] != host["counts"] and bad["d_max"] == host["d_max"]


def test_an_element_without_an_owned_point_gives_zeros():
    c = mesh(2)
    owner = c["owner"].copy(); owner[5] = 0
    P = mm.element_partials(c["chi"], c["xi"], owner, c["colw"], c["dh"], *c["par"], TAU)
    assert not P[5].any() and P[4].any()
    rest = np.delete(np.arange(P.shape[0]), 5)
    a = dg.mixing_from_partials(P, P, np.arange(P.shape[0]), P.shape[0], ntau=TAU.size)
    b = dg.mixing_from_partials(P[rest], P[rest], np.arange(rest.size), rest.size, ntau=TAU.size)
    assert a == b
    # a threshold that nothing reaches at t0 gives 0.0, not a division by zero
    none = mm.element_partials(c["chi"], c["xi"], c["owner"], c["colw"], c["dh"], *c["par"], [1e9])
    assert from_partials(none, ntau=1)["l_f"] == [0.0]


# ---- bin/preqx --mixing ----
def test_the_mixing_argument_is_refused_for_dcmip12_and_for_one_tracer(tmp_path):
    from test_prim_main import NL
    ok = pm.settings(pm.parse_namelists(NL))
    pm.check_mixing(ok)
    for nl in (NL.replace('test_case = "dcmip1-1"', 'test_case = "dcmip1-2"'), NL.replace("qsize = 4", "qsize = 1")):
        assert nl != NL
        with pytest.raises(SystemExit, match="--mixing needs test_case = dcmip1-1 and qsize >= 2"):
            pm.check_mixing(pm.settings(pm.parse_namelists(nl)))
        f = tmp_path / "case.nl"
        f.write_text(nl)
        with pytest.raises(SystemExit, match="--mixing needs"):     # the front end ends there, before it touches a device
            pm.main(["--mixing", "--namelist", str(f)])
    lines = pm.mixing_lines(3, dict(l_r=1e-3, l_u=2e-4, l_o=0.0, l_f=[100.0, 99.5]), (0.10, 0.15))
    assert lines[0].startswith("mixing ") and lines[1].startswith("filament ") and "l_f(0.15)=99.5000" in lines[1]


# ---- the declarations (no GPU): header, loader, Fortran seam ----
SIG = ("int tse_mix_partials(tse_ctx *ctx, int nt, int qa, int qb, double xmin, double xmax, double c0, double c2, const double *tau, "
       "int ntau, double *out)")


def test_header_loader_and_libraries_declare_the_entry():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()).rstrip(";").strip() for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl.get("tse_mix_partials") == SIG
    assert "tse_mix_partials" in _lib.SYMBOLS
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):     # the 72-, 64- and 80-level libraries
        L = _lib.lib(nlev=nlev)
        assert hasattr(L, "tse_mix_partials") and len(L.tse_mix_partials.argtypes) == 11, nlev
    import ctypes as C
    assert hasattr(C.CDLL(_lib.HOOKS_SO), "tse_mix_partials")


def test_fortran_seam_has_the_wrapper():
    """(compiled by the two Fortran builds of the module; tests/fortran_resident/views_harness.F90 calls it on a GPU, test_gpu_fortran_views.py)"""
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert "name='tse_mix_partials'" in src
    assert re.search(r"subroutine\s+mix_partials_hip\s*\(\s*nt, qa, qb, xmin, xmax, c0, c2, tau, ntau, out\s*\)", src)
    assert re.search(r"public\s*::[^\n]*\bmix_partials_hip\b", src)
    body = src[src.index("subroutine mix_partials_hip"):src.index("end subroutine mix_partials_hip")]
    assert "call check(" in body and "qa-1" in body and "qb-1" in body
