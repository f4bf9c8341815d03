"""The longdouble referee of the prescribed DCMIP fields and its pointwise bound (dcmip_ld.py), without a GPU.

* The bound is right: pyoracle's dcmip_init and dcmip_step_inputs, both test cases, lie under it at every point of ne2 and ne3, at steps
  chosen on the zeros of the time factors (cos(2 pi t/tau) at a quarter period, cos(pi t/tau) of 1-2 at half a period); so does an fp64
  numpy restatement of the same texts on the 72-, 64- and 80-level files (the oracle is a 72-level library).
* The bound is sharp: five planted errors, each of a kind a kernel could make, break it -- and the second passes the field-maximum
  check that test_gpu_parity.py applies.
* The 0/1 fields: at most 1 point in 1000 undecided per field, mesh and level file (ne2 to ne4; 72, 64, 80 levels), and every decided
  value of the oracle / the restatement is the referee's.
* The level constants zm, zi, pint, dph of tse_dcmip_init's host part, evaluated in Python, under their triples.
* The counts of dcmip_ld's docstring are the ones its code arrives at."""
import numpy as np
import pytest

import dcmip_ld as dl
import pyoracle as po
import step_ld as sl
import vcoord_levels as vl
from conftest import record_margin
from transport_se_amd.hybvcoord import HvCoord

pytestmark = pytest.mark.skipif(not sl.has_extended_precision(), reason="np.longdouble has no 64-bit mantissa here")

STEPS = {1: (1800.0, (0, 1, 2, 144, 145, 288, 289, 576, 577)), 2: (300.0, (0, 1, 144, 145, 288))}
QSIZE = 6
NLEVS = (72, 64, 80)


def vcoord(nlev):
    if nlev == 72:
        return po.read_vcoord()
    hv = HvCoord(*vl.paths(nlev))
    return hv.hyai, hv.hybi, hv.hyam, hv.hybm


@pytest.fixture(scope="module")
def oracles():
    os_ = {ne: po.Oracle(ne, QSIZE) for ne in (2, 3, 4)}
    yield os_
    for o in os_.values():
        o.close()


_refs = {}


def referee(o, test, nlev):
    key = (o.ne, test, nlev)
    if key not in _refs:
        _refs[key] = dl.Referee(test, o.lat, o.lon, *vcoord(nlev))
    return _refs[key]


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _assert_initial(res, name):
    for q, s in enumerate(res):
        print("%-44s slot %d ratio %.3g undecided %.3g wrong %d" % (name, q, s["ratio"], s["undecided"], s["wrong"]))
        record_margin("%s slot%d" % (name, q), s["ratio"], 1.0)
        assert s["ratio"] <= 1.0 and s["wrong"] == 0 and s["undecided"] <= dl.CAP, (name, q, s)


def test_counts():
    """the rounding counts of dcmip_ld's docstring"""
    o = po.Oracle(2, 1)
    try:
        r1, r2 = dl.Referee(1, o.lat, o.lon, *vcoord(72)), dl.Referee(2, o.lat, o.lon, *vcoord(72))
    finally:
        o.close()
    L = r1.L
    assert (L.H.m, L.zi.m, L.zm.m, L.pint.m, L.ps_v.m, L.dph.m, L.dp.m) == (3, 9, 9, 18, 18, 21, 19)
    i1, i2 = r1.step_inputs(3, 1800.0), r2.step_inputs(3, 300.0)
    assert (i1["u"].m, i1["v"].m, i1["w"].m, i1["rho"].m, i1["eta"].m) == (84, 28, 89, 21, 112)
    assert (i2["u"].m, i2["v"].m, i2["w"].m, i2["rho"].m, i2["eta"].m) == (5, 69, 68, 21, 91)
    t = r1.tracers1()
    assert (t["d1"].m, t["q1"].m, t["q2"].m, t["q4"].m) == (56, 63, 129, 133)
    assert r2.tracer2()[0].m == 19
    assert r1._levels1(dl._lev(L.zi))["s"].m == 37


# ---- the bound is right ----
@pytest.mark.parametrize("test", [1, 2])
@pytest.mark.parametrize("ne", [2, 3])
def test_oracle_is_under_the_bound(oracles, ne, test):
    o = oracles[ne]
    ref = referee(o, test, 72)
    lev = dl.fp64_levels(*vcoord(72))
    o.dcmip_init(test)
    for tl in (0, 1):
        _assert_initial(dl.check_initial(ref, QSIZE, o.qdp[tl], lev["dph"]), "dcmip-pointwise cpu-oracle Qdp%d [%d, 72, %d]" % (tl + 1, ne, test))
    worst = {"dp3d": sl.ratio(o.dp3d, dl._lev(ref.L.dp))[0], "ps_v": sl.ratio(o.ps_v, ref.L.ps_v)[0]}
    tstep, steps = STEPS[test]
    for nstep in steps:
        o.dcmip_step_inputs(test, nstep, tstep)
        assert not o.omega_p.any()
        for f, r in dl.check_step(ref, nstep, tstep, o.vn0, o.eta_dot_dpdn, o.dp).items():
            print("cpu-oracle %-13s [%d, 72, %d, %3d] %.3g" % (f, ne, test, nstep, r))
            worst[f] = max(worst.get(f, 0.0), r)
    for f, r in worst.items():
        record_margin("dcmip-pointwise cpu-oracle %s [%d, 72, %d]" % (f, ne, test), r, 1.0)
    print("worst ratios", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("test", [1, 2])
@pytest.mark.parametrize("nlev", NLEVS)
def test_fp64_restatement_is_under_the_bound(oracles, nlev, test):
    """the numpy restatement (the carrier of the planted errors) on all three level files: the 12 km tops of the 64- and 80-level files
    put plim = fmax(p, ptop) and hstar = fmin(z/ztop, 1) on the grid"""
    o = oracles[2]
    ref = referee(o, test, nlev)
    lev = dl.fp64_levels(*vcoord(nlev))
    _assert_initial(dl.check_initial(ref, QSIZE, dl.fp64_initial(test, QSIZE, o.lat, o.lon, lev), lev["dph"]),
                    "dcmip-pointwise cpu-restatement Qdp [2, %d, %d]" % (nlev, test))
    tstep, steps = STEPS[test]
    worst = {}
    for nstep in steps:
        got = dl.fp64_step_inputs(test, nstep, tstep, o.lat, o.lon, lev)
        for f, r in dl.check_step(ref, nstep, tstep, got["vn0"], got["eta"], got["dp"]).items():
            worst[f] = max(worst.get(f, 0.0), r)
    for f, r in worst.items():
        record_margin("dcmip-pointwise cpu-restatement %s [2, %d, %d]" % (f, nlev, test), r, 1.0)
    print("worst ratios", worst)
    assert max(worst.values()) <= 1.0, worst


# ---- the bound is sharp ----
def test_planted_bs_in_double(oracles):
    """1. bs = 0.2 in double in place of the single-precision literal"""
    o = oracles[2]
    ref, lev = referee(o, 1, 72), dl.fp64_levels(*vcoord(72))
    got = dl.fp64_step_inputs(1, 1, 1800.0, o.lat, o.lon, lev, bs=0.2)
    r = dl.check_step(ref, 1, 1800.0, got["vn0"], got["eta"], got["dp"])
    print(r)
    assert r["vn0-u"] > 1.0 and r["eta_dot_dpdn"] > 1.0 and r["vn0-v"] <= 1.0, r


def test_planted_scaling_of_small_eta_passes_the_max_norm(oracles):
    """2. eta_dot_dpdn times 1 + 1e-10 where its magnitude is below 1e-4 of the field maximum: the pointwise bound breaks, relerr < 1e-12
    (test_gpu_parity.py's check) does not notice"""
    o = oracles[2]
    ref = referee(o, 1, 72)
    o.dcmip_step_inputs(1, 1, 1800.0)
    eta = o.eta_dot_dpdn.copy()
    small = np.abs(eta) < 1e-4 * np.abs(eta).max()
    assert small.any() and not small.all()
    bad = np.where(small, eta * (1.0 + 1e-10), eta)
    assert relerr(bad, eta) < 1e-12
    r0 = dl.check_step(ref, 1, 1800.0, o.vn0, eta, o.dp)["eta_dot_dpdn"]
    r1 = dl.check_step(ref, 1, 1800.0, o.vn0, bad, o.dp)["eta_dot_dpdn"]
    print(r0, r1)
    assert r0 <= 1.0 < r1


def test_planted_v_at_t_now(oracles):
    """3. v of 1-1 evaluated at t_now in place of t_wind"""
    o = oracles[2]
    ref, lev = referee(o, 1, 72), dl.fp64_levels(*vcoord(72))
    for nstep in (1, 145):
        got = dl.fp64_step_inputs(1, nstep, 1800.0, o.lat, o.lon, lev, v_at_now=True)
        r = dl.check_step(ref, nstep, 1800.0, got["vn0"], got["eta"], got["dp"])
        print(nstep, r)
        assert r["vn0-v"] > 1.0 and r["vn0-u"] <= 1.0 and r["eta_dot_dpdn"] <= 1.0, r


def test_planted_checkerboard_le(oracles):
    """4. the checkerboard with <= in place of <: exactly the +-0 columns of ne2 flip, each a decided point"""
    o = oracles[2]
    ref, lev = referee(o, 1, 72), dl.fp64_levels(*vcoord(72))
    good = dl.fp64_initial(1, QSIZE, o.lat, o.lon, lev)
    bad = dl.fp64_initial(1, QSIZE, o.lat, o.lon, lev, checker_le=True)
    zero_cols = (np.sin(9.0 * o.lon) * np.sin(9.0 * o.lat)) == 0.0
    assert zero_cols.sum() == 96                                     # of 384 columns
    flipped = (good[:, 4] != bad[:, 4]).any(axis=1)
    assert np.array_equal(flipped, zero_cols)
    res = dl.check_initial(ref, QSIZE, bad, lev["dph"])
    assert [s["wrong"] for s in res] == [0, 0, 0, 0, 96 * 72, 96 * 72]
    assert res[4]["ratio"] > 1.0 and res[5]["ratio"] > 1.0 and max(s["ratio"] for s in res[:4]) <= 1.0


def test_planted_w_table_of_the_interface_below(oracles):
    """5. w of 1-2 with the level factors of interface k + 1 at the top three interfaces (the 64-level file: on the 72-level one the
    top interfaces all lie above 12 km, where fmax and fmin make those factors equal)"""
    o = oracles[2]
    ref, lev = referee(o, 2, 64), dl.fp64_levels(*vcoord(64))
    got = dl.fp64_step_inputs(2, 1, 300.0, o.lat, o.lon, lev, w_table_shift=3)
    r = dl.check_step(ref, 1, 300.0, got["vn0"], got["eta"], got["dp"])
    print(r)
    assert r["eta_dot_dpdn"] > 1.0 and max(r["vn0-u"], r["vn0-v"], r["dp"]) <= 1.0, r


# ---- decisions ----
@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("ne", [2, 3, 4])
def test_undecided_counts_and_decided_values(oracles, ne, nlev):
    o = oracles[ne]
    lev = dl.fp64_levels(*vcoord(nlev))
    for test in (1, 2):
        ref = referee(o, test, nlev)
        if nlev == 72:
            o.dcmip_init(test)
            qdp = o.qdp[0]
        else:
            qdp = dl.fp64_initial(test, QSIZE, o.lat, o.lon, lev)
        for q, s in enumerate(dl.check_initial(ref, QSIZE, qdp, lev["dph"])):
            assert s["undecided"] <= dl.CAP and s["wrong"] == 0 and s["ratio"] <= 1.0, (ne, nlev, test, q, s)
        if test == 1:
            t = ref.tracers1()
            margin = min(float(np.abs(t[d].v - 0.5).min()) for d in ("d1", "d2"))
            print("ne%d nlev%d: smallest |d - RR| %.3g, undecided q3 %d, checker %d" % (ne, nlev, margin, (~t["decided"]).sum(), (~ref.checker()[1]).sum()))


# ---- level constants ----
@pytest.mark.parametrize("nlev", NLEVS)
def test_level_constants_under_their_triples(nlev):
    vc = vcoord(nlev)
    lev, L = dl.fp64_levels(*vc), dl.Levels(*vc)
    for name, t in (("zm", L.zm), ("zi", L.zi), ("pint", L.pint), ("dph", L.dph), ("dp", L.dp)):
        r = sl.ratio(lev[name], t)[0]
        record_margin("dcmip-pointwise cpu level constant %s [%d]" % (name, nlev), r, 1.0)
        print(name, nlev, r)
        assert r <= 1.0, (name, r)
    assert lev["zi"][nlev] == 0.0 and lev["pint"][nlev] == dl.P0       # eta = 1 at the surface
