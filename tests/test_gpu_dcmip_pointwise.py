"""-m gpu: the prescribed DCMIP 1-1 / 1-2 fields the device forms itself (k_dcmip_tables, k_dcmip_step, k_dcmip_init, tse_dcmip_init's host
part, the resident loop of tse_prim_run_subcycle) under the pointwise bound of tests/dcmip_ld.py, whose referee and bound
tests/test_dcmip_bound_cpu.py shows right (the CPU oracle under it) and sharp (five planted errors caught).

* Fields under the bound: the 72-, 64- and 80-level libraries, both test cases (qsize 6 and 3), ne2 and ne3; Qdp of both time levels, dp3d
  and ps_v after dcmip_init + dcmip_set_initial, the 0/1 tracers equal to the referee at every decided point; vn0, eta_dot_dpdn and dp after
  dcmip_step_inputs at steps on the zeros of the time factors, omega_p == 0.  The 64- and 80-level libraries run in a child process each
  (this file with --worker), so that one process never holds two level counts; a child returns its ratios.
* The static-inputs skip: a second dcmip_step_inputs leaves dp and omega_p alone (a value planted behind the library's back survives:
  k_dcmip_step's null-pointer path); after tse_invalidate_cache the next call writes them again, the same bits as the first.
* The resident loop: after prim_run_subcycle(tstep, 1, n) the device's vn0 is, bit for bit, that of a direct dcmip_step_inputs of the
  loop's last step on a second context, and so is eta_dot_dpdn once the second context has taken the same tracer step (the step's
  second stage replaces levels 1..nlev of eta_dot_dpdn by their DSS; the bottom interface is compared as the inputs left it).
* The factorisation: k_dcmip_step's factored evaluation against dcmip_point itself at every (column, level) -- tse_test_dcmip_point of
  the -DTSE_AB_HOOKS library, which the product libraries must not export."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

STEPS = {1: (1800.0, (0, 1, 2, 144, 145, 288, 289, 576, 577)), 2: (300.0, (0, 1, 144, 145, 288))}
QSIZE = {1: 6, 2: 3}
NES = (2, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# one library per process: what follows runs in this process for 72 levels and in a child for 64 and 80
def _hvcoord(nlev):
    import vcoord_levels as vl
    from transport_se_amd.hybvcoord import HvCoord
    return HvCoord() if nlev == 72 else HvCoord(*vl.paths(nlev))


def _context(ne, nlev, qsize, lib_path=None, nu_q=0.0):
    """a one-rank HipMod on the ne mesh (as test_gpu_nlev64._contexts_remap makes its own) -> (hip, lat, lon, hv)"""
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    hv = _hvcoord(nlev)
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    d = cm.edge_descriptors(topo, partition(ne, 1), 0)
    mine = d["elems"]
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, nu_q, lib_path=lib_path)
    assert h.nlev == nlev and h.L.tse_nlev() == nlev
    return h, np.ascontiguousarray(geo["lat"][mine]), np.ascontiguousarray(geo["lon"][mine]), hv


def _step_fields(h):
    n, nlev = h.nelemd, h.nlev
    return (h.fetch("vn0", (n, nlev, 2, 4, 4)), h.fetch("eta_dot_dpdn", (n, nlev + 1, 4, 4)), h.fetch("dp", (n, nlev, 4, 4)),
            h.fetch("omega_p", (n, nlev, 4, 4)))


def _measure(ne, nlev, test):
    """every ratio of one (mesh, level count, test case): dict(initial=[per time level [per slot dict]], dp3d=, ps_v=,
    steps={nstep: {field: ratio}}, omega_zero=)"""
    import dcmip_ld as dl
    from step_ld import ratio
    qsize = QSIZE[test]
    h, lat, lon, hv = _context(ne, nlev, qsize)
    vc = (hv.hyai, hv.hybi, hv.hyam, hv.hybm)
    ref, lev = dl.Referee(test, lat, lon, *vc), dl.fp64_levels(*vc)
    h.dcmip_init(test, lat, lon, hv.hyam, hv.hybm); h.dcmip_set_initial()
    n = h.nelemd
    qdp = h.fetch("qdp", (2, n, qsize, nlev, 4, 4))
    out = dict(initial=[dl.check_initial(ref, qsize, qdp[tl], lev["dph"]) for tl in (0, 1)],
               dp3d=ratio(h.fetch("dp3d", (n, nlev, 4, 4)), dl._lev(ref.L.dp))[0], ps_v=ratio(h.fetch("ps_v", (n, 4, 4)), ref.L.ps_v)[0],
               steps={}, omega_zero=True)
    tstep, steps = STEPS[test]
    for nstep in steps:
        h.dcmip_step_inputs(nstep, tstep)
        vn0, eta, dp, om = _step_fields(h)
        out["steps"][str(nstep)] = dl.check_step(ref, nstep, tstep, vn0, eta, dp)
        out["omega_zero"] = bool(out["omega_zero"] and not om.any())
    h.close()
    return out


def _measure_all(nlev):
    return {"%d/%d" % (ne, test): _measure(ne, nlev, test) for ne in NES for test in (1, 2)}


def _child(nlev, tmp_path, timeout=300):
    out = str(tmp_path / ("L%d.json" % nlev))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(nlev), out], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    with open(out) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_fields_under_the_bound(tmp_path, nlev):
    import dcmip_ld as dl
    from conftest import record_margin
    from step_ld import has_extended_precision
    assert has_extended_precision(), np.finfo(np.longdouble)
    res = _measure_all(nlev) if nlev == 72 else _child(nlev, tmp_path)
    bad = []
    for key, r in sorted(res.items()):
        ne, test = (int(x) for x in key.split("/"))
        tag = "[%d, %d, %d" % (ne, nlev, test)
        for tl, slots in enumerate(r["initial"]):
            assert len(slots) == QSIZE[test]
            for q, s in enumerate(slots):
                name = "dcmip-pointwise Qdp%d slot%d %s, 0]" % (tl + 1, q, tag)
                print("%-52s %.3g undecided %.3g wrong %d" % (name, s["ratio"], s["undecided"], s["wrong"]))
                record_margin(name, s["ratio"], 1.0)
                if not (s["ratio"] <= 1.0 and s["wrong"] == 0 and s["undecided"] <= dl.CAP):
                    bad.append((name, s))
        for f in ("dp3d", "ps_v"):
            name = "dcmip-pointwise %s %s, 0]" % (f, tag)
            print("%-52s %.3g" % (name, r[f]))
            record_margin(name, r[f], 1.0)
            if not r[f] <= 1.0:
                bad.append((name, r[f]))
        assert [int(k) for k in r["steps"]] == list(STEPS[test][1])
        worst = {}
        for nstep, fields in r["steps"].items():
            for f, x in fields.items():
                name = "dcmip-pointwise %s %s, %s]" % (f, tag, nstep)
                print("%-52s %.3g" % (name, x))
                record_margin(name, x, 1.0)
                worst[f] = max(worst.get(f, 0.0), x)
                if not x <= 1.0:
                    bad.append((name, x))
        for f, x in worst.items():
            record_margin("dcmip-pointwise %s %s, every step]" % (f, tag), x, 1.0)
        assert r["omega_zero"], key
    assert not bad, bad


def _poke(h, name, value):
    """write `value` over a whole device field behind the library's back"""
    import ctypes as C
    p, nbytes = h.device_ptr(name)
    x = np.full(nbytes // 8, value)
    h.synchronize()
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0


def test_static_inputs_are_written_once_and_again_after_invalidate():
    h, lat, lon, hv = _context(2, 72, 2)
    h.dcmip_init(1, lat, lon, hv.hyam, hv.hybm); h.dcmip_set_initial()
    h.dcmip_step_inputs(0, 1800.0)
    _, _, dp0, om0 = _step_fields(h)
    assert dp0.min() > 0 and not om0.any()
    h.dcmip_step_inputs(1, 1800.0)
    _, _, dp1, om1 = _step_fields(h)
    assert np.array_equal(dp0.view(np.uint64), dp1.view(np.uint64)) and np.array_equal(om0.view(np.uint64), om1.view(np.uint64))
    _poke(h, "dp", -7.0); _poke(h, "omega_p", 3.0)
    h.dcmip_step_inputs(2, 1800.0)                       # the null-pointer path: neither field is written
    _, _, dp2, om2 = _step_fields(h)
    assert (dp2 == -7.0).all() and (om2 == 3.0).all()
    h.invalidate_cache()
    h.dcmip_step_inputs(3, 1800.0)
    _, _, dp3, om3 = _step_fields(h)
    assert np.array_equal(dp0.view(np.uint64), dp3.view(np.uint64)) and np.array_equal(om0.view(np.uint64), om3.view(np.uint64))
    h.close()


@pytest.mark.parametrize("n", [0, 4])
def test_resident_loop_forms_the_inputs_of_its_last_step(n):
    """prim_run_subcycle(tstep, 1, n) ends the rsplit cycle that holds step n: from n = 4 (inside a cycle, rsplit 3) it takes steps 4 and
    5 and returns 6, so the inputs left on the device are those of step (returned count) - 1 -- n + rsplit - 1 only when n starts a cycle"""
    tstep, rsplit = 1800.0, 3
    a, lat, lon, hv = _context(2, 72, 4, nu_q=1e19)
    b, _, _, _ = _context(2, 72, 4, nu_q=1e19)
    for h in (a, b):
        h.dcmip_init(1, lat, lon, hv.hyam, hv.hybm); h.dcmip_set_initial()
    end = a.prim_run_subcycle(tstep, 1, n)
    assert end == n - n % rsplit + rsplit
    last = end - 1
    vn0_a, eta_a, _, _ = _step_fields(a)
    b.dcmip_step_inputs(last, tstep)
    vn0_b, eta_b, _, _ = _step_fields(b)
    assert np.array_equal(vn0_a.view(np.uint64), vn0_b.view(np.uint64))
    assert np.array_equal(eta_a[:, 72].view(np.uint64), eta_b[:, 72].view(np.uint64))
    n0 = 1 if last % 2 == 0 else 2
    b.advec_tracers_remap_rk2(tstep, n0, 3 - n0)           # the step DSSes levels 1..nlev of eta_dot_dpdn in place
    _, eta_b, _, _ = _step_fields(b)
    assert np.array_equal(eta_a.view(np.uint64), eta_b.view(np.uint64))
    a.close(); b.close()


def _ulps(x, y):
    """the distance of two fp64 arrays in units in the last place (sign-magnitude order)"""
    def key(v):
        i = np.ascontiguousarray(v).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i).astype(np.float64)
    return np.abs(key(x) - key(y))


@pytest.mark.parametrize("test", [1, 2])
@pytest.mark.parametrize("ne", NES)
def test_factored_evaluation_against_dcmip_point(ne, test):
    """k_dcmip_step (level, column and time factors multiplied) against dcmip_point itself at every (column, level), 72 levels: the same
    bits, as the header comment of k_dcmip_tables states"""
    from conftest import record_margin
    from transport_se_amd import _lib
    h, lat, lon, hv = _context(ne, 72, QSIZE[test], lib_path=_lib.HOOKS_SO)
    h.dcmip_init(test, lat, lon, hv.hyam, hv.hybm)
    tstep, steps = STEPS[test]
    worst = 0.0
    for nstep in steps:
        h.dcmip_step_inputs(nstep, tstep)
        vn0, eta, _, _ = _step_fields(h)
        vn0_p, eta_p = h.test_dcmip_point(nstep, tstep)
        assert np.abs(vn0_p).max() > 0 and np.abs(eta_p).max() > 0
        du, de = _ulps(vn0, vn0_p), _ulps(eta, eta_p)
        print("ne%d test %d nstep %3d: vn0 differs at %d of %d by at most %g ulp, eta_dot_dpdn at %d of %d by at most %g ulp"
              % (ne, test, nstep, (du > 0).sum(), du.size, du.max(), (de > 0).sum(), de.size, de.max()))
        worst = max(worst, du.max(), de.max())
        assert np.array_equal(vn0.view(np.uint64), vn0_p.view(np.uint64)) and np.array_equal(eta.view(np.uint64), eta_p.view(np.uint64)), nstep
    record_margin("dcmip-pointwise factored vs dcmip_point ulps [%d, 72, %d]" % (ne, test), worst, 0.0)
    h.close()
    assert worst == 0.0, worst


def test_the_product_libraries_have_no_point_entry():
    from transport_se_amd import _lib
    assert hasattr(_lib.lib(_lib.HOOKS_SO), "tse_test_dcmip_point")
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        assert not hasattr(_lib.lib(nlev=nlev), "tse_test_dcmip_point"), nlev


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    with open(sys.argv[3], "w") as f:
        json.dump(_measure_all(int(sys.argv[2])), f)
