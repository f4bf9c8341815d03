"""-m gpu: tracer transport with the clip-and-sum limiter (limiter_option = 9), on every route of the library.

The reference model is tests/limiter9_model.py (limiter 8's bounds, the clip-and-sum slab routine with serial sums) inside
tests/unlimited_model.py's euler_step; test_limiter9_cpu.py shows that it differs from limiter 8 and from the unlimited step, that it has
work in every stage, conserves mass and keeps the bounds.  Here:
* against the model: every stage of the per-stage API with the relaxed bounds tse_get_qminmax shows (ne2, ne4), the whole-step call and
  two prim_run_subcycle cycles.  Tolerance: the project's Q_TOL / Q_TOL_CYCLES -- the operator chain around the limiter is the one that
  holds limiter 8 and the unlimited route to them, and the model run with the kernel's tree sums, reciprocal and c*x output order
  instead of the serial form moves by at most 7.8e-15 (the uniform base; about 1e-15 on the others);
* exact: slot invariance (qsize 1, 5, 9); 2 and 3 emulated ranks, TSE_BOUNDARY_STRIPS=1 and TSE_REMAP_FUSED=0 equal the one-context
  default run; the outputs that do not depend on tracers equal a limiter-8 run's;
* it is option 9: the noise field differs from a limiter-8 and from an unlimited run; a limiter-8 context created after a limiter-9
  context gives the bits of a limiter-8 run in a fresh process;
* the 64- and 80-level libraries (the limiter does not see the level count): finite output and conserved mass.  A
  prim_run_subcycle cycle ends with the vertical remap, which moves mass between levels, so the mass of every level is held to 1e-13
  over a whole tracer step (no remap) and the mass of every tracer, summed over the levels, to 1e-13 over one cycle;
* bin/preqx runs a namelist with limiter_option = 9 to its norm line, with other digits than with 8."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NOISE = 1              # tracer_fields.BASE_NAMES.index("noise")
CONTINUOUS = [0, 3, 4, 5]   # as test_unlimited_cpu.py: the base fields that are single-valued on element edges
STAGES = ((2, 1, 3, 0), (2, 2, 1, 1), (2, 2, 2, 2))   # (np1_qdp, n0_qdp, dssopt, rhs_multiplier)


def _check(name, got, ref, dp, tol):
    from conftest import record_margin
    from tracer_fields import BASE_NAMES, NBASE, q_err
    err, (q, k, e) = q_err(np.array(got), np.array(ref), np.array(dp))
    for i, x in enumerate(err):
        record_margin("q_err limiter9 %s %s" % (name, BASE_NAMES[i % NBASE]), x, tol)
    print("limiter9 %s: q_err %s" % (name, ["%.2e" % x for x in err]))
    assert np.all(err <= tol), (name, err.tolist(), "worst: tracer %d level %d element %d" % (q, k, e))


@pytest.mark.parametrize("ne", [2, 4])
def test_per_stage_api_vs_model(ne):
    """tse_euler_step (plain kernels with the clip-and-sum limiter, one DSS pass per stage) after each of the three stages -- Qdp and the
    relaxed bounds -- then tse_qdp_time_avg"""
    import pyoracle as po
    import test_gpu_unlimited as gu
    import unlimited_model as um
    from conftest import record_margin
    from gpu_common import elem_from_oracle, make_hip
    from limiter9_model import Limiter9
    from tracer_fields import NBASE, base_tracers
    nu, dt = gu._params(ne)
    o = po.Oracle(ne, NBASE, nu_q=nu)
    elem = elem_from_oracle(o)
    hip = make_hip(o, elem, limiter_option=9)
    lim = Limiter9(o)
    try:
        o.dcmip_init(1); o.dcmip_step_inputs(1, 0, dt)
        gu._load(o, elem, hip, base_tracers(o)); gu._inputs(o, elem, hip)
        hip.compute_divdp()
        for e in range(o.nelem):
            for k in range(72):
                o.divdp[e, k] = o.divergence_sphere(e, o.vn0[e, k])
        o.divdp_proj[...] = o.divdp
        for (np1, n0, dss, rhs) in STAGES:
            um.euler_step(o, np1, n0, dt / 2, dss, rhs, limiter=lim)
            hip.euler_step(np1, n0, dt / 2, dss, rhs)
            hip.copy_qdp_d2h(elem, 2)
            _check("ne%d euler_step rhs=%d" % (ne, rhs), elem["Qdp"][:, 1], o.qdp[1], o.dp, gu.Q_TOL)
            assert lim.clipped >= 1 and lim.relaxed >= 1, (rhs, lim.slabs, lim.clipped, lim.relaxed)   # (the model's limiter had work)
            qmin, qmax = hip.get_qminmax()
            scale = max(np.abs(lim.mn).max(), np.abs(lim.mx).max())
            berr = max(np.abs(qmin - lim.mn).max(), np.abs(qmax - lim.mx).max()) / scale
            record_margin("limiter9 ne%d relaxed bounds rhs=%d" % (ne, rhs), berr, 1e-13)
            print("limiter9 ne%d rhs=%d: bounds err %.2e" % (ne, rhs, berr))
            assert berr <= 1e-13, (rhs, berr)
        o.qdp[1] = (o.qdp[0] + 2.0 * o.qdp[1]) / 3.0
        hip.qdp_time_avg(3, 1, 2)
        hip.copy_qdp_d2h(elem, 2)
        _check("ne%d qdp_time_avg" % ne, elem["Qdp"][:, 1], o.qdp[1], o.dp, gu.Q_TOL)
    finally:
        hip.close(); o.close()


def test_whole_step_and_subcycle_vs_model():
    """tse_advec_tracers_remap_rk2 (DSS on read) x6 + 2 remaps on the model's inputs, and two prim_run_subcycle cycles with the fused
    remap and with TSE_REMAP_FUSED=0"""
    import limiter9_model as l9
    import pyoracle as po
    import test_gpu_unlimited as gu
    import unlimited_model as um
    from gpu_common import elem_from_oracle, make_hip
    from tracer_fields import NBASE, base_tracers, layer_dp
    nu, dt = gu._params(2)
    o = po.Oracle(2, NBASE, nu_q=nu)
    elem = elem_from_oracle(o)
    hip = make_hip(o, elem, limiter_option=9)
    lim = l9.Limiter9(o)
    try:
        o.dcmip_init(1)
        b = base_tracers(o)
        gu._load(o, elem, hip, b)
        nstep = 0
        for sub in range(2):
            for r in range(3):
                o.dcmip_step_inputs(1, nstep, dt); gu._inputs(o, elem, hip)
                n0 = 1 if nstep % 2 == 0 else 2
                hip.advec_tracers_remap_rk2(dt, n0, 3 - n0); um.advec_tracers_remap_rk2(o, dt, nstep, lim)
                if nstep == 0:
                    hip.copy_qdp_d2h(elem, 2)
                    _check("advec_tracers_remap_rk2", elem["Qdp"][:, 1], o.qdp[1], o.dp - dt * o.divdp_proj, gu.Q_TOL)
                nstep += 1
            hip.vertical_remap(3 * dt, 3 - n0); assert o.vertical_remap(3 * dt, 3 - n0) == 0
        hip.copy_qdp_d2h(elem, 1)
        _check("per-step x6 + 2 remaps", elem["Qdp"][:, 0], o.qdp[0], layer_dp(o.hyai, o.hybi, o.ps_v), gu.Q_TOL_CYCLES)
        ref = None
        for fused in ("1", "0"):
            with gu._env(TSE_REMAP_FUSED=fused):
                hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm); hip.dcmip_set_initial()
                gu._load(o, elem, hip, b)
                assert hip.prim_run_subcycle(dt, 2, 0) == 6
                hip.copy_qdp_d2h(elem, 1)
            if ref is None:   # the model's two cycles, computed once and left unchanged
                o.dcmip_init(1)
                o.qdp[0] = np.moveaxis(b, 0, 1); o.qdp[1] = o.qdp[0]
                assert l9.prim_run(o, 1, dt, 2, lim) == (6, 6)
                ref = (o.qdp[0].copy(), layer_dp(o.hyai, o.hybi, o.ps_v))
            _check("prim_run_subcycle x2 fused=%s" % fused, elem["Qdp"][:, 0], ref[0], ref[1], gu.Q_TOL_CYCLES)
    finally:
        hip.close(); o.close()


@pytest.fixture(scope="module")
def cycle_runs():
    """one prim_run_subcycle cycle at ne2 on the six base fields with limiter 9, then 8 (created after the limiter-9 context), then 0:
    Qdp and the tracer-independent outputs of each"""
    import test_gpu_unlimited as gu
    from tracer_fields import NBASE, base_tracers
    names = dict(divdp=(72,), divdp_proj=(72,), eta_dot_dpdn=(73,), omega_p=(72,), dp3d=(72,), ps_v=())
    out = {}
    for lim in (9, 8, 0):
        r = gu.Run(2, NBASE, lim)
        try:
            qdp = r.cycles(base_tracers(r.o), nsub=1)
            out[lim] = {k: r.hip.fetch(k, (r.o.nelem,) + s + (4, 4)).copy() for k, s in names.items()}
            out[lim]["qdp"] = qdp
            out[lim]["dp"] = r.hip.fetch("dp3d", (r.o.nelem, 72, 4, 4)).copy()
        finally:
            r.close()
    out["names"] = list(names)
    return out


def test_tracer_independent_outputs_equal_a_limiter_8_run(cycle_runs):
    import test_gpu_unlimited as gu
    for k in cycle_runs["names"]:
        assert np.array_equal(gu._bits(cycle_runs[9][k]), gu._bits(cycle_runs[8][k])), k


def test_is_really_option_9(cycle_runs):
    """on the 0/1 noise field the run differs from a limiter-8 run and from an unlimited run of the same state by more than 1e-6"""
    from tracer_fields import q_err
    got = cycle_runs[9]["qdp"][1]
    assert np.isfinite(got).all()
    for other in (8, 0):
        err, _ = q_err(got, cycle_runs[other]["qdp"][1], cycle_runs[9]["dp"])
        print("limiter 9 vs %d after one cycle: q_err %s" % (other, ["%.2e" % x for x in err]))
        assert err[NOISE] > 1e-6, (other, err.tolist())


def test_limiter_8_after_limiter_9_is_a_fresh_limiter_8_run(cycle_runs, tmp_path):
    """the limiter-8 context of cycle_runs was created after a limiter-9 context in this process: the bits of a limiter-8 run in a
    process of its own"""
    import test_gpu_unlimited as gu
    fresh = _child(dict(kind="fresh8"), tmp_path)
    assert np.array_equal(gu._bits(cycle_runs[8]["qdp"]), gu._bits(fresh["qdp"]))


def test_slot_invariance():
    """every slot holds the bits of its base field's run alone (qsize 1), at qsize 5 and 9"""
    import test_gpu_unlimited as gu
    from tracer_fields import BASE_NAMES, NBASE, base_tracers, slot_bases
    r = gu.Run(2, 1, 9)
    try:
        b = base_tracers(r.o)
        single = [r.cycles(b[i:i + 1]) for i in range(NBASE)]
    finally:
        r.close()
    for qsize in (5, 9):
        r = gu.Run(2, qsize, 9)
        try:
            sb = slot_bases(qsize)
            got = r.cycles(base_tracers(r.o)[sb])
            bad = [(s, BASE_NAMES[x]) for s, x in enumerate(sb) if not np.array_equal(gu._bits(got[:, :, s]), gu._bits(single[x][:, :, 0]))]
            assert not bad, (qsize, bad)
        finally:
            r.close()


def test_emulated_ranks_boundary_strips_and_unfused_remap_equal_one_context():
    """2 and 3 contexts (split boundary/interior launches, callback exchange), TSE_BOUNDARY_STRIPS=1 on 3 and TSE_REMAP_FUSED=0 give the
    one-context default run, bit for bit; the bounds are exchanged (kind 1) as with limiter 8"""
    import test_gpu_unlimited as gu
    kinds = set()
    with gu._env():
        one = gu._emulated(1, 4, 3, 9, kinds)
        assert np.isfinite(one).all() and one.max() > 0
        for world in (2, 3):
            assert np.array_equal(gu._bits(gu._emulated(world, 4, 3, 9, kinds)), gu._bits(one)), world
    assert kinds == {0, 1}, kinds
    with gu._env(TSE_BOUNDARY_STRIPS="1"):
        assert np.array_equal(gu._bits(gu._emulated(3, 4, 3, 9, kinds)), gu._bits(one))
    with gu._env(TSE_REMAP_FUSED="0"):
        assert np.array_equal(gu._bits(gu._emulated(1, 4, 3, 9, kinds)), gu._bits(one))


# ---------------------------------------------------------------------------------------------------------------------------
# child processes: one library per process (the 64- and 80-level builds), and the fresh limiter-8 run
def _nlev_job(nlev):
    """the library built for `nlev` levels at ne2, limiter 9, the four continuous base fields on the grid's own levels: a whole tracer
    step (no remap) and one prim_run_subcycle cycle"""
    import tracer_fields as tf
    import vcoord_levels as vl
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    ne, dt, nu = 2, 1800.0, 1e19
    hv = HvCoord(*vl.paths(nlev))
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    d = cm.edge_descriptors(topo)   # one rank: every element, in mesh order
    assert np.array_equal(d["elems"], np.arange(6 * ne * ne))
    n, qsize = 6 * ne * ne, len(CONTINUOUS)
    elem = dict(Dinv=geo["Dinv"], metdet=geo["metdet"], rmetdet=geo["rmetdet"], spheremp=geo["spheremp"], rspheremp=geo["rspheremp"],
                putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, nu, limiter_option=9, device=0, schedule=dict(send=d["send"], recv=d["recv"]))
    assert h.nlev == nlev and h.L.tse_nlev() == nlev
    tf.NLEV = nlev   # base_mixing_ratios builds its fields on tracer_fields.NLEV levels (this process serves one level count)
    Q = tf.base_mixing_ratios(geo["lat"], geo["lon"], np.random.default_rng(20261015))[CONTINUOUS]
    out = {}

    def start():
        h.dcmip_init(1, geo["lat"], geo["lon"], hv.hyam, hv.hybm); h.dcmip_set_initial(); h.dcmip_step_inputs(0, dt)
        qdp = np.moveaxis(Q * h.fetch("dp", (n, nlev, 4, 4))[None], 0, 1)
        elem["Qdp"] = np.ascontiguousarray(np.stack([qdp, qdp], axis=1))
        h.copy_qdp_h2d(elem, 1); h.copy_qdp_h2d(elem, 2)
        return qdp
    out["step_in"] = start()
    h.advec_tracers_remap_rk2(dt, 1, 2)
    out["step_out"] = h.fetch("qdp", (2, n, qsize, nlev, 4, 4))[1].copy()
    out["cycle_in"] = start()
    h.dcmip_init(1, geo["lat"], geo["lon"], hv.hyam, hv.hybm); h.dcmip_set_initial()
    h.copy_qdp_h2d(elem, 1); h.copy_qdp_h2d(elem, 2)
    assert h.prim_run_subcycle(dt, 1, 0) == 3
    out["cycle_out"] = h.fetch("qdp", (2, n, qsize, nlev, 4, 4))[1].copy()   # (3 steps from nstep 0 end in time level 2)
    out["spheremp"] = geo["spheremp"]
    h.close()
    return out


def _fresh8_job():
    import test_gpu_unlimited as gu
    from tracer_fields import NBASE, base_tracers
    r = gu.Run(2, NBASE, 8)
    try:
        return dict(qdp=r.cycles(base_tracers(r.o), nsub=1))
    finally:
        r.close()


def _worker(spec):
    out = _nlev_job(spec["nlev"]) if spec["kind"] == "nlev" else _fresh8_job()
    np.savez(spec["out"], **out)


def _child_env():
    env = dict(os.environ)
    for k in ("TSE_REMAP_FUSED", "TSE_BOUNDARY_STRIPS", "TSE_DSS_ON_READ", "TSE_LIB", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    return env


def _child(spec, tmp_path, timeout=300):
    out = str(tmp_path / "r.npz")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(spec, out=out))], env=_child_env(), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(tmp_path, nlev):
    res = _child(dict(kind="nlev", nlev=nlev), tmp_path)
    sp = res["spheremp"]

    def mass(x, f=lambda y: y):
        return np.einsum("eqkji,eji->qk", f(x), sp)
    for key in ("step_out", "cycle_out"):
        assert res[key].shape[2] == nlev and np.isfinite(res[key]).all() and np.abs(res[key]).max() > 0, key
        assert not np.array_equal(res[key], res[key.replace("out", "in")])
    rel = np.abs(mass(res["step_out"]) - mass(res["step_in"])) / np.maximum(mass(res["step_out"], np.abs), 1e-300)
    print("limiter 9, %d levels: per-level mass error of a tracer step %.2e" % (nlev, rel.max()))
    assert rel.max() < 1e-13, rel.max()
    col = np.abs(mass(res["cycle_out"]).sum(1) - mass(res["cycle_in"]).sum(1)) / np.maximum(mass(res["cycle_out"], np.abs).sum(1), 1e-300)
    print("limiter 9, %d levels: tracer mass error of a prim_run_subcycle cycle %s" % (nlev, col.tolist()))
    assert col.max() < 1e-13, col.tolist()


NL9 = """
&ctl_nl
  test_case = "dcmip1-1"
  ne = 8
  qsize = 4
  nmax = 6
  statefreq = 3
  tstep = 400
  qsplit = 1, rsplit = 3
  nu_q = 6e16
  limiter_option = 9
/
&vert_nl
  vform = "ccm"
/
"""


def test_preqx_runs_a_namelist_with_limiter_option_9(tmp_path):
    """the ne8, qsize 4, six-step namelist of the other preqx tests with limiter_option = 9 runs to its norm line, whose digits differ
    from the same run with 8"""
    norm = {}
    for lim in (9, 8):
        res = subprocess.run([os.path.join(ROOT, "bin", "preqx")], input=NL9.replace("limiter_option = 9", "limiter_option = %d" % lim).encode(),
                             cwd=str(tmp_path), env=_child_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = res.stdout.decode()
        assert res.returncode == 0, out[-3000:]
        lines = [l for l in out.splitlines() if l.startswith("DCMIP 1-1:")]
        assert lines, out[-2000:]
        norm[lim] = lines[-1]
        for l in [l for l in out.splitlines() if l.startswith("Q") and "relative change" in l]:
            assert abs(float(l.split("relative change")[1].strip(" )"))) < 1e-11, l
    print(norm)
    assert norm[9] != norm[8], norm


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    _worker(json.loads(sys.argv[2]))
